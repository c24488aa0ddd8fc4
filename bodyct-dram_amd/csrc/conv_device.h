// Device helpers shared by the convolution kernels (conv3d_k3*.hip, conv3d_gen.hip): vector types, buffer (SRD) loads,
// wave-uniform pointers, the XCD-aware block order and the multiply + shift division.
#pragma once
#include "common.h"

namespace dram {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int KC = 4;  // input channels per LDS stage

// x / d by the multiply + shift that fast_div_prepare (conv_args.h) derives on the host
__device__ __forceinline__ unsigned fast_div(unsigned x, unsigned m, unsigned sh) {
    return (__umulhi(x, m) + x) >> sh;
}

// Buffer (SRD) loads: 32-bit per-lane byte offset against a wave-uniform descriptor.  Offsets at or
// beyond num_records return 0, so zero padding (volume border, channel tails) needs neither a
// branch nor a select -- and a branch around a load would make hipcc wait vmcnt(0) per element.
constexpr unsigned OOB = 0x80000000u;   // > any plane / filter size in bytes (checked on the host: check_conv_shape)

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ float buf_load(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, (int)soff, 0));
}
__device__ __forceinline__ f32x4 buf_load4(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
    const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 0);
    return __builtin_bit_cast(f32x4, v);
}
__device__ __forceinline__ const float* uniform_ptr(const float* p) {
    const unsigned long long v = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return (const float*)(((unsigned long long)hi << 32) | lo);
}

typedef __attribute__((address_space(3))) void* lds_ptr_t;    // destination of an LDS-DMA load

// Workgroups are dealt round-robin over the 8 XCDs (each with a private 4 MiB L2): hardware block b
// runs on XCD b % 8.  Map it to a logical work item so that every XCD walks a contiguous range of
// items: neighbouring boxes (shared halos) and the tiles that share a box then hit the same L2.
// Bijective for any n; placement is a speed matter only.
__device__ __forceinline__ int xcd_remap(int b, int n) {
    const int q = n / 8, r = n % 8;
    const int xcd = b % 8, idx = b / 8;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

}  // namespace dram
