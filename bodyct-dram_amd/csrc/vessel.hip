// Pseudo-vessel mask (gfx950): Frangi's multi-scale Hessian vesselness.  The definition -- taps, boundary, order of the
// operations -- is in include/dram_hip.h (dram_hessian ...); this file is the kernels.
//
// One scale: the scale-normalised Hessian of Gaussian by three separable passes x, y, z, every intermediate materialised
//   hess_x_kernel     scan (int16 / fp32, clamped on load) -> g0, g1, g2: orders 0, 1, 2 along x              2|4 B in, 12 B out
//   hess_axis_kernel  along y: g0 -> orders 0, 1, 2;  g1 -> orders 0, 1;  g2 -> order 0                       12 B in, 24 B out
//   hess_axis_kernel  along z: one order per output, times sv[a] * sv[b]                                      24 B in, 24 B out
// then hessian_norm_max (c = None), vesselness (eigenvalues, tube measure, running maximum over scales) and vessel_mask.
//
// Every output of a filter pass is one chain, the same for every voxel whatever tile it falls in:
//   acc = w[0] * v[i];   for j = 1 .. 4 * ceil(r / 4):   acc = fmaf(w[j], v[i - j] (+|-) v[i + j], acc)
// with the sum for the even orders and the difference v[i + j] - v[i - j] for order 1 (whose acc starts at 0): the symmetry of
// the taps halves the multiplications.  Taps past the radius are zero in the table; the staged halo is reflected at every
// distance, so they multiply finite values.  A thread owns 4 consecutive outputs along the filtered axis and walks the taps four
// at a time over two sliding 8-value windows held in registers (filter_taps4), so a value read from LDS serves up to 4 outputs
// x 3 orders.  The x pass reads its windows as 16-byte LDS accesses and stores 16 bytes per lane; the axis passes keep x across
// the lanes (one dword per lane, 256 B per wave and row).
#include <math.h>
#include "common.h"
#include "vessel_device.h"

#pragma clang fp contract(off)

namespace dram {

constexpr int VES_RMAX = 32;                 // largest radius: s = 4 mm at 0.5 mm spacing; a multiple of 4
constexpr int VES_TS = VES_RMAX + 1;         // taps per (axis, order) in the table
constexpr int VX_T = 256;                    // x pass: outputs along x per wave (4 per lane)
constexpr int VX_ROWS = 4;                   //         rows per block, one per wave
constexpr int VA_TX = 64;                    // axis pass: columns per block (one wave wide)
constexpr int VA_TY = 4;                     //            waves per block
constexpr int VA_LT = 64;                    //            outputs along the axis per block: 4 groups of 4 per wave

// scipy's 'reflect' (d c b a | a b c d), folded as often as needed
__device__ __forceinline__ int reflect_index(int i, int n) {
    const int period = 2 * n;
    int m = i % period;
    if (m < 0) m += period;
    return m >= n ? period - 1 - m : m;
}

__device__ __forceinline__ float load_clamped(const int16_t* p, long long i, float lo, float hi) {
    float v = (float)p[i];
    v = v < lo ? lo : v;
    return v > hi ? hi : v;
}
__device__ __forceinline__ float load_clamped(const float* p, long long i, float lo, float hi) {
    float v = p[i];
    v = v < lo ? lo : v;           // a NaN stays a NaN
    return v > hi ? hi : v;
}

// Taps j0 + 1 .. j0 + 4 for the outputs i0 .. i0 + 3.  lo[4 + k - j] = v[i0 + k - j0 - j], hi[k + j] = v[i0 + k + j0 + j].
// w0, w1, w2 point at tap j0 of the three orders.  MASK: bit o set = order o is wanted.
template <int MASK>
__device__ __forceinline__ void filter_taps4(const float* lo, const float* hi, const float* __restrict__ w0, const float* __restrict__ w1,
                                             const float* __restrict__ w2, float* a0, float* a1, float* a2) {
#pragma unroll
    for (int j = 1; j <= 4; ++j) {
        const float t0 = (MASK & 1) ? w0[j] : 0.f, t1 = (MASK & 2) ? w1[j] : 0.f, t2 = (MASK & 4) ? w2[j] : 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float l = lo[4 + k - j], h = hi[k + j];
            if (MASK & 5) {
                const float s = l + h;
                if (MASK & 1) a0[k] = fmaf(t0, s, a0[k]);
                if (MASK & 4) a2[k] = fmaf(t2, s, a2[k]);
            }
            if (MASK & 2) a1[k] = fmaf(t1, h - l, a1[k]);
        }
    }
}

// Chunk(c, v): v[0..3] = the four values at offset 4c .. 4c + 3 from the thread's first output.
template <int MASK, typename Chunk>
__device__ __forceinline__ void filter4(Chunk chunk, const float* __restrict__ taps, int r, float* a0, float* a1, float* a2) {
    const float* w0 = taps;
    const float* w1 = taps + VES_TS;
    const float* w2 = taps + 2 * VES_TS;
    float lo[8], hi[8];
    chunk(-1, lo);
    chunk(0, lo + 4);
    chunk(1, hi + 4);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        hi[k] = lo[4 + k];
        a0[k] = w0[0] * lo[4 + k];
        a1[k] = 0.f;
        a2[k] = w2[0] * lo[4 + k];
    }
    for (int j0 = 0; j0 < r; j0 += 4) {
        filter_taps4<MASK>(lo, hi, w0 + j0, w1 + j0, w2 + j0, a0, a1, a2);
        if (j0 + 4 < r) {                                     // uniform: r is a launch argument
            const int b = j0 >> 2;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                lo[4 + k] = lo[k];
                hi[k] = hi[4 + k];
            }
            chunk(-b - 2, lo);
            chunk(b + 2, hi + 4);
        }
    }
}

// rows x W.  Block: VX_ROWS rows (one per wave) x VX_T outputs.  The row piece with its halo of hb = max(4, 4 * ceil(r / 4)) values is
// converted, clamped and staged in LDS; stage[w][hb + i] = v[x0 + i].  taps: the x axis' three orders.
template <typename T>
__global__ __launch_bounds__(256) void hess_x_kernel(const T* __restrict__ scan, float clip_lo, float clip_hi, const float* __restrict__ taps,
                                                      int r, float* __restrict__ g0, float* __restrict__ g1, float* __restrict__ g2,
                                                      long long rows, int W, int xtiles, int vec) {
    __shared__ __attribute__((aligned(16))) float stage[VX_ROWS][VX_T + 2 * VES_RMAX];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long row = (long long)(blockIdx.x / xtiles) * VX_ROWS + wv;
    const int x0 = (int)(blockIdx.x % xtiles) * VX_T;
    const int hb = r > 4 ? ((r + 3) >> 2) << 2 : 4;
    if (row < rows) {                                         // wave-uniform
        for (int p = lane; p < VX_T + 2 * hb; p += 64)
            stage[wv][p] = load_clamped(scan, row * W + reflect_index(x0 - hb + p, W), clip_lo, clip_hi);
    }
    __syncthreads();
    const int x = x0 + 4 * lane;
    if (row >= rows || x >= W) return;
    const float* mine = &stage[wv][hb + 4 * lane];            // 16-byte aligned: hb and the row length are multiples of 4
    float a0[4], a1[4], a2[4];
    filter4<7>([&](int c, float* v) {
        const float4 q = *reinterpret_cast<const float4*>(mine + 4 * c);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    }, taps, r, a0, a1, a2);
    const long long at = row * W + x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {                             // a zero leaves every pass as +0, whatever the zero taps past r met
        a0[k] += 0.f;
        a1[k] += 0.f;
        a2[k] += 0.f;
    }
    if (vec) {                                                // W % 4 == 0 and 16-byte aligned bases: x + 3 < W
        *reinterpret_cast<float4*>(g0 + at) = make_float4(a0[0], a0[1], a0[2], a0[3]);
        *reinterpret_cast<float4*>(g1 + at) = make_float4(a1[0], a1[1], a1[2], a1[3]);
        *reinterpret_cast<float4*>(g2 + at) = make_float4(a2[0], a2[1], a2[2], a2[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x + k < W) {
                g0[at + k] = a0[k];
                g1[at + k] = a1[k];
                g2[at + k] = a2[k];
            }
    }
}

// src, d0, d1, d2: [outer][L][inner], filtered along L.  Block: VA_LT outputs along L x VA_TX columns; blockIdx.x = (o * ltiles +
// lt) * ctiles + ct.  stage[hb + i][tx] = src[l0 + i].  Wave ty owns the groups ty, ty + VA_TY, ... of 4 consecutive outputs.
// d_o = order o of the axis (taps) times scale_o; only the orders of MASK are computed and written.
template <int MASK>
__global__ __launch_bounds__(VA_TX* VA_TY) void hess_axis_kernel(const float* __restrict__ src, float* __restrict__ d0, float* __restrict__ d1,
                                                                  float* __restrict__ d2, const float* __restrict__ taps, int r, float scale0,
                                                                  float scale1, float scale2, int L, long long inner, int ctiles, int ltiles) {
    __shared__ float stage[VA_LT + 2 * VES_RMAX][VA_TX];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const long long col = (long long)(blockIdx.x % ctiles) * VA_TX + tx;
    const long long rest = blockIdx.x / ctiles;
    const int l0 = (int)(rest % ltiles) * VA_LT;
    const long long base = (rest / ltiles) * L * inner + col;
    const int hb = r > 4 ? ((r + 3) >> 2) << 2 : 4;
    const bool live = col < inner;
    for (int p = ty; p < VA_LT + 2 * hb; p += VA_TY)
        stage[p][tx] = live ? src[base + (long long)reflect_index(l0 - hb + p, L) * inner] : 0.f;
    __syncthreads();
    if (!live) return;
    for (int g = ty; g < VA_LT / 4; g += VA_TY) {
        const int l = l0 + 4 * g;
        if (l >= L) break;                                    // wave-uniform
        const int at = hb + 4 * g;
        float a0[4], a1[4], a2[4];
        filter4<MASK>([&](int c, float* v) {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = stage[at + 4 * c + k][tx];
        }, taps, r, a0, a1, a2);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (l + k < L) {
                const long long o = base + (long long)(l + k) * inner;
                if (MASK & 1) d0[o] = a0[k] * scale0 + 0.f;       // (-0 -> +0, as in the x pass)
                if (MASK & 2) d1[o] = a1[k] * scale1 + 0.f;
                if (MASK & 4) d2[o] = a2[k] * scale2 + 0.f;
            }
    }
}

// Non-negative floats order like their bit patterns: an integer max-atomic is exact and does not depend on the order.
__global__ __launch_bounds__(256) void hessian_norm_max_kernel(const float* __restrict__ h6, const uint8_t* __restrict__ lobe, long long S,
                                                               unsigned int* out) {
    unsigned int m = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < S; i += (long long)gridDim.x * 256) {
        if (lobe && !lobe[i]) continue;
        float h[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) h[k] = h6[k * S + i];
        m = max(m, __float_as_uint(hessian_frobenius(h)));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned int)__shfl_xor((int)m, o, 64));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

// c = half the maximum; 1 for a zero maximum
__global__ void hessian_norm_finish_kernel(float* c) {
    const float m = *c;
    *c = m == 0.f ? 1.f : 0.5f * m;
}

__global__ __launch_bounds__(256) void vesselness_kernel(const float* __restrict__ h6, long long S, double two_a2, double two_b2,
                                                         const float* __restrict__ c_dev, float* __restrict__ vmax, int accumulate,
                                                         double* __restrict__ eig) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= S) return;
    const double c = (double)*c_dev;
    float h[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) h[k] = h6[k * S + i];
    double l[3];
    hessian_eigenvalues(h, l);
    const float v = (float)vesselness_value(l, two_a2, two_b2, 2.0 * c * c);
    vmax[i] = accumulate ? fmaxf(vmax[i], v) : v;
    if (eig) {
        eig[i] = l[0];
        eig[S + i] = l[1];
        eig[2 * S + i] = l[2];
    }
}

__global__ __launch_bounds__(256) void vessel_mask_kernel(const float* __restrict__ vmax, const uint8_t* __restrict__ lobe, float th,
                                                          uint8_t* __restrict__ mask, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) mask[i] = vmax[i] >= th && (!lobe || lobe[i] != 0);
}

// (2 * n of reflect_index stays an int)
static inline bool vessel_sizes_ok(int D, int H, int W) {
    return D > 0 && H > 0 && W > 0 && D < (1 << 30) && H < (1 << 30) && W < (1 << 30) && (long long)D * H * W < (1LL << 31);
}

template <int MASK>
static void hess_axis_launch(const float* src, float* d0, float* d1, float* d2, const float* taps, int r, float s0, float s1, float s2,
                             long long outer, int L, long long inner, hipStream_t st) {
    const long long ctiles = cdiv64(inner, VA_TX), ltiles = cdiv(L, VA_LT);   // outer * ltiles * ctiles <= D * H * W < 2^31
    hipLaunchKernelGGL((hess_axis_kernel<MASK>), dim3((unsigned)(outer * ltiles * ctiles)), dim3(VA_TX, VA_TY), 0, st, src, d0, d1, d2,
                       taps, r, s0, s1, s2, L, inner, (int)ctiles, (int)ltiles);
}

}  // namespace dram

using namespace dram;

extern "C" int dram_vessel_max_radius(void) { return VES_RMAX; }

extern "C" size_t dram_hessian_ws_bytes(int D, int H, int W) {
    if (!vessel_sizes_ok(D, H, W)) {
        set_error("hessian_ws_bytes: sizes must be positive with D*H*W < 2^31");
        return 0;
    }
    return (size_t)9 * D * H * W * sizeof(float);             // g0, g1, g2 of the x pass and the six outputs of the y pass
}

extern "C" int dram_hessian(const void* scan, int dtype, float clip_lo, float clip_hi, const float* taps, const int* radius,
                            const double* sv, int D, int H, int W, float* h6, void* ws, size_t ws_bytes, void* stream) {
    DRAM_REQUIRE(scan && taps && radius && sv && h6 && ws, "hessian: null pointer");
    DRAM_REQUIRE(dtype == DRAM_VESSEL_INT16 || dtype == DRAM_VESSEL_FLOAT32, "hessian: dtype must be DRAM_VESSEL_INT16 or DRAM_VESSEL_FLOAT32");
    DRAM_REQUIRE(vessel_sizes_ok(D, H, W), "hessian: sizes must be positive with D*H*W < 2^31");
    DRAM_REQUIRE(clip_lo <= clip_hi, "hessian: clip_lo must not exceed clip_hi");
    for (int a = 0; a < 3; ++a) {
        DRAM_REQUIRE(radius[a] >= 0 && radius[a] <= VES_RMAX, "hessian: radius %d of axis %d is outside 0 .. %d", radius[a], a, VES_RMAX);
        DRAM_REQUIRE(sv[a] > 0.0 && sv[a] <= 1e6, "hessian: sigma in voxels must be positive and at most 1e6");
    }
    DRAM_REQUIRE(((uintptr_t)ws & 3) == 0 && ((uintptr_t)h6 & 3) == 0 && ((uintptr_t)taps & 3) == 0,
                 "hessian: workspace, h6 and taps must be 4-byte aligned");
    if (ws_bytes < dram_hessian_ws_bytes(D, H, W)) {
        set_error("hessian: workspace too small");
        return DRAM_EWS;
    }
    const long long S = (long long)D * H * W, rows = (long long)D * H, plane = (long long)H * W;
    float* g = (float*)ws;                                    // g[o]: order o along x
    float* t = g + 3 * S;                                     // t[k]: the y pass' outputs, in h6's order
    const float *tz = taps, *ty = taps + 3 * VES_TS, *tx = taps + 6 * VES_TS;
    hipStream_t st = (hipStream_t)stream;
    const int xtiles = cdiv(W, VX_T);
    const int vec = W % 4 == 0 && aligned16(g);               // S * 4 bytes is then a multiple of 16 as well
    const unsigned xblocks = (unsigned)(cdiv64(rows, VX_ROWS) * xtiles);
    if (dtype == DRAM_VESSEL_INT16)
        hipLaunchKernelGGL(hess_x_kernel<int16_t>, dim3(xblocks), dim3(256), 0, st, (const int16_t*)scan, clip_lo, clip_hi, tx, radius[2],
                           g, g + S, g + 2 * S, rows, W, xtiles, vec);
    else
        hipLaunchKernelGGL(hess_x_kernel<float>, dim3(xblocks), dim3(256), 0, st, (const float*)scan, clip_lo, clip_hi, tx, radius[2], g,
                           g + S, g + 2 * S, rows, W, xtiles, vec);
    // y: (x order, y order) -> zz (0,0), yy (0,2), xx (2,0), zy (0,1), zx (1,0), yx (1,1)
    hess_axis_launch<7>(g, t, t + 3 * S, t + S, ty, radius[1], 1.f, 1.f, 1.f, D, H, W, st);
    hess_axis_launch<3>(g + S, t + 4 * S, t + 5 * S, nullptr, ty, radius[1], 1.f, 1.f, 1.f, D, H, W, st);
    hess_axis_launch<1>(g + 2 * S, t + 2 * S, nullptr, nullptr, ty, radius[1], 1.f, 1.f, 1.f, D, H, W, st);
    // z: zz order 2, zy and zx order 1, the others order 0; times sv[a] * sv[b]
    const float szz = (float)(sv[0] * sv[0]), syy = (float)(sv[1] * sv[1]), sxx = (float)(sv[2] * sv[2]);
    const float szy = (float)(sv[0] * sv[1]), szx = (float)(sv[0] * sv[2]), syx = (float)(sv[1] * sv[2]);
    hess_axis_launch<4>(t, nullptr, nullptr, h6, tz, radius[0], 0.f, 0.f, szz, 1, D, plane, st);
    hess_axis_launch<1>(t + S, h6 + S, nullptr, nullptr, tz, radius[0], syy, 0.f, 0.f, 1, D, plane, st);
    hess_axis_launch<1>(t + 2 * S, h6 + 2 * S, nullptr, nullptr, tz, radius[0], sxx, 0.f, 0.f, 1, D, plane, st);
    hess_axis_launch<2>(t + 3 * S, nullptr, h6 + 3 * S, nullptr, tz, radius[0], 0.f, szy, 0.f, 1, D, plane, st);
    hess_axis_launch<2>(t + 4 * S, nullptr, h6 + 4 * S, nullptr, tz, radius[0], 0.f, szx, 0.f, 1, D, plane, st);
    hess_axis_launch<1>(t + 5 * S, h6 + 5 * S, nullptr, nullptr, tz, radius[0], syx, 0.f, 0.f, 1, D, plane, st);
    return check_launch("hessian");
}

extern "C" int dram_hessian_norm_max(const float* h6, const uint8_t* lobe, int64_t S, float* c_out, void* stream) {
    DRAM_REQUIRE(h6 && c_out, "hessian_norm_max: null pointer");
    DRAM_REQUIRE(S > 0 && S < (1LL << 31), "hessian_norm_max: S must be in 1 .. 2^31 - 1");
    DRAM_REQUIRE(((uintptr_t)c_out & 3) == 0 && ((uintptr_t)h6 & 3) == 0, "hessian_norm_max: h6 and c_out must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    (void)hipMemsetAsync(c_out, 0, sizeof(float), st);
    const long long blocks = cdiv64(S, 256);
    hipLaunchKernelGGL(hessian_norm_max_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, h6, lobe, (long long)S,
                       (unsigned int*)c_out);
    hipLaunchKernelGGL(hessian_norm_finish_kernel, dim3(1), dim3(1), 0, st, c_out);
    return check_launch("hessian_norm_max");
}

extern "C" int dram_vesselness(const float* h6, int64_t S, double alpha, double beta, const float* c_dev, float* vmax, int accumulate,
                               double* eig, void* stream) {
    DRAM_REQUIRE(h6 && c_dev && vmax, "vesselness: null pointer");
    DRAM_REQUIRE(S > 0 && S < (1LL << 31), "vesselness: S must be in 1 .. 2^31 - 1");
    DRAM_REQUIRE(alpha > 0.0 && beta > 0.0 && alpha <= 1e6 && beta <= 1e6, "vesselness: alpha and beta must be positive and at most 1e6");
    DRAM_REQUIRE(((uintptr_t)eig & 7) == 0 && ((uintptr_t)h6 & 3) == 0 && ((uintptr_t)vmax & 3) == 0 && ((uintptr_t)c_dev & 3) == 0,
                 "vesselness: eig must be 8-byte, h6, vmax and c 4-byte aligned");
    hipLaunchKernelGGL(vesselness_kernel, dim3((unsigned)cdiv64(S, 256)), dim3(256), 0, (hipStream_t)stream, h6, (long long)S,
                       2.0 * alpha * alpha, 2.0 * beta * beta, c_dev, vmax, accumulate, eig);
    return check_launch("vesselness");
}

extern "C" int dram_vessel_mask(const float* vmax, const uint8_t* lobe, float threshold, uint8_t* mask, int64_t n, void* stream) {
    DRAM_REQUIRE(vmax && mask, "vessel_mask: null pointer");
    DRAM_REQUIRE(n > 0 && n < (1LL << 31), "vessel_mask: n must be in 1 .. 2^31 - 1");
    hipLaunchKernelGGL(vessel_mask_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, (hipStream_t)stream, vmax, lobe, threshold, mask,
                       (long long)n);
    return check_launch("vessel_mask");
}
