// Device arithmetic that the volume paths share (infer.hip, prep.hip, crop.hip, augment.hip): the resampling grid of
// sitk.ResampleImageFilter, its fp64 lerp, the fp64 window of a scan with its 8-bit bin, and order-preserving unsigned keys.
// One definition each: a correction to any of them is made here and reaches every kernel.
#pragma once
#include "common.h"

namespace dram {

// ---------------------------------------------------------------- the ITK resampling grid
// The reference resamples through utils.resample (utils.py:299-381, 414-434): sitk.ResampleImageFilter.Execute with the identity
// transform, the image's own origin and direction, default value 0, output pixel type = input pixel type.  SimpleITK is not
// available here (PARITY UNPINNED); this restates the grid from ITK's published semantics of that call.  Per axis, output voxel
// o sits at physical position origin + o * spacing_out, i.e. at the continuous input index
//     c = o * spacing_out / spacing_in        (Resample('fixed_size'): spacing_out = spacing_in * size_in / size_out)
// and c >= 0 always (same origin).  Forming c is the caller's: its rounding is part of the result, and the callers differ.
//   inside   c < size - 0.5 (ImageFunction::IsInsideBuffer: [-0.5, size - 0.5)); otherwise the output is the default value
//   linear   between floor(c) and floor(c) + 1, the upper neighbour clamped to the last voxel, t = 0 where the two coincide
//            (LinearInterpolateImageFunction::EvaluateOptimized); lerps along x, then y, then z in double (RealType of short /
//            float pixels), then ResampleImageFilter::CastPixelWithBoundsChecking
//   nearest  voxel floor(c + 0.5) (NearestNeighborInterpolateImageFunction: Math::RoundHalfIntegerUp)
struct ItkAxis {
    bool inside;
    int lo, hi;         // the linear pair (when !inside: both the last voxel)
    double t;           // weight of hi
    int nearest;        // (when !inside: the last voxel)
};

__device__ __forceinline__ double mul_rn(double a, double b) {       // (HIP's __dmul_rn is a plain `*`, open to contraction)
#pragma clang fp contract(off)
    return a * b;
}

// (no contraction, here and in mul_rn: hipcc would otherwise turn c - lo into fma(o, step, -lo) and c + 0.5 into fma(o, step, 0.5),
//  which is not what ITK or the oracle compute)
__device__ __forceinline__ ItkAxis itk_axis(double c, int size) {
#pragma clang fp contract(off)
    ItkAxis a;
    a.inside = c < (double)size - 0.5;                 // false for NaN and for every c that would overflow an int:
    const int b = a.inside ? (int)c : size - 1;        // (int) is only taken of a c that is inside
    a.lo = b > size - 1 ? size - 1 : b;
    a.hi = a.lo + 1 <= size - 1 ? a.lo + 1 : a.lo;
    a.t = a.hi == a.lo ? 0.0 : c - (double)a.lo;
    // inside means c + 0.5 < size, so the nearest voxel needs no clamp -- but for one value: size == 1 and c = 0.5 - 2^-54, the
    // double below 0.5, whose sum with 0.5 rounds to 1.0.  The clamp is there for that value alone.
    const int n = a.inside ? (int)(c + 0.5) : size - 1;
    a.nearest = n > size - 1 ? size - 1 : n;
    return a;
}

// u + (v - u) * t in fp64 with the product rounded on its own.  No fused multiply-add: ITK's x86 builds round the product, and
// so does the oracle.  It shows where an int16 result truncates: -484 + 705 * 0.4 is -202 with a rounded product and
// -201.99999999999997 fused.
__device__ __forceinline__ double lerp_rn(double u, double v, double t) {
#pragma clang fp contract(off)
    const double p = (v - u) * t;
    return u + p;
}

// ---------------------------------------------------------------- the fp64 window of a scan and its 8-bit bin
// w_scan = windowing(scan, from_span=(wmin, wmax), to_span=(0, 1)) (utils.py:189-198): numpy clips the int16 scan, subtracts in
// integers and divides by float(wmax - wmin), in fp64.  binary_cam's 8-bit view of it (utils.py:233): windowing(., (0, 1)) ->
// (w / 1.0) * 255 + 0 -> astype(uint8) truncates.  The same fp64 operations in the same order, so that bin and comparison are
// bit-identical to numpy's.
__device__ __forceinline__ double windowed_scan(int s, int wmin, int wmax) {
#pragma clang fp contract(off)
    const int c = s < wmin ? wmin : (s > wmax ? wmax : s);
    return (double)(c - wmin) / (double)(wmax - wmin);
}
__device__ __forceinline__ int scan_bin(double w) {
#pragma clang fp contract(off)
    return (int)((w / 1.0) * 255.0 + 0.0);
}

// ---------------------------------------------------------------- order keys
// Elements mapped to unsigned keys of the same order, so that one integer min / max serves fp32 and uint8: integer atomics are
// exact, associative and commutative (also in LDS), so a result does not depend on which lane or block arrives first.
template <typename T> struct Key;
template <> struct Key<float> {
    static __device__ __forceinline__ unsigned enc(float f) {
        const unsigned u = __float_as_uint(f);
        return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
    static __device__ __forceinline__ float dec(unsigned e) {
        return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e);
    }
};
template <> struct Key<unsigned char> {
    static __device__ __forceinline__ unsigned enc(unsigned char v) { return v; }
    static __device__ __forceinline__ unsigned char dec(unsigned e) { return (unsigned char)e; }
};
constexpr unsigned KEY_TOP = 0xffffffffu;
__device__ __forceinline__ unsigned umin_(unsigned a, unsigned b) { return a < b ? a : b; }

}  // namespace dram
