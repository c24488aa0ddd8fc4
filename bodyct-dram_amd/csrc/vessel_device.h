// The per-voxel part of the Hessian vesselness (vessel.hip): eigenvalues of a symmetric 3x3 matrix, ordered by magnitude, and
// Frangi's tube measure.  Everything in fp64; the caller rounds the result once.  Compile with floating-point contraction off
// (vessel.hip does): tests/vessel_cases.py runs the same operations in numpy to measure the solver's own error.
#pragma once
#include <math.h>

namespace dram {

constexpr int VES_JACOBI_SWEEPS = 5;    // cyclic Jacobi on 3x3 reaches its fp64 floor after 4; one to spare

// One Jacobi rotation in the (p, q) plane: annihilates a_pq; r is the third index.  A zero a_pq leaves everything as it is.
// An a_pq so small that theta^2 overflows gives t = 0, i.e. a_pq is dropped, which is below half an ulp of either diagonal entry.
__device__ __forceinline__ void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.0;
    const double rp = arp, rq = arq;
    arp = c * rp - s * rq;
    arq = s * rp + c * rq;
}

// |a| < |b|, equal magnitudes by value: the order of a stable argsort of |eigvalsh(H)|
__device__ __forceinline__ bool magnitude_before(double a, double b) {
    const double fa = fabs(a), fb = fabs(b);
    return fa < fb || (fa == fb && a < b);
}

// h = {zz, yy, xx, zy, zx, yx}; l[0..2] = the eigenvalues by ascending magnitude
__device__ __forceinline__ void hessian_eigenvalues(const float* h, double* l) {
    double a00 = h[0], a11 = h[1], a22 = h[2], a01 = h[3], a02 = h[4], a12 = h[5];
#pragma unroll 1
    for (int sweep = 0; sweep < VES_JACOBI_SWEEPS; ++sweep) {
        jacobi_rotate(a00, a11, a01, a02, a12);
        jacobi_rotate(a00, a22, a02, a01, a12);
        jacobi_rotate(a11, a22, a12, a01, a02);
    }
    double t;
    if (magnitude_before(a11, a00)) { t = a00; a00 = a11; a11 = t; }
    if (magnitude_before(a22, a11)) { t = a11; a11 = a22; a22 = t; }
    if (magnitude_before(a11, a00)) { t = a00; a00 = a11; a11 = t; }
    l[0] = a00;
    l[1] = a11;
    l[2] = a22;
}

// Bright tube on dark.  two_a2 = 2 alpha^2, two_b2 = 2 beta^2, two_c2 = 2 c^2.  1 - exp(-x) is taken as -expm1(-x).
__device__ __forceinline__ double vesselness_value(const double* l, double two_a2, double two_b2, double two_c2) {
    if (l[1] >= 0.0 || l[2] >= 0.0) return 0.0;
    const double ra = fabs(l[1]) / fabs(l[2]);
    const double rb = fabs(l[0]) / sqrt(fabs(l[1] * l[2]));
    const double s2 = l[0] * l[0] + l[1] * l[1] + l[2] * l[2];
    const double v = -expm1(-(ra * ra) / two_a2) * exp(-(rb * rb) / two_b2) * -expm1(-s2 / two_c2);
    return isfinite(v) ? v : 0.0;
}

// sqrt(zz^2 + yy^2 + xx^2 + 2 (zy^2 + zx^2 + yx^2)) in fp64, rounded to fp32
__device__ __forceinline__ float hessian_frobenius(const float* h) {
    const double zz = h[0], yy = h[1], xx = h[2], zy = h[3], zx = h[4], yx = h[5];
    return (float)sqrt(zz * zz + yy * yy + xx * xx + 2.0 * (zy * zy + zx * zx + yx * yx));
}

}  // namespace dram
