// What the forward / backward-data 3x3x3 kernels of conv3d_k3.hip other than the (z,y) one -- direct, Winograd-z and the two
// first-layer kernels -- share: which (box, co tile) a block is, and the operand transform of a lazily normalised source.
#pragma once
#include "conv_args.h"
#include "conv_device.h"

namespace dram {

// logical item = (box, co tile), co tile fastest, then the box's x, y, z and the sample
struct FwdItem {
    int co0, bx, by, bz, n, x0, y0, z0;
};
template <int COB>
__device__ __forceinline__ FwdItem fwd_item(const ConvArgs& a, int BX, int BY, int BZ) {
    int b = xcd_remap(blockIdx.x, gridDim.x);
    const int co0 = (b % a.co_tiles) * COB; b /= a.co_tiles;
    const int bx = b % a.nbx; b /= a.nbx;
    const int by = b % a.nby; b /= a.nby;
    const int bz = b % a.nbz;
    return {co0, bx, by, bz, b / a.nbz, bx * BX, by * BY, bz * BZ};
}

// Operand transform of a lazily normalised source (ConvArgs::coef1/2): per K-chunk channel the wave-uniform
// {a, b, lo}: v -> max(a*v + b, lo), lo = 0 with ReLU and -inf without; identity {1, 0, -inf} for a plain source,
// {0, 0, 0} for the channel tail beyond Cin.
struct LazyCoef {
    float a, b, lo;
};
__device__ __forceinline__ LazyCoef lazy_coef(const ConvArgs& a, int n, int ci) {
    LazyCoef c;
    if (ci >= a.Cin) { c.a = 0.f; c.b = 0.f; c.lo = 0.f; return c; }
    const bool first = ci < a.src.C1;
    const float* cf = first ? a.coef1 : a.coef2;
    const int relu = first ? a.relu1 : a.relu2;
    if (cf == nullptr) { c.a = 1.f; c.b = 0.f; c.lo = -INFINITY; return c; }
    const int64_t row = first ? (int64_t)n * a.src.C1 + ci : (int64_t)n * a.src.C2 + (ci - a.src.C1);
    c.a = cf[2 * row];
    c.b = cf[2 * row + 1];
    c.lo = relu ? 0.f : -INFINITY;
    return c;
}

}  // namespace dram
