// Block scaffold of the 3x3x3 backward-weights kernels of conv3d_k3.hip: which (split, co tile, ci tile) item a block is and which
// sub-tile a wave owns, where a box lies, and the two direct kernels' 27-tap MFMA loop and epilogue.
#pragma once
#include "conv_args.h"
#include "conv_device.h"

namespace dram {

// logical item = (split, co tile, ci tile), ci tile fastest; wave (wco, wci) owns one 16x16 (co, ci) sub-tile of the
// (16*COS) x CI_B block tile, lane = (i, k) of the MFMA operand layout
struct WgradItem {
    int sp, ci0, co0, wco, wci, i, k;
};
template <int CO_B, int CI_B, int COS>
__device__ __forceinline__ WgradItem wgrad_item(const WgradArgs& a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int b = xcd_remap(blockIdx.x, gridDim.x);
    const int ci_t = b % a.ci_tiles; b /= a.ci_tiles;
    const int co_t = b % a.co_tiles;
    return {b / a.co_tiles, ci_t * CI_B, co_t * CO_B, wave % COS, wave / COS, lane & 15, lane >> 4};
}

// box index -> sample and origin (x fastest, then y, z, n)
struct WgradBox {
    int n, x0, y0, z0;
};
__device__ __forceinline__ WgradBox wgrad_box(const WgradArgs& a, int box, int BX, int BY, int BZ) {
    const int bx = box % a.nbx; box /= a.nbx;
    const int by = box % a.nby; box /= a.nby;
    const int bz = box % a.nbz;
    return {box / a.nbz, bx * BX, by * BY, bz * BZ};
}

// The direct kernels' MFMA loop over one BX x BY x BZ box: VOX/4 k-steps (4 voxels along x each) x 27 taps of 16x16x4 MFMAs.
// ap: this lane's dY row [BZ][BY][BX]; bp: its X halo row at halo x = 0 of the first row, rows ROW floats apart, HY rows a plane.
template <int BX, int BY, int BZ, int ROW, int HY>
__device__ __forceinline__ void wgrad_direct_mfma(const float* ap, const float* bp, f32x4 (&acc)[27]) {
    constexpr int NS = BX * BY * BZ / 4;
    float av[2], bv[2][27];
    // two operand sets live; one operand read of k-step s beside each MFMA of k-step s-1: the 28 LDS reads of a step are spread
    // over its 27 MFMA slots instead of being issued as one burst that the 4-bit lgkmcnt counter throttles
#pragma unroll
    for (int s = 0; s <= NS; ++s) {
        const int x4 = s % (BX / 4), vy = (s / (BX / 4)) % BY, vz = s / ((BX / 4) * BY);
        const float* bq = bp + (vz * HY + vy) * ROW + 4 * x4;
        if (s < NS) av[s & 1] = ap[(vz * BY + vy) * BX + 4 * x4];
#pragma unroll
        for (int tap = 0; tap < 27; ++tap) {
            const int dz = tap / 9, dy = (tap / 3) % 3, dx = tap % 3;
            if (s < NS) bv[s & 1][tap] = bq[(dz * HY + dy) * ROW + dx];
            if (s > 0) acc[tap] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[(s - 1) & 1], bv[(s - 1) & 1][tap], acc[tap], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// The direct kernels' partial slab [sp][co][ci][27]: accumulator row = co (4*k + r), column = ci (i)
__device__ __forceinline__ void wgrad_store_slab27(const WgradArgs& a, const WgradItem& it, const f32x4 (&acc)[27]) {
    const int ci = it.ci0 + it.wci * 16 + it.i;
    if (ci < a.Cin) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int co = it.co0 + it.wco * 16 + 4 * it.k + r;
            if (co < a.Cout) {
                float* o = a.slabs + (((size_t)it.sp * a.Cout + co) * a.Cin + ci) * 27;
#pragma unroll
                for (int tap = 0; tap < 27; ++tap) o[tap] = acc[tap][r];
            }
        }
    }
}

}  // namespace dram
