// Heat-map refinement (gfx950): the masked 3-D guided filter.  The definition -- window, selection by the region, order of the
// operations of steps 2 and 3 -- is in include/dram_hip.h ("heat-map refinement"); this file is the kernels.
//
// Two stages of three separable box-sum passes x, y, z over fp64 fields [F][D][H][W]; every pass carries all fields of its
// stage in one launch, and the point-wise steps ride on the last pass of each stage:
//   stage 1  guided_x_kernel<int16|float>  G, P, M -> N, Sg, Sp, Sgg, Sgp summed along x       9 (7) B in, 40 B out
//            guided_axis_kernel<5, NONE>   along y                                              40 B in, 40 B out
//            guided_axis_kernel<5, COEF>   along z, then step 2: a, b (0 outside M) and N       40 + 1 B in, 24 B out
//   stage 2  guided_x_kernel<ab>           a, b summed along x                                  16 B in, 16 B out
//            guided_axis_kernel<2, NONE>   along y                                              16 B in, 16 B out
//            guided_axis_kernel<2, APPLY>  along z, then step 3: q = (float)(A g + B)           16 + 8 + 1 + 2|4 B in, 4 B out
//
// Every box sum is a DIRECT window sum: acc = 0; for j = -r .. r: acc += v[i + j], ascending, with 0 for a position outside
// the volume.  No running sum, no tree: the value at a voxel depends on nothing but the 2r + 1 values around it, so it is the
// same whatever tile the voxel falls in and whatever lies beyond the bounding box of M (there every field is +0, and adding +0
// changes no bit) -- which is what lets the host filter the lobe box alone and get the whole-volume bits.  A voxel outside M
// enters stage 1 as a selected +0 in every field, never as a product.
//
// Layout.  A thread owns 4 consecutive outputs along the summed axis and walks the 2r + 4 staged values once, ascending; each
// value read from LDS is added to the (up to 4) outputs whose window holds it.  x pass: a wave owns a row piece of 256 outputs
// (4 per lane: 16-byte global loads of P, 16-byte stores of every field); the piece and its halo are staged as fp64 with one
// pad entry per 32, which spreads the lanes' stride of 4 doubles over all banks.  Axis passes: a block of 8 waves owns 32
// outputs along the axis x 128 columns, a lane two adjacent columns (16-byte global and LDS accesses, lanes contiguous: no
// bank conflicts); the fields go through the one 64 KiB stage one after the other.
#include <math.h>
#include "common.h"

#pragma clang fp contract(off)

namespace dram {

constexpr int GF_RMAX = 16;                  // largest radius: 8 mm at 0.5 mm spacing; a multiple of 4
constexpr int GX_T = 256;                    // x pass: outputs along x per wave (4 per lane)
constexpr int GX_ROWS = 4;                   //         rows per block, one per wave
constexpr int GX_SW = GX_T + 2 * GF_RMAX;    //         staged values per row, before padding
constexpr int GA_TX = 128;                   // axis pass: columns per block (2 per lane)
constexpr int GA_LT = 32;                    //            outputs along the axis per block: 4 per wave
constexpr int GA_WAVES = GA_LT / 4;

enum { GF_EPI_NONE = 0, GF_EPI_COEF = 1, GF_EPI_APPLY = 2 };
enum { GF_SRC_INT16 = 0, GF_SRC_FLOAT = 1, GF_SRC_AB = 2 };

__device__ __forceinline__ int gx_pos(int e) { return e + (e >> 5); }

__device__ __forceinline__ double guide_value(const void* guide, int kind, long long i, double lo, double hi) {
    if (kind == GF_SRC_FLOAT) return (double)((const float*)guide)[i];
    const double g = ((double)((const int16_t*)guide)[i] - lo) / (hi - lo);
    return g < 0.0 ? 0.0 : (g > 1.0 ? 1.0 : g);
}

// rows x W.  Block: GX_ROWS rows (one per wave) x GX_T outputs.  stage[s][w][gx_pos(hb + i)] = source s at x0 + i, hb = r rounded
// up to a multiple of 4; 0 outside the row and, for the raw sources, outside M.
//   SRC int16 / float: s = g, p, [M != 0];  dst[5][S] = N, Sg, Sp, Sgg, Sgp.       SRC ab: s = a, b (src0[2][S]);  dst[2][S].
template <int SRC>
__global__ __launch_bounds__(256) void guided_x_kernel(const void* __restrict__ src0, const float* __restrict__ p, const uint8_t* __restrict__ mask,
                                                        double lo, double hi, int r, double* __restrict__ dst, long long rows, int W,
                                                        long long S, int xtiles, int vec) {
    constexpr int NS = SRC == GF_SRC_AB ? 2 : 3, NF = SRC == GF_SRC_AB ? 2 : 5;
    __shared__ __attribute__((aligned(16))) double stage[NS][GX_ROWS][GX_SW + GX_SW / 32 + 1];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long row = (long long)(blockIdx.x / xtiles) * GX_ROWS + wv;
    const int x0 = (int)(blockIdx.x % xtiles) * GX_T;
    const int hb = (r + 3) & ~3;
    if (row < rows) {                                         // wave-uniform
        const long long rbase = row * W;
        for (int c = lane; c < (GX_T + 2 * hb) / 4; c += 64) {
            const int e0 = 4 * c, x = x0 - hb + e0;
            double v[NS][4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int s = 0; s < NS; ++s) v[s][k] = 0.0;
            if (x >= 0 && x < W) {
                const long long at = rbase + x;
                if constexpr (SRC == GF_SRC_AB) {
                    const double* ab = (const double*)src0;
                    if (vec) {                                // W % 4 == 0: x + 3 < W
                        const double2 a0 = *reinterpret_cast<const double2*>(ab + at), a1 = *reinterpret_cast<const double2*>(ab + at + 2);
                        const double2 b0 = *reinterpret_cast<const double2*>(ab + S + at), b1 = *reinterpret_cast<const double2*>(ab + S + at + 2);
                        v[0][0] = a0.x; v[0][1] = a0.y; v[0][2] = a1.x; v[0][3] = a1.y;
                        v[1][0] = b0.x; v[1][1] = b0.y; v[1][2] = b1.x; v[1][3] = b1.y;
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (x + k < W) {
                                v[0][k] = ab[at + k];
                                v[1][k] = ab[S + at + k];
                            }
                    }
                } else {
                    float pv[4] = {0.f, 0.f, 0.f, 0.f};
                    unsigned char mv[4] = {0, 0, 0, 0};
                    if (vec) {
                        const float4 q = *reinterpret_cast<const float4*>(p + at);
                        const uchar4 m = *reinterpret_cast<const uchar4*>(mask + at);
                        pv[0] = q.x; pv[1] = q.y; pv[2] = q.z; pv[3] = q.w;
                        mv[0] = m.x; mv[1] = m.y; mv[2] = m.z; mv[3] = m.w;
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (x + k < W) {
                                pv[k] = p[at + k];
                                mv[k] = mask[at + k];
                            }
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const bool in = mv[k] != 0;           // (mv stays 0 past the end of the row)
                        const double g = in ? guide_value(src0, SRC, at + k, lo, hi) : 0.0;
                        v[0][k] = g;
                        v[1][k] = in ? (double)pv[k] : 0.0;   // selected: a NaN outside the region stops here
                        v[2][k] = in ? 1.0 : 0.0;
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int s = 0; s < NS; ++s) stage[s][wv][gx_pos(e0 + k)] = v[s][k];
        }
    }
    __syncthreads();
    const int x = x0 + 4 * lane;
    if (row >= rows || x >= W) return;
    double acc[NF][4];
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[f][k] = 0.0;
    const int first = hb - r + 4 * lane;                      // the staged position of x - r
    for (int t = 0; t < 2 * r + 4; ++t) {
        const int at = gx_pos(first + t);
        double f[NF];
        if constexpr (SRC == GF_SRC_AB) {
            f[0] = stage[0][wv][at];
            f[1] = stage[1][wv][at];
        } else {
            const double g = stage[0][wv][at], pp = stage[1][wv][at];
            f[0] = stage[2][wv][at];
            f[1] = g;
            f[2] = pp;
            f[3] = g * g;
            f[4] = g * pp;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (t >= k && t - k <= 2 * r) {
#pragma unroll
                for (int i = 0; i < NF; ++i) acc[i][k] += f[i];
            }
    }
    const long long o = row * W + x;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        double* d = dst + f * S + o;
        if (vec) {
            *reinterpret_cast<double2*>(d) = make_double2(acc[f][0], acc[f][1]);
            *reinterpret_cast<double2*>(d + 2) = make_double2(acc[f][2], acc[f][3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x + k < W) d[k] = acc[f][k];
        }
    }
}

struct GuidedEpi {
    const uint8_t* mask;
    const void* guide;       // APPLY
    int guide_kind;
    double lo, hi, eps;
    const double* n_in;      // APPLY: N of stage 1
    double* a;               // COEF: a, b, N out
    double* b;
    double* n_out;
    float* q;                // APPLY
};

// src, dst: [NF][outer][L][inner] (field stride S), summed along L.  Block: GA_LT outputs along L x GA_TX columns; blockIdx.x = (o *
// ltiles + lt) * ctiles + ct.  stage[hb + i][c] = src[l0 + i][column c], 0 outside 0 .. L - 1.  Wave ty owns the outputs l0 + 4 ty ..
// + 3, lane tx the columns 2 tx and 2 tx + 1 of the tile.  EPI NONE: dst = the sums.  COEF (NF 5, the last pass of stage 1): step 2.
// APPLY (NF 2, the last pass of stage 2): step 3.
template <int NF, int EPI>
__global__ __launch_bounds__(64 * GA_WAVES) void guided_axis_kernel(const double* __restrict__ src, double* __restrict__ dst, int r, int L,
                                                                     long long inner, long long S, int ctiles, int ltiles, int vec,
                                                                     GuidedEpi epi) {
    __shared__ __attribute__((aligned(16))) double stage[GA_LT + 2 * GF_RMAX][GA_TX];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const long long col = (long long)(blockIdx.x % ctiles) * GA_TX + 2 * tx;
    const long long rest = blockIdx.x / ctiles;
    const int l0 = (int)(rest % ltiles) * GA_LT;
    const long long base = (rest / ltiles) * L * inner + col;
    const int hb = (r + 3) & ~3;
    const bool live0 = col < inner, live1 = col + 1 < inner;
    const int lout = l0 + 4 * ty;
    double acc[NF][4][2];
    for (int f = 0; f < NF; ++f) {
        const double* s = src + f * S + base;
        if (f) __syncthreads();                               // the previous field has been read by every wave
        for (int pz = ty; pz < GA_LT + 2 * hb; pz += GA_WAVES) {
            const int l = l0 - hb + pz;
            double2 v = make_double2(0.0, 0.0);
            if (l >= 0 && l < L && live0) {
                const double* at = s + (long long)l * inner;
                if (vec) {                                    // inner is even: col + 1 < inner
                    v = *reinterpret_cast<const double2*>(at);
                } else {
                    v.x = at[0];
                    if (live1) v.y = at[1];
                }
            }
            *reinterpret_cast<double2*>(&stage[pz][2 * tx]) = v;
        }
        __syncthreads();
        double a[4][2];
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k][0] = a[k][1] = 0.0;
        if (lout < L) {                                       // wave-uniform
            const int first = hb - r + 4 * ty;                // the staged position of lout - r
            for (int t = 0; t < 2 * r + 4; ++t) {
                const double2 v = *reinterpret_cast<const double2*>(&stage[first + t][2 * tx]);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (t >= k && t - k <= 2 * r) {
                        a[k][0] += v.x;
                        a[k][1] += v.y;
                    }
            }
        }
        if constexpr (EPI == GF_EPI_NONE) {
            if (live0) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (lout + k < L) {
                        double* d = dst + f * S + base + (long long)(lout + k) * inner;
                        if (vec) {
                            *reinterpret_cast<double2*>(d) = make_double2(a[k][0], a[k][1]);
                        } else {
                            d[0] = a[k][0];
                            if (live1) d[1] = a[k][1];
                        }
                    }
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                acc[f][k][0] = a[k][0];
                acc[f][k][1] = a[k][1];
            }
        }
    }
    if (EPI == GF_EPI_NONE || !live0) return;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (lout + k >= L) break;
        const long long at = base + (long long)(lout + k) * inner;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if (c == 1 && !live1) break;
            const long long i = at + c;
            const bool in = epi.mask[i] != 0;
            if constexpr (EPI == GF_EPI_COEF) {
                const double n = acc[0][k][c];
                double av = 0.0, bv = 0.0;
                if (in) {                                     // n >= 1
                    const double mg = acc[1][k][c] / n, mp = acc[2][k][c] / n;
                    av = (acc[4][k][c] / n - mg * mp) / ((acc[3][k][c] / n - mg * mg) + epi.eps);
                    bv = mp - av * mg;
                }
                epi.a[i] = av;
                epi.b[i] = bv;
                epi.n_out[i] = n;
            } else if constexpr (EPI == GF_EPI_APPLY) {
                float qv = 0.f;
                if (in) {
                    const double n = epi.n_in[i];
                    const double A = acc[0][k][c] / n, B = acc[1][k][c] / n;
                    qv = (float)(A * guide_value(epi.guide, epi.guide_kind, i, epi.lo, epi.hi) + B);
                }
                epi.q[i] = qv;
            }
        }
    }
}

static inline bool guided_sizes_ok(int D, int H, int W) {
    return D > 0 && H > 0 && W > 0 && (long long)D * H * W < (1LL << 31);
}

template <int NF, int EPI>
static void guided_axis_launch(const double* src, double* dst, int r, long long outer, int L, long long inner, long long S, const GuidedEpi& epi,
                               hipStream_t st) {
    const long long ctiles = cdiv64(inner, GA_TX), ltiles = cdiv(L, GA_LT);      // outer * ltiles * ctiles <= D * H * W < 2^31
    const int vec = inner % 2 == 0;                                              // every base is 16-byte aligned, S is even
    hipLaunchKernelGGL((guided_axis_kernel<NF, EPI>), dim3((unsigned)(outer * ltiles * ctiles)), dim3(64, GA_WAVES), 0, st, src, dst, r, L,
                       inner, S, (int)ctiles, (int)ltiles, vec, epi);
}

}  // namespace dram

using namespace dram;

extern "C" int dram_guided_max_radius(void) { return GF_RMAX; }

extern "C" size_t dram_guided_ws_bytes(int D, int H, int W) {
    if (!guided_sizes_ok(D, H, W)) {
        set_error("guided_ws_bytes: sizes must be positive with D*H*W < 2^31");
        return 0;
    }
    return (size_t)12 * D * H * W * sizeof(double);           // two sets of five fields, and a, b
}

extern "C" int dram_guided_filter(const void* guide, int guide_kind, double lo, double hi, const float* p, const uint8_t* mask,
                                  const int* radius, double eps, int D, int H, int W, float* q, double* ab, void* ws, size_t ws_bytes,
                                  void* stream) {
    DRAM_REQUIRE(guide && p && mask && radius && q && ws, "guided_filter: null pointer");
    DRAM_REQUIRE(guide_kind == DRAM_GUIDE_INT16 || guide_kind == DRAM_GUIDE_FLOAT32,
                 "guided_filter: guide_kind must be DRAM_GUIDE_INT16 or DRAM_GUIDE_FLOAT32");
    DRAM_REQUIRE(guided_sizes_ok(D, H, W), "guided_filter: sizes must be positive with D*H*W < 2^31");
    DRAM_REQUIRE(eps > 0.0 && isfinite(eps), "guided_filter: eps must be positive and finite");
    for (int a = 0; a < 3; ++a)
        DRAM_REQUIRE(radius[a] >= 0 && radius[a] <= GF_RMAX, "guided_filter: radius %d of axis %d is outside 0 .. %d", radius[a], a, GF_RMAX);
    if (guide_kind == DRAM_GUIDE_INT16)
        DRAM_REQUIRE(hi > lo && isfinite(lo) && isfinite(hi), "guided_filter: an int16 guide needs a finite window with hi > lo");
    DRAM_REQUIRE(aligned16(ws) && aligned16(ab), "guided_filter: ws and ab must be 16-byte aligned");
    DRAM_REQUIRE(((uintptr_t)p & 3) == 0 && ((uintptr_t)q & 3) == 0 && ((uintptr_t)guide & (guide_kind == DRAM_GUIDE_INT16 ? 1 : 3)) == 0,
                 "guided_filter: p, q and a float32 guide must be 4-byte, an int16 guide 2-byte aligned");
    if (ws_bytes < dram_guided_ws_bytes(D, H, W)) {
        set_error("guided_filter: workspace too small");
        return DRAM_EWS;
    }
    const long long S = (long long)D * H * W, rows = (long long)D * H, plane = (long long)H * W;
    double* t0 = (double*)ws;                                 // x pass out; t0[0] is N once the y pass of stage 1 has read it
    double* t1 = t0 + 5 * S;                                  // y pass out
    double* abw = ab ? ab : t1 + 5 * S;
    hipStream_t st = (hipStream_t)stream;
    const int xtiles = cdiv(W, GX_T);
    const unsigned xblocks = (unsigned)(cdiv64(rows, GX_ROWS) * xtiles);
    const int vec_raw = W % 4 == 0 && aligned16(p) && ((uintptr_t)mask & 3) == 0, vec_ab = W % 4 == 0;
    GuidedEpi epi = {mask, guide, guide_kind, lo, hi, eps, t0, abw, abw + S, t0, q};
    if (guide_kind == DRAM_GUIDE_INT16)
        hipLaunchKernelGGL(guided_x_kernel<GF_SRC_INT16>, dim3(xblocks), dim3(256), 0, st, guide, p, mask, lo, hi, radius[2], t0, rows, W, S,
                           xtiles, vec_raw);
    else
        hipLaunchKernelGGL(guided_x_kernel<GF_SRC_FLOAT>, dim3(xblocks), dim3(256), 0, st, guide, p, mask, lo, hi, radius[2], t0, rows, W, S,
                           xtiles, vec_raw);
    guided_axis_launch<5, GF_EPI_NONE>(t0, t1, radius[1], D, H, W, S, epi, st);
    guided_axis_launch<5, GF_EPI_COEF>(t1, nullptr, radius[0], 1, D, plane, S, epi, st);
    hipLaunchKernelGGL(guided_x_kernel<GF_SRC_AB>, dim3(xblocks), dim3(256), 0, st, (const void*)abw, nullptr, nullptr, 0.0, 0.0, radius[2],
                       t0 + S, rows, W, S, xtiles, vec_ab);
    guided_axis_launch<2, GF_EPI_NONE>(t0 + S, t1, radius[1], D, H, W, S, epi, st);
    guided_axis_launch<2, GF_EPI_APPLY>(t1, nullptr, radius[0], 1, D, plane, S, epi, st);
    return check_launch("guided_filter");
}
