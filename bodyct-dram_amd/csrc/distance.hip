// Surface-distance metrics at inference (gfx950): the exact Euclidean distance transform of a feature mask with anisotropic
// voxel spacing, the 6-neighbour surface of a mask, and the compaction of a distance map over a surface.
//
// dist[v] = (float) sqrt(d2[v]),  d2[v] = min over features f of  fl(fl(fl(dx^2 * wx) + fl(dy^2 * wy)) + fl(dz^2 * wz))
// in fp64, wx = fl(sx * sx) etc. formed on the host.  dx, dy, dz are integers below 2^12, so their squares are exact and every
// term has ONE rounding (the product with w), every sum one more.  Rounded addition is monotone (a <= b  =>  fl(a + c) <=
// fl(b + c)), so a minimum commutes with it and three separable passes give exactly that value:
//   edt_x      per row, the integer |dx| to the nearest feature of the row, EDT_NONE for a row without one
//   edt_axis   along y:  g2[i] = min_j fl(g1[j] + fl((i - j)^2 * wy)),  g1[j] = fl(dx[j]^2 * wx), +inf for EDT_NONE
//   edt_axis   along z:  the same on g2 with wz, then the square root and the conversion to float
// A row, or a whole plane, without a feature carries +inf through a pass (inf + c = inf, and min leaves the other operand)
// and is resolved by a later one; a volume without a feature ends as +inf everywhere.  No product is ever fused with a sum:
// the file is compiled with floating-point contraction off (the pragma below), since an fma would skip the product's rounding.
//
// edt_axis: a block owns (the whole line along the axis) x (EDT_TX adjacent columns of the contiguous dimension), so every
// global access runs along x.  It walks the line in laps of EDT_OC outputs -- a thread keeps the running minima of EDT_R
// consecutive outputs in registers -- and, per lap, stages the line in chunks of EDT_SC sources in LDS.  A thread takes EDT_S
// sources at a time: the EDT_R x EDT_S pairs need only EDT_R + EDT_S - 1 distinct costs fl((i - j)^2 * w), so a pair costs
// little more than its add and its min.  A chunk that holds no finite source is skipped (decided by the whole block).  The
// plain O(L^2) minimum per line; a lower-envelope pass would have to reproduce the same bits.
#include <math.h>
#include "common.h"

#pragma clang fp contract(off)

namespace dram {

constexpr int EDT_MAX_DIM = 4096;   // per dimension: edt_x keeps one 64-voxel ballot per lane (64 * 64), and (i - j)^2 < 2^24
constexpr int EDT_NONE = -1;        // edt_x: no feature in this row
constexpr int EDT_TX = 64;          // columns per block of edt_axis: one wave = one 512-byte row piece of doubles
constexpr int EDT_TY = 4;           // waves per block
constexpr int EDT_R = 16;           // consecutive outputs per thread
constexpr int EDT_OC = EDT_TY * EDT_R;   // outputs per lap of a block
constexpr int EDT_SC = 64;          // sources per LDS chunk
constexpr int EDT_S = 8;            // sources a thread takes at a time

// One wave per row.  First sweep: the ballot of chunk c (voxels 64c .. 64c + 63) goes to lane c.  Two wave scans then give every
// chunk the last feature before it and the first one after it; the second sweep resolves each voxel from its own chunk's
// ballot or from those two.
__global__ __launch_bounds__(256) void edt_x_kernel(const uint8_t* __restrict__ feature, int* __restrict__ dx, long long rows, int W) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                  // wave-uniform
    const uint8_t* f = feature + row * W;
    int* out = dx + row * W;
    const int nchunks = (W + 63) >> 6;                        // <= 64 (EDT_MAX_DIM)
    unsigned long long mine = 0;
    for (int c = 0; c < nchunks; ++c) {
        const int x = c * 64 + lane;
        const unsigned long long b = __ballot(x < W && f[x] != 0);
        if (lane == c) mine = b;
    }
    int last = mine ? lane * 64 + 63 - __clzll((long long)mine) : -1;
    int first = mine ? lane * 64 + __ffsll((long long)mine) - 1 : INT_MAX;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(last, o, 64), u = __shfl_down(first, o, 64);
        if (lane >= o) last = max(last, t);
        if (lane + o < 64) first = min(first, u);
    }
    int prev = __shfl_up(last, 1, 64), next = __shfl_down(first, 1, 64);
    if (lane == 0) prev = -1;
    if (lane == 63) next = INT_MAX;
    for (int c = 0; c < nchunks; ++c) {
        const unsigned long long m = __shfl(mine, c, 64);
        const int p = __shfl(prev, c, 64), n = __shfl(next, c, 64);
        const int x = c * 64 + lane;
        const unsigned long long lo = m & (~0ull >> (63 - lane)), hi = m >> lane;
        const int left = lo ? c * 64 + 63 - __clzll((long long)lo) : p;
        const int right = hi ? x + __ffsll((long long)hi) - 1 : n;
        int d = INT_MAX;
        if (left >= 0) d = x - left;
        if (right != INT_MAX) d = min(d, right - x);
        if (x < W) out[x] = d == INT_MAX ? EDT_NONE : d;
    }
}

__device__ __forceinline__ double edt_source(const int* src, long long i, double wx) {
    const int v = src[i];
    return v < 0 ? (double)INFINITY : (double)(v * v) * wx;
}
__device__ __forceinline__ double edt_source(const double* src, long long i, double) { return src[i]; }
__device__ __forceinline__ void edt_result(double* dst, long long i, double d2) { dst[i] = d2; }
__device__ __forceinline__ void edt_result(float* dst, long long i, double d2) { dst[i] = (float)sqrt(d2); }

// src, dst: [outer][L][inner].  Block b: outer index b / tiles, columns (b % tiles) * EDT_TX ...  Every loop bound and the
// skip of a chunk are uniform over the block, so every thread reaches every barrier.
template <typename Src, typename Dst>
__global__ __launch_bounds__(EDT_TX* EDT_TY) void edt_axis_kernel(const Src* __restrict__ src, Dst* __restrict__ dst, double w, double wx,
                                                                   int L, long long inner, int tiles) {
    __shared__ double stage[EDT_SC][EDT_TX];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const long long col = (long long)(blockIdx.x % tiles) * EDT_TX + tx;
    const long long base = (long long)(blockIdx.x / tiles) * L * inner + col;
    const bool live = col < inner;
    for (int ob = 0; ob < L; ob += EDT_OC) {
        const int i0 = ob + ty * EDT_R;
        double m[EDT_R];
#pragma unroll
        for (int r = 0; r < EDT_R; ++r) m[r] = (double)INFINITY;
        for (int sb = 0; sb < L; sb += EDT_SC) {
            __syncthreads();                                  // the previous chunk has been read
            int finite = 0;
            for (int k = ty; k < EDT_SC; k += EDT_TY) {
                const int j = sb + k;
                const double g = live && j < L ? edt_source(src, base + (long long)j * inner, wx) : (double)INFINITY;
                stage[k][tx] = g;
                finite |= g < (double)INFINITY;
            }
            if (!__syncthreads_or(finite)) continue;
            for (int s0 = 0; s0 < EDT_SC; s0 += EDT_S) {
                // output i0 + r against source sb + s0 + s: delta = first + (r - s + EDT_S - 1)
                const int first = i0 - (sb + s0) - (EDT_S - 1);
                double cost[EDT_R + EDT_S - 1], g[EDT_S];
#pragma unroll
                for (int k = 0; k < EDT_R + EDT_S - 1; ++k) cost[k] = (double)((first + k) * (first + k)) * w;
#pragma unroll
                for (int s = 0; s < EDT_S; ++s) g[s] = stage[s0 + s][tx];
#pragma unroll
                for (int s = 0; s < EDT_S; ++s)
#pragma unroll
                    for (int r = 0; r < EDT_R; ++r) m[r] = fmin(m[r], g[s] + cost[r - s + EDT_S - 1]);
            }
        }
#pragma unroll
        for (int r = 0; r < EDT_R; ++r)
            if (live && i0 + r < L) edt_result(dst, base + (long long)(i0 + r) * inner, m[r]);
    }
}

// One thread per voxel; neighbours by (z, y, x) with a bounds check per axis.  A wave adds its count once.
__global__ __launch_bounds__(256) void mask_surface_kernel(const uint8_t* __restrict__ mask, uint8_t* __restrict__ surf,
                                                           unsigned long long* count, int D, int H, int W) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long nvox = (long long)D * H * W, plane = (long long)H * W;
    bool s = false;
    if (i < nvox) {
        if (mask[i]) {
            const int x = (int)(i % W);
            const long long row = i / W;
            const int y = (int)(row % H), z = (int)(row / H);
            s = x == 0 || !mask[i - 1] || x == W - 1 || !mask[i + 1] || y == 0 || !mask[i - W] || y == H - 1 || !mask[i + W] ||
                z == 0 || !mask[i - plane] || z == D - 1 || !mask[i + plane];
        }
        surf[i] = s;
    }
    const unsigned long long b = __ballot(s);
    if (b && (threadIdx.x & 63) == 0) atomicAdd(count, (unsigned long long)__popcll(b));
}

// A wave reserves its surface voxels' slots with one atomic; slots at or past `capacity` are not written (the cursor still
// counts them, so the caller can tell).
__global__ __launch_bounds__(256) void surface_gather_kernel(const uint8_t* __restrict__ surf, const float* __restrict__ dist,
                                                             float* __restrict__ out, unsigned long long* cursor, long long capacity,
                                                             long long nvox) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool s = i < nvox && surf[i] != 0;
    const unsigned long long b = __ballot(s);
    if (!b) return;                                           // wave-uniform
    const int leader = __ffsll((long long)b) - 1;
    unsigned long long at = 0;
    if (lane == leader) at = atomicAdd(cursor, (unsigned long long)__popcll(b));
    at = __shfl(at, leader, 64);
    const long long slot = (long long)at + __popcll(b & ((1ull << lane) - 1ull));
    if (s && slot < capacity) out[slot] = dist[i];
}

static inline bool edt_sizes_ok(int D, int H, int W) {
    return D > 0 && H > 0 && W > 0 && D <= EDT_MAX_DIM && H <= EDT_MAX_DIM && W <= EDT_MAX_DIM && (long long)D * H * W < (1LL << 31);
}
static inline bool edt_spacing_ok(double s) { return s > 0.0 && s <= 1e6; }    // also refuses NaN and inf; (s * s) * 2^24 finite

// dx: int32 [nvox], then g2: fp64 [nvox] from the next 8-byte boundary
static inline size_t edt_g2_offset(long long nvox) { return align_up((size_t)nvox * sizeof(int), 8); }

template <typename Src, typename Dst>
static void edt_axis_launch(const Src* src, Dst* dst, double w, double wx, long long outer, int L, long long inner, hipStream_t st) {
    const long long tiles = cdiv64(inner, EDT_TX);            // outer * tiles <= D * H * W < 2^31
    hipLaunchKernelGGL((edt_axis_kernel<Src, Dst>), dim3((unsigned)(outer * tiles)), dim3(EDT_TX, EDT_TY), 0, st, src, dst, w, wx, L,
                       inner, (int)tiles);
}

}  // namespace dram

using namespace dram;

extern "C" int dram_edt_max_dim(void) { return EDT_MAX_DIM; }

extern "C" size_t dram_edt_ws_bytes(int D, int H, int W) {
    if (!edt_sizes_ok(D, H, W)) {
        set_error("edt_ws_bytes: sizes must be in 1 .. %d with D*H*W < 2^31", EDT_MAX_DIM);
        return 0;
    }
    const long long nvox = (long long)D * H * W;
    return edt_g2_offset(nvox) + (size_t)nvox * sizeof(double);
}

extern "C" int dram_edt(const uint8_t* feature, float* dist, double sz, double sy, double sx, int D, int H, int W, void* ws,
                        size_t ws_bytes, void* stream) {
    DRAM_REQUIRE(feature && dist && ws, "edt: null pointer");
    DRAM_REQUIRE(edt_sizes_ok(D, H, W), "edt: sizes must be in 1 .. %d with D*H*W < 2^31", EDT_MAX_DIM);
    DRAM_REQUIRE(edt_spacing_ok(sz) && edt_spacing_ok(sy) && edt_spacing_ok(sx), "edt: spacing must be positive and at most 1e6");
    DRAM_REQUIRE(((uintptr_t)ws & 7) == 0 && ((uintptr_t)dist & 3) == 0, "edt: workspace must be 8-byte, dist 4-byte aligned");
    if (ws_bytes < dram_edt_ws_bytes(D, H, W)) {
        set_error("edt: workspace too small");
        return DRAM_EWS;
    }
    const long long nvox = (long long)D * H * W, rows = (long long)D * H;
    int* dx = (int*)ws;
    double* g2 = (double*)((char*)ws + edt_g2_offset(nvox));
    const double wz = sz * sz, wy = sy * sy, wx = sx * sx;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(edt_x_kernel, dim3((unsigned)cdiv64(rows, 4)), dim3(256), 0, st, feature, dx, rows, W);
    edt_axis_launch((const int*)dx, g2, wy, wx, D, H, W, st);
    edt_axis_launch((const double*)g2, dist, wz, 0.0, 1, D, (long long)H * W, st);
    return check_launch("edt");
}

extern "C" int dram_mask_surface(const uint8_t* mask, uint8_t* surf, int64_t* count, int D, int H, int W, void* stream) {
    DRAM_REQUIRE(mask && surf && count, "mask_surface: null pointer");
    DRAM_REQUIRE(D > 0 && H > 0 && W > 0 && (long long)D * H * W < (1LL << 31), "mask_surface: sizes must be positive with D*H*W < 2^31");
    DRAM_REQUIRE(((uintptr_t)count & 7) == 0, "mask_surface: count must be 8-byte aligned");
    const long long nvox = (long long)D * H * W;
    hipStream_t st = (hipStream_t)stream;
    (void)hipMemsetAsync(count, 0, sizeof(int64_t), st);
    hipLaunchKernelGGL(mask_surface_kernel, dim3((unsigned)cdiv64(nvox, 256)), dim3(256), 0, st, mask, surf, (unsigned long long*)count,
                       D, H, W);
    return check_launch("mask_surface");
}

extern "C" int dram_surface_gather(const uint8_t* surf, const float* dist, float* out, int64_t* cursor, int64_t capacity, int64_t nvox,
                                   void* stream) {
    DRAM_REQUIRE(surf && dist && cursor, "surface_gather: null pointer");
    DRAM_REQUIRE(capacity >= 0 && (out || capacity == 0), "surface_gather: out must hold capacity floats");
    DRAM_REQUIRE(nvox > 0 && nvox < (1LL << 31), "surface_gather: nvox must be in 1 .. 2^31 - 1");
    DRAM_REQUIRE(((uintptr_t)cursor & 7) == 0, "surface_gather: cursor must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    (void)hipMemsetAsync(cursor, 0, sizeof(int64_t), st);
    hipLaunchKernelGGL(surface_gather_kernel, dim3((unsigned)cdiv64(nvox, 256)), dim3(256), 0, st, surf, dist, out,
                       (unsigned long long*)cursor, (long long)capacity, (long long)nvox);
    return check_launch("surface_gather");
}
