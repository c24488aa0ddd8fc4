// Lesion shape report at inference (gfx950): per label of a label volume, in one pass, the histogram of the 2x2x2 neighbourhood
// configurations (the table behind the Minkowski functionals: surface area by Crofton's formula, Euler number) and the moments
// of the voxel positions up to second order.  Everything is integers, summed by integer atomics, so no result depends on the
// order in which they land (the same bits every run).
//
// Cells lie over the zero-padded volume: cell (z, y, x), z in -1..D-1, y in -1..H-1, x in -1..W-1, covers the voxels
// (z+dz, y+dy, x+dx), and bit dz*4 + dy*2 + dx of its configuration for label k says that this voxel carries k.  A block takes
// a tile of 16 x 16 cell rows (one per thread) and marches along x: the 17 x 17 voxel rows under the tile are staged in LDS a
// chunk of 128 bytes per row at a time (16-byte loads where a row piece is 16-byte aligned and wholly inside the row, single
// elements otherwise), so a voxel comes from memory once per tile and is used for the eight cells it touches from LDS and
// registers: a thread keeps the 2x2 plane at x and reads the plane at x+1.  The voxel (z+1, y+1, x+1) of a thread's cell is the
// one whose moments the thread sums, which gives every voxel exactly one owner.
//
// A cell whose eight corners are equal is skipped: all background, or all one label (configuration 255).  Entry 255 follows
// exactly from the rest of the row, because every voxel of a label lies in eight cells and sets one bit in each:
// sum_c popcount(c) * cfg[c] = 8 * count.  A last small kernel solves this for cfg[255].
//
// dram_label_shape serves two regimes, chosen by dram_label_shape_plan from (label_kind, n) alone:
//   SHAPE_LDS   n <= SHAPE_LDS_LABELS: the call's table, n * (256 + 2 * 10) 32-bit words, is kept per block in LDS beside the
//               staged rows and flushed once with one 64-bit global atomic per occupied entry.
//   SHAPE_WAVE  otherwise (component labels).  A thread merges the run of equal (label, configuration) along x and the run of
//               its owned voxels of one label; at the end of a work item the lanes of a wave that hold the same pending
//               (label, configuration), or the same label, are reduced together (wave_reduce_by_key, label_stream.h) and the
//               group's first lane sends the global atomics.  A run that ends inside an item is sent directly.
#include "label_stream.h"
#include <type_traits>

namespace dram {

constexpr int SHAPE_LDS = 0, SHAPE_WAVE = 1;
constexpr int SHAPE_TILE = 16;                                       // cell rows of a tile along z and along y
constexpr int SHAPE_SIDE = SHAPE_TILE + 1;                           // voxel rows under them
constexpr int SHAPE_ROWS = SHAPE_SIDE * SHAPE_SIDE;
constexpr int SHAPE_ROW_DWORDS = 32;                                 // a staged row piece: 128 bytes
constexpr int SHAPE_ROW_STRIDE = SHAPE_ROW_DWORDS + 1;               // odd: the rows of a wave's threads fall on different banks
constexpr int SHAPE_STAGE_WORDS = (SHAPE_ROWS * SHAPE_ROW_STRIDE + 3) / 4 * 4;
constexpr int SHAPE_MOM = 10;
constexpr int SHAPE_LDS_LABELS = 24;                                 // staged rows + 24 * 1104 bytes stay below 64 KiB
constexpr int SHAPE_MAX_GRID = 512;
constexpr int SHAPE_MAX_DIM = 32768;

struct ShapeArgs {
    const void* labels;
    unsigned long long *cfg, *mom;
    int n, D, H, W;
    int nty, nseg, cps, nchunks;             // tiles along y; x segments per tile, chunks per segment, chunks in all
    int items;                               // tiles * nseg
};

template <class LabelT> struct ShapeVoxels;
template <> struct ShapeVoxels<uint8_t> { static constexpr int PER_DWORD = 4; };
template <> struct ShapeVoxels<int32_t> { static constexpr int PER_DWORD = 1; };

__global__ __launch_bounds__(256) void shape_init_kernel(unsigned long long* __restrict__ cfg, unsigned long long* __restrict__ mom, int n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;   // n blocks: one entry of cfg per thread
    cfg[i] = 0;
    if (i < (long long)n * SHAPE_MOM) mom[i] = 0;
}

// cfg[k][255] = (8 * count[k] - sum_{c < 255} popcount(c) * cfg[k][c]) / 8; one wave per label.
__global__ __launch_bounds__(64) void shape_uniform_kernel(unsigned long long* __restrict__ cfg, const unsigned long long* __restrict__ mom) {
    unsigned long long* row = cfg + (size_t)blockIdx.x * 256;
    unsigned long long s = 0;
    for (int c = threadIdx.x; c < 255; c += 64) s += (unsigned long long)__popc((unsigned)c) * row[c];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (threadIdx.x == 0) row[255] = (8ull * mom[(size_t)blockIdx.x * SHAPE_MOM] - s) >> 3;
}

// a label outside 0..n belongs to nobody
__device__ __forceinline__ int shape_valid(int l, int n) { return (unsigned)l <= (unsigned)n ? l : 0; }

// Where a thread's finished runs go: the block's LDS table (32-bit configuration counts: the volume has fewer than 2^32 cells)
// or global memory.
template <class CfgT>
struct ShapeSink {
    CfgT* cfg;
    unsigned long long* mom;
    __device__ __forceinline__ void add_cfg(int key, unsigned cnt) const { atomicAdd(&cfg[key], (CfgT)cnt); }
    __device__ __forceinline__ void add_mom(int label, const unsigned long long (&m)[SHAPE_MOM]) const {
        unsigned long long* row = mom + (size_t)(label - 1) * SHAPE_MOM;
#pragma unroll
        for (int e = 0; e < SHAPE_MOM; ++e)
            if (m[e]) atomicAdd(&row[e], m[e]);
    }
};

// What a thread has pending: the run of equal (label, configuration) along x, key = (label - 1) * 256 + configuration, and the run
// of owned voxels of one label in its row (z, y): their number, the sum of x and the sum of x^2.
struct ShapeRun {
    int key, label;                          // -1 and 0: nothing pending
    unsigned kcnt, cnt, sx;                  // sx < 32768^2 / 2
    unsigned long long sxx;
    __device__ __forceinline__ void reset() { key = -1; label = 0; kcnt = cnt = sx = 0; sxx = 0; }
    // {count, z, y, x, z^2, y^2, x^2, zy, zx, yx} summed over the run
    __device__ __forceinline__ void moments(unsigned z, unsigned y, unsigned long long (&m)[SHAPE_MOM]) const {
        const unsigned long long c = cnt, s = sx;
        m[0] = c; m[1] = z * c; m[2] = y * c; m[3] = s;
        m[4] = (unsigned long long)z * z * c; m[5] = (unsigned long long)y * y * c; m[6] = sxx;
        m[7] = (unsigned long long)z * y * c; m[8] = z * s; m[9] = y * s;
    }
};

// Called by all 64 lanes of a wave together: the pending configuration counts by key, then the pending moments by label.
__device__ __forceinline__ void shape_wave_flush(const ShapeSink<unsigned long long>& sink, const ShapeRun& run, unsigned z, unsigned y) {
    wave_reduce_by_key(run.key >= 0, run.key, WaveSums<unsigned, 1>{{run.kcnt}},
                       [&](int key, const WaveSums<unsigned, 1>& c) { sink.add_cfg(key, c.v[0]); });
    WaveSums<unsigned long long, SHAPE_MOM> m;
    run.moments(z, y, m.v);
    wave_reduce_by_key(run.label > 0, run.label, m, [&](int label, const WaveSums<unsigned long long, SHAPE_MOM>& r) { sink.add_mom(label, r.v); });
}

extern __shared__ unsigned shape_lds[];

// One voxel of global memory, 0 outside the volume; only indices inside the volume are read.
template <class LabelT>
__device__ __forceinline__ int shape_voxel(const LabelT* labels, const ShapeArgs& a, int z, int y, int x) {
    if (z < 0 || z >= a.D || y < 0 || y >= a.H || x < 0 || x >= a.W) return 0;
    return (int)labels[((size_t)z * a.H + y) * a.W + x];
}

template <class LabelT, bool LDS_TABLE>
__global__ __launch_bounds__(256) void label_shape_kernel(const ShapeArgs a) {
    constexpr int VPD = ShapeVoxels<LabelT>::PER_DWORD, XC = SHAPE_ROW_DWORDS * VPD, V16 = 4 * VPD;
    using CfgT = typename std::conditional<LDS_TABLE, unsigned, unsigned long long>::type;
    const LabelT* labels = static_cast<const LabelT*>(a.labels);
    unsigned* stage = shape_lds;
    ShapeSink<CfgT> sink;
    if (LDS_TABLE) {
        unsigned* table = shape_lds + SHAPE_STAGE_WORDS;
        for (int k = threadIdx.x; k < a.n * (2 * SHAPE_MOM + 256); k += 256) table[k] = 0;
        sink.mom = reinterpret_cast<unsigned long long*>(table);
        sink.cfg = reinterpret_cast<CfgT*>(table + 2 * SHAPE_MOM * a.n);
        __syncthreads();
    } else {
        sink.mom = a.mom;
        sink.cfg = reinterpret_cast<CfgT*>(a.cfg);
    }
    const int tj = threadIdx.x & 15, ti = threadIdx.x >> 4;          // the thread's cell row in the tile: y and z
    const unsigned* r00 = stage + (ti * SHAPE_SIDE + tj) * SHAPE_ROW_STRIDE;
    const unsigned *r01 = r00 + SHAPE_ROW_STRIDE, *r10 = r00 + SHAPE_SIDE * SHAPE_ROW_STRIDE, *r11 = r10 + SHAPE_ROW_STRIDE;
    ShapeRun run;
    for (int item = blockIdx.x; item < a.items; item += gridDim.x) {  // block-uniform
        const int seg = item % a.nseg, t = item / a.nseg;
        const int z0 = (t / a.nty) * SHAPE_TILE - 1, y0 = (t % a.nty) * SHAPE_TILE - 1;   // voxel row (0, 0) under the tile
        const int cz = z0 + ti, cy = y0 + tj;                        // the thread's cell row; it owns the voxels of row (cz + 1, cy + 1)
        const int chunk0 = seg * a.cps, chunk1 = chunk0 + a.cps < a.nchunks ? chunk0 + a.cps : a.nchunks;
        const int xp = chunk0 * XC - 1;                              // the plane before the segment's first
        int p00 = shape_valid(shape_voxel(labels, a, cz, cy, xp), a.n), p01 = shape_valid(shape_voxel(labels, a, cz, cy + 1, xp), a.n);
        int p10 = shape_valid(shape_voxel(labels, a, cz + 1, cy, xp), a.n), p11 = shape_valid(shape_voxel(labels, a, cz + 1, cy + 1, xp), a.n);
        run.reset();
        for (int chunk = chunk0; chunk < chunk1; ++chunk) {
            const int xs = chunk * XC;
            __syncthreads();                                         // the previous chunk has been read
            for (int u = threadIdx.x; u < SHAPE_ROWS * 8; u += 256) {
                const int r = u >> 3, q = u & 7;
                const int z = z0 + r / SHAPE_SIDE, y = y0 + r % SHAPE_SIDE, x = xs + q * V16;
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if (z >= 0 && z < a.D && y >= 0 && y < a.H && x < a.W) {
                    const LabelT* p = labels + ((size_t)z * a.H + y) * a.W + x;
                    if (x + V16 <= a.W && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
                        v = *reinterpret_cast<const uint4*>(p);
                    } else {
                        unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                        for (int e = 0; e < V16; ++e)
                            if (x + e < a.W) w[e / VPD] |= (unsigned)p[e] << (8 * sizeof(LabelT) * (e % VPD) % 32);
                        v = make_uint4(w[0], w[1], w[2], w[3]);
                    }
                }
                unsigned* dst = stage + r * SHAPE_ROW_STRIDE + q * 4;
                dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
            }
            __syncthreads();
            const int xend = xs + XC < a.W + 1 ? xs + XC : a.W + 1;   // plane W is the padding: staged as zeros
            for (int q = 0; q < SHAPE_ROW_DWORDS && xs + q * VPD < xend; ++q) {
                const unsigned w00 = r00[q], w01 = r01[q], w10 = r10[q], w11 = r11[q];
#pragma unroll
                for (int b = 0; b < VPD; ++b) {
                    const int x = xs + q * VPD + b;
                    if (x >= xend) break;                            // block-uniform
                    int n00, n01, n10, n11;
                    if (VPD == 4) {
                        n00 = (int)((w00 >> (8 * b)) & 0xffu); n01 = (int)((w01 >> (8 * b)) & 0xffu);
                        n10 = (int)((w10 >> (8 * b)) & 0xffu); n11 = (int)((w11 >> (8 * b)) & 0xffu);
                    } else {
                        n00 = (int)w00; n01 = (int)w01; n10 = (int)w10; n11 = (int)w11;
                    }
                    n00 = shape_valid(n00, a.n); n01 = shape_valid(n01, a.n); n10 = shape_valid(n10, a.n); n11 = shape_valid(n11, a.n);
                    // moments of the owned voxel (cz + 1, cy + 1, x)
                    if (n11 != run.label) {
                        if (run.label > 0) {
                            unsigned long long m[SHAPE_MOM];
                            run.moments((unsigned)(cz + 1), (unsigned)(cy + 1), m);
                            sink.add_mom(run.label, m);
                        }
                        run.label = n11; run.cnt = 0; run.sx = 0; run.sxx = 0;
                    }
                    if (n11 > 0) { ++run.cnt; run.sx += (unsigned)x; run.sxx += (unsigned)x * (unsigned)x; }
                    // the cell (cz, cy, x - 1): bit dz*4 + dy*2 + dx, dx = 0 the kept plane, dx = 1 the new one
                    const int l[8] = {p00, n00, p01, n01, p10, n10, p11, n11};
                    const bool uniform = (p00 == n00) & (p00 == p01) & (p00 == n01) & (p00 == p10) & (p00 == n10) & (p00 == p11) & (p00 == n11);
                    if (!uniform) {
                        unsigned done = 0;
#pragma unroll
                        for (int c0 = 0; c0 < 8; ++c0) {
                            if (l[c0] > 0 && !((done >> c0) & 1u)) {
                                unsigned c = 0;
#pragma unroll
                                for (int c1 = 0; c1 < 8; ++c1) c |= (unsigned)(l[c1] == l[c0]) << c1;
                                done |= c;
                                const int key = (l[c0] - 1) * 256 + (int)c;
                                if (key != run.key) {
                                    if (run.key >= 0) sink.add_cfg(run.key, run.kcnt);
                                    run.key = key;
                                    run.kcnt = 0;
                                }
                                ++run.kcnt;
                            }
                        }
                    }
                    p00 = n00; p01 = n01; p10 = n10; p11 = n11;
                }
            }
        }
        if constexpr (LDS_TABLE) {
            if (run.key >= 0) sink.add_cfg(run.key, run.kcnt);
            if (run.label > 0) {
                unsigned long long m[SHAPE_MOM];
                run.moments((unsigned)(cz + 1), (unsigned)(cy + 1), m);
                sink.add_mom(run.label, m);
            }
        } else {
            shape_wave_flush(sink, run, (unsigned)(cz + 1), (unsigned)(cy + 1));
        }
    }
    if (LDS_TABLE) {
        __syncthreads();
        const unsigned long long* lmom = sink.mom;
        const unsigned* lcfg = reinterpret_cast<const unsigned*>(sink.cfg);
        for (int e = threadIdx.x; e < a.n * SHAPE_MOM; e += 256)
            if (lmom[e]) atomicAdd(&a.mom[e], lmom[e]);
        for (int e = threadIdx.x; e < a.n * 256; e += 256)
            if (lcfg[e]) atomicAdd(&a.cfg[e], (unsigned long long)lcfg[e]);
    }
}

static inline bool shape_labels_ok(int label_kind, int n) {
    return label_kind_ok(label_kind, n) && (int64_t)n * 256 < (1LL << 31);
}

static inline int shape_regime(int n) { return n <= SHAPE_LDS_LABELS ? SHAPE_LDS : SHAPE_WAVE; }

template <class LabelT>
static void shape_launch(ShapeArgs& a, hipStream_t st) {
    constexpr int XC = SHAPE_ROW_DWORDS * ShapeVoxels<LabelT>::PER_DWORD;
    const int64_t tiles = cdiv64(a.D + 1, SHAPE_TILE) * cdiv64(a.H + 1, SHAPE_TILE);
    a.nty = (int)cdiv64(a.H + 1, SHAPE_TILE);
    a.nchunks = (int)cdiv64(a.W + 1, XC);
    // split x into segments of at least two chunks until there are blocks for every CU; a segment re-reads one plane from global
    // memory
    a.cps = a.nchunks;
    while (a.cps > 2 && tiles * cdiv64(a.nchunks, a.cps) < SHAPE_MAX_GRID) a.cps = (a.cps + 1) / 2;
    a.nseg = (int)cdiv64(a.nchunks, a.cps);
    a.items = (int)(tiles * a.nseg);                                 // D * H * W < 2^31 keeps this far below 2^31
    const unsigned grid = (unsigned)(a.items < SHAPE_MAX_GRID ? a.items : SHAPE_MAX_GRID);
    if (shape_regime(a.n) == SHAPE_LDS) {
        const size_t lds = (size_t)(SHAPE_STAGE_WORDS + a.n * (2 * SHAPE_MOM + 256)) * 4;
        hipLaunchKernelGGL((label_shape_kernel<LabelT, true>), dim3(grid), dim3(256), lds, st, a);
    } else {
        hipLaunchKernelGGL((label_shape_kernel<LabelT, false>), dim3(grid), dim3(256), (size_t)SHAPE_STAGE_WORDS * 4, st, a);
    }
}

}  // namespace dram

using namespace dram;

#define SHAPE_LABELS_MSG "label_shape: label_kind 0 (uint8, n <= 255) or 1 (int32), n >= 1, n * 256 < 2^31"

extern "C" int dram_label_shape_plan(int label_kind, int n) {
    DRAM_REQUIRE(shape_labels_ok(label_kind, n), SHAPE_LABELS_MSG);
    return shape_regime(n);
}

extern "C" int dram_label_shape(const void* labels, int label_kind, int n, int64_t* cfg, int64_t* mom, int D, int H, int W, void* stream) {
    DRAM_REQUIRE(labels && cfg && mom, "label_shape: null pointer");
    DRAM_REQUIRE(shape_labels_ok(label_kind, n), SHAPE_LABELS_MSG);
    DRAM_REQUIRE(D >= 1 && H >= 1 && W >= 1 && D <= SHAPE_MAX_DIM && H <= SHAPE_MAX_DIM && W <= SHAPE_MAX_DIM,
                 "label_shape: D, H, W must each be in 1..%d", SHAPE_MAX_DIM);
    DRAM_REQUIRE((int64_t)D * H * W < (1LL << 31), "label_shape: D * H * W < 2^31");
    DRAM_REQUIRE(label_kind == 0 || ((uintptr_t)labels & 3) == 0, "label_shape: misaligned labels");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(shape_init_kernel, dim3((unsigned)n), dim3(256), 0, st, (unsigned long long*)cfg, (unsigned long long*)mom, n);
    ShapeArgs a{};
    a.labels = labels; a.cfg = (unsigned long long*)cfg; a.mom = (unsigned long long*)mom;
    a.n = n; a.D = D; a.H = H; a.W = W;
    if (label_kind == 0) shape_launch<uint8_t>(a, st);
    else shape_launch<int32_t>(a, st);
    hipLaunchKernelGGL(shape_uniform_kernel, dim3((unsigned)n), dim3(64), 0, st, (unsigned long long*)cfg, (const unsigned long long*)mom);
    return check_launch("label_shape");
}
