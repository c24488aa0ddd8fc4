// Lesion texture report at inference (gfx950): per label of a label volume and per direction of the half 26-neighbourhood, in one
// pass over scan and labels, the grey-level co-occurrence table (GLCM) behind Haralick's second-order statistics.  Everything is
// integers, summed by integer atomics, so no result depends on the order in which they land (the same bits every run).
//
// A voxel is staged as one 32-bit word, label << 5 | grey level, 0 for a voxel that belongs to nobody (label outside 1..n, mask
// 0, outside the volume); n * 13 * levels^2 < 2^31 keeps the label below 2^26.  A block of 256 threads takes a tile of
// GLCM_TY x GLCM_TX = 16 x 64 voxels in (y, x) and marches along z over a segment of planes, keeping the distance + 1 planes
// z .. z + distance of the tile with a halo of `distance` in a ring in LDS: a voxel comes from memory once per tile and segment
// (a segment re-reads `distance` planes of the next one) and its 13 forward neighbours come from LDS.  Wave w takes the rows
// 4w .. 4w+3 of the tile, a lane one x, so the LDS reads of a wave are consecutive words.  The interior of a staged row is loaded
// in pieces of 8 voxels, 16-byte loads of the scan and of int32 labels (8-byte loads of uint8 labels and mask) where the piece is
// so aligned and wholly inside the row, single elements otherwise and for the halo.  The scan of a piece whose labels are all
// zero is not read, and a plane of the ring without any labelled voxel is skipped by the whole block.
//
// A thread merges, per direction, the run of equal (label, direction, gi, gj) over its four rows and along the z march, so a
// homogeneous region costs one add per thread, direction and work item rather than one per pair.
//
// dram_label_glcm serves two regimes, chosen by dram_label_glcm_plan from (label_kind, n, levels, distance) alone:
//   GLCM_LDS    n * 13 * levels^2 <= GLCM_LDS_WORDS = 24576 (the lobe map at 16 levels is 16640): the call's table is kept per
//               block in LDS as 32-bit counts beside the staged planes (at most 8640 words: 130 KiB in all) and flushed once
//               with one 64-bit global atomic per occupied entry.  A call covers fewer than 2^31 voxels, so no count wraps.
//   GLCM_WAVE   otherwise.  Finished runs go to global memory directly; at the end of a work item the lanes of a wave that hold
//               the same pending key are reduced together (wave_reduce_by_key, label_stream.h) and the group's first lane
//               sends the 64-bit global atomic.
#include "label_stream.h"

namespace dram {

constexpr int GLCM_LDS = 0, GLCM_WAVE = 1;
constexpr int GLCM_TY = 16, GLCM_TX = 64;                             // the tile; 4 rows per wave, one x per lane
constexpr int GLCM_PIECE = 8;                                         // voxels of an interior row piece
constexpr int GLCM_UNITS = GLCM_TX / GLCM_PIECE + 1;                  // staging units of a row: the pieces and the halo
constexpr int GLCM_DIRS = 13;
constexpr int GLCM_MAX_LEVELS = 32, GLCM_MAX_DISTANCE = 4;
constexpr int GLCM_LDS_WORDS = 24576;                                 // 96 KiB of table beside at most 34 KiB of planes
constexpr int GLCM_MAX_DIM = 32768;
constexpr int GLCM_GRID_LDS = 512, GLCM_GRID_WAVE = 2048;

// direction i = code - 5 of code = dz * 9 + (dy + 1) * 3 + (dx + 1): lexicographic, the first non-zero component positive
__host__ __device__ constexpr int glcm_dz(int dir) { return (dir + 5) / 9; }
__host__ __device__ constexpr int glcm_dy(int dir) { return (dir + 5) / 3 % 3 - 1; }
__host__ __device__ constexpr int glcm_dx(int dir) { return (dir + 5) % 3 - 1; }

struct GlcmArgs {
    const int16_t* scan;
    const void* labels;
    const uint8_t* mask;
    unsigned long long* glcm;
    int n, lo, width, levels, distance, D, H, W;
    int ntx, nseg, zlen, items;              // tiles along x; z segments per tile, planes per segment; tiles * nseg
    int table_words;                         // n * 13 * levels^2
};

__global__ __launch_bounds__(256) void glcm_init_kernel(unsigned long long* __restrict__ glcm, int total) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) glcm[i] = 0;
}

__device__ __forceinline__ unsigned glcm_level(int v, const GlcmArgs& a) {
    const long long diff = (long long)v - a.lo;                       // < 2^32
    if (diff < 0) return 0u;
    const unsigned q = (unsigned)diff / (unsigned)a.width;
    return q < (unsigned)a.levels ? q : (unsigned)a.levels - 1u;
}

// a label outside 1..n belongs to nobody
__device__ __forceinline__ unsigned glcm_valid(int l, int n) { return (unsigned)(l - 1) < (unsigned)n ? (unsigned)l : 0u; }

// the staged word of voxel idx, which lies inside the volume
template <class LabelT>
__device__ __forceinline__ unsigned glcm_word(const GlcmArgs& a, size_t idx) {
    const unsigned l = glcm_valid((int)static_cast<const LabelT*>(a.labels)[idx], a.n);
    if (l == 0 || (a.mask && a.mask[idx] == 0)) return 0u;
    return l << 5 | glcm_level((int)a.scan[idx], a);
}

// 8 elements from p: one vector load (two for 32-bit elements) where p is aligned to min(16, 8 * sizeof(T)) bytes
template <class T>
__device__ __forceinline__ bool glcm_aligned8(const T* p) {
    return (reinterpret_cast<uintptr_t>(p) & (sizeof(T) == 1 ? 7u : 15u)) == 0;
}
__device__ __forceinline__ void glcm_load8(const uint8_t* p, int (&o)[8]) {
    const uint2 v = *reinterpret_cast<const uint2*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) { o[e] = (int)((v.x >> (8 * e)) & 0xffu); o[4 + e] = (int)((v.y >> (8 * e)) & 0xffu); }
}
__device__ __forceinline__ void glcm_load8(const int16_t* p, int (&o)[8]) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) { o[2 * e] = (int)(short)(w[e] & 0xffffu); o[2 * e + 1] = (int)(short)(w[e] >> 16); }
}
__device__ __forceinline__ void glcm_load8(const int32_t* p, int (&o)[8]) {
    const int4 u = reinterpret_cast<const int4*>(p)[0], v = reinterpret_cast<const int4*>(p)[1];
    o[0] = u.x; o[1] = u.y; o[2] = u.z; o[3] = u.w; o[4] = v.x; o[5] = v.y; o[6] = v.z; o[7] = v.w;
}

extern __shared__ unsigned glcm_lds[];

// Stages plane z of the tile at (y0, x0) with its halo into `plane`: every word of it is written.  Returns whether any staged
// voxel of the block carries a label.  Two barriers: before the first write and after the last.
template <class LabelT>
__device__ __forceinline__ bool glcm_stage(const GlcmArgs& a, unsigned* plane, int z, int y0, int x0) {
    const LabelT* labels = static_cast<const LabelT*>(a.labels);
    const int d = a.distance, SW = GLCM_TX + 2 * d, SH = GLCM_TY + 2 * d;
    unsigned any = 0;
    __syncthreads();                                                  // the plane that lay here has been read
    for (int u = threadIdx.x; u < SH * GLCM_UNITS; u += 256) {
        const int r = u / GLCM_UNITS, q = u % GLCM_UNITS;
        const int y = y0 - d + r;
        const bool rowin = z < a.D && y >= 0 && y < a.H;
        const size_t row = ((size_t)z * a.H + (rowin ? y : 0)) * a.W;   // used only when rowin
        unsigned* dst = plane + r * SW;
        if (q < GLCM_TX / GLCM_PIECE) {
            const int x = x0 + q * GLCM_PIECE;
            unsigned w[GLCM_PIECE];
#pragma unroll
            for (int e = 0; e < GLCM_PIECE; ++e) w[e] = 0u;
            if (rowin && x < a.W) {
                const size_t idx = row + x;
                if (x + GLCM_PIECE <= a.W && glcm_aligned8(labels + idx)) {
                    int l[GLCM_PIECE];
                    glcm_load8(labels + idx, l);
                    unsigned some = 0;
#pragma unroll
                    for (int e = 0; e < GLCM_PIECE; ++e) { w[e] = glcm_valid(l[e], a.n); some |= w[e]; }
                    if (some && a.mask) {
                        if (glcm_aligned8(a.mask + idx)) {
                            glcm_load8(a.mask + idx, l);
#pragma unroll
                            for (int e = 0; e < GLCM_PIECE; ++e) w[e] = l[e] ? w[e] : 0u;
                        } else {
#pragma unroll
                            for (int e = 0; e < GLCM_PIECE; ++e) w[e] = a.mask[idx + e] ? w[e] : 0u;
                        }
                        some = 0;
#pragma unroll
                        for (int e = 0; e < GLCM_PIECE; ++e) some |= w[e];
                    }
                    if (some) {                                       // only now the scan
                        if (glcm_aligned8(a.scan + idx)) {
                            glcm_load8(a.scan + idx, l);
#pragma unroll
                            for (int e = 0; e < GLCM_PIECE; ++e) w[e] = w[e] ? (w[e] << 5 | glcm_level(l[e], a)) : 0u;
                        } else {
#pragma unroll
                            for (int e = 0; e < GLCM_PIECE; ++e) w[e] = w[e] ? (w[e] << 5 | glcm_level((int)a.scan[idx + e], a)) : 0u;
                        }
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < GLCM_PIECE; ++e)
                        if (x + e < a.W) w[e] = glcm_word<LabelT>(a, idx + e);
                }
            }
#pragma unroll
            for (int e = 0; e < GLCM_PIECE; ++e) { dst[d + q * GLCM_PIECE + e] = w[e]; any |= w[e]; }
        } else {
            for (int e = 0; e < 2 * d; ++e) {                         // the halo: d columns on either side
                const int pos = e < d ? e : GLCM_TX + e, x = x0 - d + pos;
                const unsigned w = rowin && x >= 0 && x < a.W ? glcm_word<LabelT>(a, row + x) : 0u;
                dst[pos] = w;
                any |= w;
            }
        }
    }
    return __syncthreads_or((int)(any != 0)) != 0;
}

// Where a finished run goes: the block's LDS table or global memory.
template <bool LDS_TABLE>
struct GlcmSink {
    unsigned* table;
    unsigned long long* glcm;
    __device__ __forceinline__ void add(int key, unsigned cnt) const {
        if (LDS_TABLE) atomicAdd(&table[key], cnt);
        else atomicAdd(&glcm[key], (unsigned long long)cnt);
    }
};

template <class LabelT, bool LDS_TABLE>
__global__ __launch_bounds__(256) void label_glcm_kernel(const GlcmArgs a) {
    const int d = a.distance, SW = GLCM_TX + 2 * d, SH = GLCM_TY + 2 * d, PW = SH * SW, L = a.levels, L2 = L * L;
    unsigned* stage = glcm_lds;
    GlcmSink<LDS_TABLE> sink{glcm_lds + (d + 1) * PW, a.glcm};
    if (LDS_TABLE)
        for (int k = threadIdx.x; k < a.table_words; k += 256) sink.table[k] = 0;   // the first staging barrier follows
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int pk[GLCM_DIRS];                                                // per direction the pending key, -1: none, and its count
    unsigned pc[GLCM_DIRS];
#pragma unroll
    for (int i = 0; i < GLCM_DIRS; ++i) { pk[i] = -1; pc[i] = 0; }
    for (int item = blockIdx.x; item < a.items; item += gridDim.x) {  // block-uniform
        const int seg = item % a.nseg, t = item / a.nseg;
        const int y0 = (t / a.ntx) * GLCM_TY, x0 = (t % a.ntx) * GLCM_TX;
        const int za = seg * a.zlen, zb = za + a.zlen < a.D ? za + a.zlen : a.D;
        unsigned anymask = 0;                                         // bit s: the plane in slot s has a labelled voxel
        int fwd = 0;                                                  // the slot of plane z + d; plane z lies one slot further round
        for (int p = 0; p < d; ++p) {
            anymask |= (unsigned)glcm_stage<LabelT>(a, stage + p * PW, za + p, y0, x0) << p;
            fwd = p + 1;
        }
        for (int z = za; z < zb; ++z) {
            const bool some = glcm_stage<LabelT>(a, stage + fwd * PW, z + d, y0, x0);
            anymask = (anymask & ~(1u << fwd)) | (unsigned)some << fwd;
            const int own = fwd == d ? 0 : fwd + 1;
            if ((anymask >> own) & 1u) {                              // block-uniform
                const unsigned *P0 = stage + own * PW, *P1 = stage + fwd * PW;
#pragma unroll
                for (int j = 0; j < GLCM_TY / 4; ++j) {
                    const int c = (wave * (GLCM_TY / 4) + j + d) * SW + lane + d;
                    const unsigned wp = P0[c], lab = wp >> 5;
                    if (lab == 0) continue;
                    const int base = (int)(lab - 1) * GLCM_DIRS * L2 + (int)(wp & 31u) * L;
#pragma unroll
                    for (int i = 0; i < GLCM_DIRS; ++i) {
                        const unsigned wq = (glcm_dz(i) ? P1 : P0)[c + d * (glcm_dy(i) * SW + glcm_dx(i))];
                        if ((wq >> 5) == lab) {
                            const int key = base + i * L2 + (int)(wq & 31u);
                            if (key != pk[i]) {
                                if (pk[i] >= 0) sink.add(pk[i], pc[i]);
                                pk[i] = key;
                                pc[i] = 0;
                            }
                            ++pc[i];
                        }
                    }
                }
            }
            fwd = own;
        }
#pragma unroll
        for (int i = 0; i < GLCM_DIRS; ++i) {                         // reached by all 64 lanes of every wave together
            if constexpr (LDS_TABLE) {
                if (pk[i] >= 0) sink.add(pk[i], pc[i]);
            } else {
                wave_reduce_by_key(pk[i] >= 0, pk[i], WaveSums<unsigned, 1>{{pc[i]}},
                                   [&](int key, const WaveSums<unsigned, 1>& r) { sink.add(key, r.v[0]); });
            }
            pk[i] = -1;
            pc[i] = 0;
        }
    }
    if (LDS_TABLE) {
        __syncthreads();
        for (int e = threadIdx.x; e < a.table_words; e += 256) {
            const unsigned cnt = sink.table[e];
            if (cnt) atomicAdd(&a.glcm[e], (unsigned long long)cnt);
        }
    }
}

static inline bool glcm_shape_ok(int label_kind, int n, int levels, int distance) {
    return label_kind_ok(label_kind, n) && levels >= 2 && levels <= GLCM_MAX_LEVELS && distance >= 1 && distance <= GLCM_MAX_DISTANCE &&
           (int64_t)n * GLCM_DIRS * levels * levels < (1LL << 31);
}

static inline int glcm_regime(int n, int levels) { return (int64_t)n * GLCM_DIRS * levels * levels <= GLCM_LDS_WORDS ? GLCM_LDS : GLCM_WAVE; }

template <class LabelT>
static int glcm_launch(GlcmArgs& a, hipStream_t st) {
    const int d = a.distance;
    const int64_t tiles = cdiv64(a.H, GLCM_TY) * cdiv64(a.W, GLCM_TX);
    const bool lds_table = glcm_regime(a.n, a.levels) == GLCM_LDS;
    const int cap = lds_table ? GLCM_GRID_LDS : GLCM_GRID_WAVE;
    a.ntx = (int)cdiv64(a.W, GLCM_TX);
    // split z into segments of at least 8 * distance planes until there are several items for every block; a segment re-reads
    // `distance` planes of the next
    a.zlen = a.D;
    while (a.zlen >= 16 * d && tiles * cdiv64(a.D, a.zlen) < 4 * (int64_t)cap) a.zlen = (a.zlen + 1) / 2;
    a.nseg = (int)cdiv64(a.D, a.zlen);
    a.items = (int)(tiles * a.nseg);                                  // D * H * W < 2^31 keeps this far below 2^31
    // a block takes at least two items where there are two: the table's zeroing and flush are shared among them
    const int want = (a.items + 1) / 2;
    const unsigned grid = (unsigned)(want < cap ? want : cap);
    const size_t stage_words = (size_t)(d + 1) * (GLCM_TY + 2 * d) * (GLCM_TX + 2 * d);
    if (lds_table) {
        const size_t lds = (stage_words + (size_t)a.table_words) * 4;
        if (lds > 65536) {
            static LdsAttrOnce once;
            const int rc = ensure_dynamic_lds((const void*)label_glcm_kernel<LabelT, true>, lds, once, "label_glcm");
            if (rc != DRAM_OK) return rc;
        }
        hipLaunchKernelGGL((label_glcm_kernel<LabelT, true>), dim3(grid), dim3(256), lds, st, a);
    } else {
        hipLaunchKernelGGL((label_glcm_kernel<LabelT, false>), dim3(grid), dim3(256), stage_words * 4, st, a);
    }
    return DRAM_OK;
}

}  // namespace dram

using namespace dram;

#define GLCM_SHAPE_MSG "label_glcm: label_kind 0 (uint8, n <= 255) or 1 (int32), n >= 1, levels in 2..32, distance in 1..4, n * 13 * levels^2 < 2^31"

extern "C" int dram_label_glcm_plan(int label_kind, int n, int levels, int distance) {
    DRAM_REQUIRE(glcm_shape_ok(label_kind, n, levels, distance), GLCM_SHAPE_MSG);
    return glcm_regime(n, levels);
}

extern "C" int dram_label_glcm(const int16_t* scan, const void* labels, int label_kind, const uint8_t* mask, int n, int lo, int width,
                               int levels, int distance, int64_t* glcm, int D, int H, int W, void* stream) {
    DRAM_REQUIRE(scan && labels && glcm, "label_glcm: null pointer");
    DRAM_REQUIRE(glcm_shape_ok(label_kind, n, levels, distance), GLCM_SHAPE_MSG);
    DRAM_REQUIRE(width >= 1, "label_glcm: width must be at least 1");
    DRAM_REQUIRE(D >= 1 && H >= 1 && W >= 1 && D <= GLCM_MAX_DIM && H <= GLCM_MAX_DIM && W <= GLCM_MAX_DIM,
                 "label_glcm: D, H, W must each be in 1..%d", GLCM_MAX_DIM);
    DRAM_REQUIRE((int64_t)D * H * W < (1LL << 31), "label_glcm: D * H * W < 2^31");
    DRAM_REQUIRE(((uintptr_t)scan & 1) == 0 && (label_kind == 0 || ((uintptr_t)labels & 3) == 0), "label_glcm: misaligned scan or labels");
    hipStream_t st = (hipStream_t)stream;
    GlcmArgs a{};
    a.scan = scan; a.labels = labels; a.mask = mask; a.glcm = (unsigned long long*)glcm;
    a.n = n; a.lo = lo; a.width = width; a.levels = levels; a.distance = distance; a.D = D; a.H = H; a.W = W;
    a.table_words = n * GLCM_DIRS * levels * levels;
    const unsigned init_grid = (unsigned)(cdiv64(a.table_words, 256) < 1024 ? cdiv64(a.table_words, 256) : 1024);
    hipLaunchKernelGGL(glcm_init_kernel, dim3(init_grid), dim3(256), 0, st, a.glcm, a.table_words);
    const int rc = label_kind == 0 ? glcm_launch<uint8_t>(a, st) : glcm_launch<int32_t>(a, st);
    if (rc != DRAM_OK) return rc;
    return check_launch("label_glcm");
}
