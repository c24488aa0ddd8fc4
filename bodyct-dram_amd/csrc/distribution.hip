// Lesion distribution report at inference (gfx950): per label of a label volume, the reduction of a depth map (the distance of
// every voxel from the lung surface, dram_edt) and of the voxel positions in one pass -- count, a fixed-point depth sum, the
// minimum and maximum depth as bit patterns, the sums of the voxel indices, a depth histogram in the row layout of
// dram_hist_summary and the counts per positional zone of a box.  Everything is integers: sums, minima and maxima by integer
// atomics and integer reductions, so no result depends on the order in which they land (the same bits every run).
//
// dram_label_depth serves two regimes, chosen by dram_label_depth_plan from (label_kind, n, nbins, nzones) alone:
//   DEPTH_LDS   the whole table of the call -- n * (11 + nbins + 2 + nzones) 32-bit words -- fits in DEPTH_LDS_WORDS of LDS (the
//               lobe map).  One table per block, the pattern of DensLdsAcc (density.hip): a thread keeps the moments of its
//               current label in registers and goes to LDS when the label changes; a histogram or zone count is one 32-bit LDS
//               atomic; at the end one 64-bit global atomic per occupied entry.
//   DEPTH_WAVE  the table does not fit (component labels).  A thread folds its 16 voxels into the run of its current label; at
//               the end of a lap the lanes of a wave that hold the same label are reduced together (a ballot elects the leader)
//               and the leader sends one set of global atomics.  A label change inside a thread's 16 voxels sends the finished
//               run directly.  Histogram and zone counts go to global memory, equal consecutive entries of a thread merged.
// Both stream 16 voxels per thread with 16-byte loads where depth, labels and mask are 16-byte aligned, and fall back to one
// voxel per thread otherwise and for the last nvox % 16 voxels.  A group of 16 voxels may cross the end of a row and of a plane:
// the position of its first voxel is decoded by division and carried from voxel to voxel.  The zone of an index along an axis
// is the number of zone thresholds at or below it (at most 7, formed on the host from the box), which is the clamped quotient of
// the definition without a division.
#include "common.h"

namespace dram {

constexpr int DEPTH_LDS = 0, DEPTH_WAVE = 1;
constexpr int DEPTH_MAX_BINS = 4096;
constexpr int DEPTH_MAX_AXIS_ZONES = 8;
constexpr int DEPTH_MOM_WORDS = 11;           // per label in LDS: depth sum (2 words), index sums z, y, x (6), count, min, max
constexpr int DEPTH_LDS_WORDS = 32768;        // 128 of the CU's 160 KiB
constexpr int DEPTH_BIG_BYTES = 16384;        // a table above this: 1024 threads and one block per CU instead of 256 and eight
constexpr unsigned DEPTH_INF_BITS = 0x7f800000u;
constexpr int DEPTH_NO_THRESHOLD = INT32_MAX;  // no voxel index reaches it: D * H * W < 2^31

struct DepthArgs {
    const float* depth;
    const void* labels;
    const uint8_t* mask;
    unsigned long long *count, *qsum;
    unsigned *dmin, *dmax;
    unsigned long long *possum, *hist, *zones;
    int n, nbins, nzt;                        // nzt: entries of a zones row
    float bins_per_mm;
    int ny, nx;                               // zones along y and x (those along z only enter through tz)
    int tz[DEPTH_MAX_AXIS_ZONES - 1], ty[DEPTH_MAX_AXIS_ZONES - 1], tx[DEPTH_MAX_AXIS_ZONES - 1];
    unsigned H, W, HW;
    long long nvox, groups;                   // groups of 16 voxels taken with 16-byte loads; the rest goes voxel by voxel
};

__global__ __launch_bounds__(256) void depth_init_kernel(unsigned long long* __restrict__ count, unsigned long long* __restrict__ qsum,
                                                         unsigned* __restrict__ dmin, unsigned* __restrict__ dmax,
                                                         unsigned long long* __restrict__ possum, unsigned long long* __restrict__ hist,
                                                         unsigned long long* __restrict__ zones, int n, long long nhist, long long nzones) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) { count[i] = 0; qsum[i] = 0; dmin[i] = DEPTH_INF_BITS; dmax[i] = 0; }
    if (i < 3LL * n) possum[i] = 0;
    if (hist && i < nhist) hist[i] = 0;
    if (zones && i < nzones) zones[i] = 0;
}

// the comparison comes before the conversion: +inf and everything at or above nbins / bins_per_mm go to the overflow entry
__device__ __forceinline__ int depth_bin(float d, float bins_per_mm, int nbins) {
    const float b = d * bins_per_mm;         // bins_per_mm is a power of two: exact
    return b >= (float)nbins ? nbins + 1 : 1 + (int)b;
}

// 2^21 * 2^10 = 2^31 at most: the product is exact and fits the unsigned conversion
__device__ __forceinline__ unsigned depth_q(float d) { return (unsigned)(fminf(d, 2097152.0f) * 1024.0f); }

__device__ __forceinline__ int depth_axis_zone(int i, const int (&t)[DEPTH_MAX_AXIS_ZONES - 1]) {
    int s = 0;
#pragma unroll
    for (int j = 0; j < DEPTH_MAX_AXIS_ZONES - 1; ++j) s += i >= t[j];
    return s;
}

// The position of a voxel and its zone, carried along the flat index.
template <bool ZONES>
struct DepthPos {
    unsigned z, y, x;
    int zz, zy, zx;
    __device__ __forceinline__ DepthPos(const DepthArgs& a, unsigned e) {
        z = e / a.HW;
        const unsigned r = e - z * a.HW;
        y = r / a.W;
        x = r - y * a.W;
        zz = zy = zx = 0;
        if (ZONES) {
            zz = depth_axis_zone((int)z, a.tz);
            zy = a.ny > 1 ? depth_axis_zone((int)y, a.ty) : 0;
            zx = a.nx > 1 ? depth_axis_zone((int)x, a.tx) : 0;
        }
    }
    __device__ __forceinline__ void step(const DepthArgs& a) {
        if (++x == a.W) {
            x = 0;
            if (++y == a.H) {
                y = 0;
                ++z;
                if (ZONES) zz = depth_axis_zone((int)z, a.tz);
            }
            if (ZONES) zy = a.ny > 1 ? depth_axis_zone((int)y, a.ty) : 0;
        }
        if (ZONES) zx = a.nx > 1 ? depth_axis_zone((int)x, a.tx) : 0;
    }
    __device__ __forceinline__ int zone(const DepthArgs& a) const { return (zz * a.ny + zy) * a.nx + zx; }
};

// What a thread has seen of one label since the label last changed.
struct DepthRun {
    int label;                               // 0: nothing pending
    unsigned cnt, mn, mx;
    unsigned long long q, pz, py, px;
    __device__ __forceinline__ void reset(int l) { label = l; cnt = 0; mn = DEPTH_INF_BITS; mx = 0; q = 0; pz = 0; py = 0; px = 0; }
    __device__ __forceinline__ void add(float d, unsigned z, unsigned y, unsigned x) {
        const unsigned bits = __float_as_uint(d);
        ++cnt;
        q += depth_q(d);
        mn = bits < mn ? bits : mn;
        mx = bits > mx ? bits : mx;
        pz += z; py += y; px += x;
    }
};

extern __shared__ unsigned long long depth_lds[];

// DEPTH_LDS: the block's table {qsum[n], possum[3][n] (64-bit), count[n], min[n], max[n], hist[n][nbins + 2], zones[n][nzt]
// (32-bit)}.  A block covers at most 2^23 voxels (see the launch), so the 32-bit counts cannot wrap.
struct DepthLdsAcc {
    unsigned long long *lq, *lp;
    unsigned *lcnt, *lmn, *lmx, *lhist, *lzone;
    int n, nbins, row, nzt;
    float bpm;
    DepthRun run;
    __device__ __forceinline__ DepthLdsAcc(const DepthArgs& a) : n(a.n), nbins(a.nbins), row(a.nbins + 2), nzt(a.nzt), bpm(a.bins_per_mm) {
        lq = depth_lds;
        lp = lq + n;
        lcnt = reinterpret_cast<unsigned*>(lp + 3 * n);
        lmn = lcnt + n;
        lmx = lmn + n;
        lhist = lmx + n;
        lzone = lhist + (a.hist ? n * row : 0);
        const int words = n * (DEPTH_MOM_WORDS + (a.hist ? row : 0) + (a.zones ? nzt : 0));
        unsigned* w = reinterpret_cast<unsigned*>(depth_lds);
        for (int k = threadIdx.x; k < words; k += blockDim.x) w[k] = 0;
        __syncthreads();
        for (int k = threadIdx.x; k < n; k += blockDim.x) lmn[k] = DEPTH_INF_BITS;
        __syncthreads();
        run.reset(0);
    }
    __device__ __forceinline__ void flush() {
        if (run.label > 0) {
            const int k = run.label - 1;
            atomicAdd(&lcnt[k], run.cnt);
            atomicAdd(&lq[k], run.q);
            atomicMin(&lmn[k], run.mn);
            atomicMax(&lmx[k], run.mx);
            atomicAdd(&lp[3 * k], run.pz);
            atomicAdd(&lp[3 * k + 1], run.py);
            atomicAdd(&lp[3 * k + 2], run.px);
        }
    }
    template <bool HIST, bool ZONES>
    __device__ __forceinline__ void add(const DepthArgs& a, int l, float d, const DepthPos<ZONES>& p) {
        if (l < 1 || l > n || !(d >= 0.0f)) return;
        if (l != run.label) { flush(); run.reset(l); }
        run.add(d, p.z, p.y, p.x);
        if (HIST) atomicAdd(&lhist[(l - 1) * row + depth_bin(d, bpm, nbins)], 1u);
        if (ZONES) atomicAdd(&lzone[(l - 1) * nzt + p.zone(a)], 1u);
    }
    __device__ __forceinline__ void end_lap() {}
    __device__ __forceinline__ void finish(const DepthArgs& a) {
        flush();
        __syncthreads();
        for (int k = threadIdx.x; k < n; k += blockDim.x) {
            const unsigned c = lcnt[k];
            if (c) {
                atomicAdd(&a.count[k], (unsigned long long)c);
                if (lq[k]) atomicAdd(&a.qsum[k], lq[k]);
                atomicMin(&a.dmin[k], lmn[k]);
                atomicMax(&a.dmax[k], lmx[k]);
#pragma unroll
                for (int c3 = 0; c3 < 3; ++c3)
                    if (lp[3 * k + c3]) atomicAdd(&a.possum[3 * k + c3], lp[3 * k + c3]);
            }
        }
        if (a.hist) {
            for (int e = threadIdx.x; e < n * row; e += blockDim.x) {
                const unsigned c = lhist[e];
                if (c) atomicAdd(&a.hist[e], (unsigned long long)c);
            }
        }
        if (a.zones) {
            for (int e = threadIdx.x; e < n * nzt; e += blockDim.x) {
                const unsigned c = lzone[e];
                if (c) atomicAdd(&a.zones[e], (unsigned long long)c);
            }
        }
    }
};

// DEPTH_WAVE: runs in registers, one set of global atomics per label and wave at the end of a lap.
struct DepthWaveAcc {
    const DepthArgs& a;
    int n, nbins, row, nzt;
    float bpm;
    DepthRun run;
    long long hcur, zcur;                    // pending histogram and zone entries, -1: none
    unsigned hcnt, zcnt;
    __device__ __forceinline__ DepthWaveAcc(const DepthArgs& a_) : a(a_), n(a_.n), nbins(a_.nbins), row(a_.nbins + 2), nzt(a_.nzt), bpm(a_.bins_per_mm) {
        run.reset(0);
        hcur = zcur = -1;
        hcnt = zcnt = 0;
    }
    __device__ __forceinline__ void send(int label, unsigned cnt, unsigned long long q, unsigned mn, unsigned mx, unsigned long long pz,
                                         unsigned long long py, unsigned long long px) {
        const int k = label - 1;
        atomicAdd(&a.count[k], (unsigned long long)cnt);
        if (q) atomicAdd(&a.qsum[k], q);
        atomicMin(&a.dmin[k], mn);
        atomicMax(&a.dmax[k], mx);
        if (pz) atomicAdd(&a.possum[3 * (size_t)k], pz);
        if (py) atomicAdd(&a.possum[3 * (size_t)k + 1], py);
        if (px) atomicAdd(&a.possum[3 * (size_t)k + 2], px);
    }
    __device__ __forceinline__ void flush_tables() {
        if (hcur >= 0) atomicAdd(&a.hist[hcur], (unsigned long long)hcnt);
        if (zcur >= 0) atomicAdd(&a.zones[zcur], (unsigned long long)zcnt);
        hcur = zcur = -1;
        hcnt = zcnt = 0;
    }
    template <bool HIST, bool ZONES>
    __device__ __forceinline__ void add(const DepthArgs&, int l, float d, const DepthPos<ZONES>& p) {
        if (l < 1 || l > n || !(d >= 0.0f)) return;
        if (l != run.label) {
            if (run.label > 0) send(run.label, run.cnt, run.q, run.mn, run.mx, run.pz, run.py, run.px);
            run.reset(l);
        }
        run.add(d, p.z, p.y, p.x);
        if (HIST) {
            const long long h = (long long)(l - 1) * row + depth_bin(d, bpm, nbins);
            if (h != hcur) {
                if (hcur >= 0) atomicAdd(&a.hist[hcur], (unsigned long long)hcnt);
                hcur = h;
                hcnt = 0;
            }
            ++hcnt;
        }
        if (ZONES) {
            const long long zn = (long long)(l - 1) * nzt + p.zone(a);
            if (zn != zcur) {
                if (zcur >= 0) atomicAdd(&a.zones[zcur], (unsigned long long)zcnt);
                zcur = zn;
                zcnt = 0;
            }
            ++zcnt;
        }
    }
    // Called by all 64 lanes of a wave together.  Every round serves the lanes whose pending run carries the leader's label and
    // clears at least the leader's bit, so the loop ends after at most 64 rounds.
    __device__ __forceinline__ void end_lap() {
        const int lane = threadIdx.x & 63;
        unsigned long long todo = __ballot(run.label > 0);
        while (todo) {                                     // wave-uniform
            const int lead = __shfl(run.label, __ffsll((long long)todo) - 1, 64);
            const bool mine = run.label == lead;
            const unsigned long long m = __ballot(mine);
            if (__popcll(m) == 1) {
                if (mine) send(lead, run.cnt, run.q, run.mn, run.mx, run.pz, run.py, run.px);
            } else {
                unsigned c = mine ? run.cnt : 0u, mn = mine ? run.mn : DEPTH_INF_BITS, mx = mine ? run.mx : 0u;
                unsigned long long q = mine ? run.q : 0ull, pz = mine ? run.pz : 0ull, py = mine ? run.py : 0ull, px = mine ? run.px : 0ull;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    c += __shfl_xor(c, o, 64);
                    q += __shfl_xor(q, o, 64);
                    pz += __shfl_xor(pz, o, 64);
                    py += __shfl_xor(py, o, 64);
                    px += __shfl_xor(px, o, 64);
                    const unsigned tn = __shfl_xor(mn, o, 64), tx = __shfl_xor(mx, o, 64);
                    mn = tn < mn ? tn : mn;
                    mx = tx > mx ? tx : mx;
                }
                if (lane == __ffsll((long long)m) - 1) send(lead, c, q, mn, mx, pz, py, px);
            }
            todo &= ~m;
        }
        run.reset(0);
        flush_tables();
    }
    __device__ __forceinline__ void finish(const DepthArgs&) {}
};

template <class LabelT>
__device__ __forceinline__ bool depth_labels16(const LabelT* labels, long long g, int (&l)[16]);

// false: all 16 are zero
template <>
__device__ __forceinline__ bool depth_labels16<uint8_t>(const uint8_t* labels, long long g, int (&l)[16]) {
    const uint4 v = reinterpret_cast<const uint4*>(labels)[g];
    if ((v.x | v.y | v.z | v.w) == 0) return false;
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 16; ++k) l[k] = (int)((w[k >> 2] >> (8 * (k & 3))) & 0xffu);
    return true;
}

template <>
__device__ __forceinline__ bool depth_labels16<int32_t>(const int32_t* labels, long long g, int (&l)[16]) {
    int any = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int4 v = reinterpret_cast<const int4*>(labels)[g * 4 + j];
        l[4 * j] = v.x; l[4 * j + 1] = v.y; l[4 * j + 2] = v.z; l[4 * j + 3] = v.w;
        any |= v.x | v.y | v.z | v.w;
    }
    return any != 0;
}

// Both loops run a wave-uniform number of laps (the bound is tested on the wave's first index), so that end_lap is reached by
// all 64 lanes together.  Every index read lies below nvox: g < groups = nvox / 16 in the first loop, e < nvox in the second.
template <class Acc, class LabelT, bool HIST, bool ZONES>
__global__ __launch_bounds__(1024) void label_depth_kernel(const DepthArgs a) {
    Acc acc(a);
    const LabelT* labels = static_cast<const LabelT*>(a.labels);
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * blockDim.x, t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (long long base = t0 - lane; base < a.groups; base += stride) {
        const long long g = base + lane;
        int l[16];
        if (g < a.groups && depth_labels16<LabelT>(labels, g, l)) {
            bool some = true;
            if (a.mask) {
                const uint4 mv = reinterpret_cast<const uint4*>(a.mask)[g];
                const unsigned mw[4] = {mv.x, mv.y, mv.z, mv.w};
                some = (mv.x | mv.y | mv.z | mv.w) != 0;
#pragma unroll
                for (int k = 0; k < 16; ++k) l[k] = ((mw[k >> 2] >> (8 * (k & 3))) & 0xffu) ? l[k] : 0;
            }
            if (some) {
                float d[16];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float4 v = reinterpret_cast<const float4*>(a.depth)[g * 4 + j];
                    d[4 * j] = v.x; d[4 * j + 1] = v.y; d[4 * j + 2] = v.z; d[4 * j + 3] = v.w;
                }
                DepthPos<ZONES> p(a, (unsigned)(g * 16));
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    acc.template add<HIST, ZONES>(a, l[k], d[k], p);
                    if (k < 15) p.step(a);
                }
            }
        }
        acc.end_lap();
    }
    for (long long base = a.groups * 16 + t0 - lane; base < a.nvox; base += stride) {
        const long long e = base + lane;
        if (e < a.nvox) {
            const int l = (int)labels[e];
            if (l != 0 && (!a.mask || a.mask[e])) {
                const DepthPos<ZONES> p(a, (unsigned)e);
                acc.template add<HIST, ZONES>(a, l, a.depth[e], p);
            }
        }
        acc.end_lap();
    }
    acc.finish(a);
}

static inline bool depth_shape_ok(int label_kind, int n, int nbins, int nzones) {
    return (label_kind == 0 || label_kind == 1) && n >= 1 && !(label_kind == 0 && n > 255) && nbins >= 0 && nbins <= DEPTH_MAX_BINS &&
           nzones >= 0 && nzones <= DEPTH_MAX_AXIS_ZONES * DEPTH_MAX_AXIS_ZONES * DEPTH_MAX_AXIS_ZONES &&
           (int64_t)n * (nbins + 2) < (1LL << 31) && (int64_t)n * (nzones > 3 ? nzones : 3) < (1LL << 31);
}

static inline int64_t depth_table_words(int n, int nbins, int nzones) {
    return (int64_t)n * (DEPTH_MOM_WORDS + (nbins > 0 ? nbins + 2 : 0) + nzones);
}

static inline int depth_regime(int n, int nbins, int nzones) {
    return depth_table_words(n, nbins, nzones) <= DEPTH_LDS_WORDS ? DEPTH_LDS : DEPTH_WAVE;
}

static inline bool depth_bins_per_mm_ok(int b) { return b == 1 || b == 2 || b == 4 || b == 8 || b == 16; }

// The zone of index i along an axis with the box [a0, a1) and nz zones is ((clamp(i, a0, a1 - 1) - a0) * nz) / (a1 - a0), which
// is the number of j in 1 .. nz - 1 with clamp(i) - a0 >= ceil(j * (a1 - a0) / nz).  A threshold that the clamped index cannot
// reach (more zones than the box has voxels) is set out of reach, and the clamp is then no longer needed.
static inline void depth_thresholds(int a0, int a1, int nz, int (&t)[DEPTH_MAX_AXIS_ZONES - 1]) {
    const int64_t ext = (int64_t)a1 - a0;
    for (int j = 1; j < DEPTH_MAX_AXIS_ZONES; ++j) {
        const int64_t b = (int64_t)a0 + (j * ext + nz - 1) / nz;
        t[j - 1] = (j < nz && b <= (int64_t)a1 - 1) ? (int)b : DEPTH_NO_THRESHOLD;
    }
}

template <class Acc, class LabelT, bool HIST, bool ZONES>
static int depth_launch_one(const DepthArgs& a, unsigned grid, unsigned threads, size_t lds, hipStream_t st) {
    if (lds > 65536) {
        static LdsAttrOnce once;
        const int rc = ensure_dynamic_lds((const void*)label_depth_kernel<Acc, LabelT, HIST, ZONES>, lds, once, "label_depth");
        if (rc != DRAM_OK) return rc;
    }
    hipLaunchKernelGGL((label_depth_kernel<Acc, LabelT, HIST, ZONES>), dim3(grid), dim3(threads), lds, st, a);
    return DRAM_OK;
}

template <class Acc, class LabelT>
static int depth_launch(const DepthArgs& a, unsigned grid, unsigned threads, size_t lds, hipStream_t st) {
    if (a.hist) return a.zones ? depth_launch_one<Acc, LabelT, true, true>(a, grid, threads, lds, st)
                               : depth_launch_one<Acc, LabelT, true, false>(a, grid, threads, lds, st);
    return a.zones ? depth_launch_one<Acc, LabelT, false, true>(a, grid, threads, lds, st)
                   : depth_launch_one<Acc, LabelT, false, false>(a, grid, threads, lds, st);
}

}  // namespace dram

using namespace dram;

#define DEPTH_SHAPE_MSG "label_depth: label_kind 0 (uint8, n <= 255) or 1 (int32), n >= 1, nbins in 0..%d, nzones in 0..512, every table below 2^31 words"

extern "C" int dram_label_depth_plan(int label_kind, int n, int nbins, int nzones) {
    DRAM_REQUIRE(depth_shape_ok(label_kind, n, nbins, nzones), DEPTH_SHAPE_MSG, DEPTH_MAX_BINS);
    return depth_regime(n, nbins, nzones);
}

extern "C" int dram_label_depth(const float* depth, const void* labels, int label_kind, const uint8_t* mask, int n, int64_t* count,
                                int64_t* qsum, uint32_t* dmin, uint32_t* dmax, int64_t* possum, int64_t* hist, int bins_per_mm, int nbins,
                                int64_t* zones, const int32_t* box, int nz, int ny, int nx, int D, int H, int W, void* stream) {
    DRAM_REQUIRE(depth && labels && count && qsum && dmin && dmax && possum, "label_depth: null pointer");
    DRAM_REQUIRE(D >= 1 && H >= 1 && W >= 1 && (int64_t)D * H * W < (1LL << 31), "label_depth: D, H, W >= 1 and D * H * W < 2^31");
    DRAM_REQUIRE(nz >= 1 && nz <= DEPTH_MAX_AXIS_ZONES && ny >= 1 && ny <= DEPTH_MAX_AXIS_ZONES && nx >= 1 && nx <= DEPTH_MAX_AXIS_ZONES,
                 "label_depth: nz, ny, nx must each be in 1..%d", DEPTH_MAX_AXIS_ZONES);
    const int nzt = nz * ny * nx;
    DRAM_REQUIRE((zones == nullptr) == (nzt == 1 && box == nullptr),
                 "label_depth: zones and its box go together (zones NULL iff nz * ny * nx == 1 and box NULL)");
    DRAM_REQUIRE(depth_shape_ok(label_kind, n, nbins, zones ? nzt : 0), DEPTH_SHAPE_MSG, DEPTH_MAX_BINS);
    DRAM_REQUIRE((hist == nullptr) == (nbins == 0), "label_depth: hist and nbins go together (NULL iff 0)");
    DRAM_REQUIRE(nbins == 0 || depth_bins_per_mm_ok(bins_per_mm), "label_depth: bins_per_mm must be 1, 2, 4, 8 or 16");
    DRAM_REQUIRE(!box || (box[0] < box[1] && box[2] < box[3] && box[4] < box[5]), "label_depth: an empty box (a0 >= a1 on an axis)");
    DRAM_REQUIRE(((uintptr_t)depth & 3) == 0 && (label_kind == 0 || ((uintptr_t)labels & 3) == 0), "label_depth: misaligned depth or labels");
    hipStream_t st = (hipStream_t)stream;
    const int64_t nvox = (int64_t)D * H * W;
    const int64_t nhist = hist ? (int64_t)n * (nbins + 2) : 0, nzones = zones ? (int64_t)n * nzt : 0;
    int64_t total = 3LL * n;
    total = nhist > total ? nhist : total;
    total = nzones > total ? nzones : total;
    hipLaunchKernelGGL(depth_init_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, st, (unsigned long long*)count,
                       (unsigned long long*)qsum, dmin, dmax, (unsigned long long*)possum, (unsigned long long*)hist,
                       (unsigned long long*)zones, n, (long long)nhist, (long long)nzones);
    const bool vec = aligned16(depth) && aligned16(labels) && (!mask || aligned16(mask));
    DepthArgs a{};
    a.depth = depth; a.labels = labels; a.mask = mask;
    a.count = (unsigned long long*)count; a.qsum = (unsigned long long*)qsum; a.dmin = dmin; a.dmax = dmax;
    a.possum = (unsigned long long*)possum; a.hist = (unsigned long long*)hist; a.zones = (unsigned long long*)zones;
    a.n = n; a.nbins = nbins; a.nzt = nzt; a.bins_per_mm = (float)(nbins > 0 ? bins_per_mm : 1); a.ny = ny; a.nx = nx;
    const int32_t whole[6] = {0, D, 0, H, 0, W};           // zones without a box: the zones of the whole volume
    const int32_t* b = box ? box : whole;
    depth_thresholds(b[0], b[1], nz, a.tz);
    depth_thresholds(b[2], b[3], ny, a.ty);
    depth_thresholds(b[4], b[5], nx, a.tx);
    a.H = (unsigned)H; a.W = (unsigned)W; a.HW = (unsigned)((int64_t)H * W);
    a.nvox = nvox; a.groups = vec ? nvox / 16 : 0;
    const int64_t work = a.groups > 0 ? a.groups : nvox;
    const int nzw = zones ? nzt : 0;
    int rc;
    if (depth_regime(n, nbins, nzw) == DEPTH_LDS) {
        // 32-bit LDS counts: a block covers at most cdiv(2^31, grid * threads) laps of threads voxels (16 * threads voxels over
        // 2^27 groups), 2^23 voxels at the 256 blocks of 1024 threads and 2^20 at the 2048 blocks of 256
        const size_t lds = (size_t)depth_table_words(n, nbins, nzw) * 4;
        const bool big = lds > (size_t)DEPTH_BIG_BYTES;
        const unsigned threads = big ? 1024 : 256;
        const int64_t want = cdiv64(work, threads * 4), cap = big ? 256 : 2048;
        const unsigned grid = (unsigned)(want > cap ? cap : want);
        rc = label_kind == 0 ? depth_launch<DepthLdsAcc, uint8_t>(a, grid, threads, lds, st)
                             : depth_launch<DepthLdsAcc, int32_t>(a, grid, threads, lds, st);
    } else {
        const int64_t want = cdiv64(work, 256 * 4);
        const unsigned grid = (unsigned)(want > 4096 ? 4096 : want);
        rc = label_kind == 0 ? depth_launch<DepthWaveAcc, uint8_t>(a, grid, 256, 0, st)
                             : depth_launch<DepthWaveAcc, int32_t>(a, grid, 256, 0, st);
    }
    if (rc != DRAM_OK) return rc;
    return check_launch("label_depth");
}
