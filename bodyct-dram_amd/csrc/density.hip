// Lesion density report at inference (gfx950): per-label moments and histograms of an int16 scan in one pass, and the reduction
// of those histograms to percentiles and band counts.  Everything is integers: sums by integer atomics, min / max by integer
// atomics, so no result depends on the order in which they land (the same bits every run).
//
// dram_label_density serves two regimes, chosen by dram_label_density_plan from (label_kind, n, nbins) alone:
//   DENS_LDS   the whole table of the call -- n * (7 + nbins + 2) 32-bit words -- fits in DENS_LDS_WORDS of LDS (the lobe map:
//              5 labels with a 4096-bin histogram are 82 KiB).  One table per block, the pattern of lobe_burden_kernel
//              (components.hip): a thread keeps the moments of its current label in registers and goes to LDS when the label
//              changes; a histogram count is one 32-bit LDS atomic; at the end one 64-bit global atomic per occupied entry.
//   DENS_WAVE  the table does not fit (component labels, or many labels with a histogram).  A thread folds its 16 voxels into
//              the run of its current label; at the end of a lap the lanes of a wave that hold the same label are reduced
//              together (a ballot elects the leader, as in cc_stats_kernel) and the leader sends one set of global atomics: a
//              component costs one set per wave and 1024 voxels, not one per voxel.  A label change inside a thread's 16
//              voxels sends the finished run directly.  Histogram counts go to global memory, equal consecutive (label, bin)
//              pairs of a thread merged into one add.
// Both stream 16 voxels per thread with 16-byte loads where scan, labels and mask are 16-byte aligned, and fall back to one
// voxel per thread otherwise and for the last nvox % 16 voxels.
#include "common.h"

namespace dram {

constexpr int DENS_LDS = 0, DENS_WAVE = 1;
constexpr int DENS_MAX_BINS = 4096;
constexpr int DENS_MOM_WORDS = 7;            // per label in LDS: sum (2 words), sum of squares (2), count, min, max
constexpr int DENS_LDS_WORDS = 32768;        // 128 of the CU's 160 KiB
constexpr int DENS_BIG_BYTES = 16384;        // a table above this: 1024 threads and one block per CU instead of 256 and eight

struct DensArgs {
    const int16_t* scan;
    const void* labels;
    const uint8_t* mask;
    unsigned long long *count, *sum, *sumsq;
    int *vmin, *vmax;
    unsigned long long* hist;
    int n, lo, nbins;
    unsigned width;
    long long nvox, groups;                  // groups of 16 voxels taken with 16-byte loads; the rest goes voxel by voxel
};

__global__ __launch_bounds__(256) void dens_init_kernel(unsigned long long* __restrict__ count, unsigned long long* __restrict__ sum,
                                                        unsigned long long* __restrict__ sumsq, int* __restrict__ vmin,
                                                        int* __restrict__ vmax, unsigned long long* __restrict__ hist, int n, int total) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) { count[i] = 0; sum[i] = 0; sumsq[i] = 0; vmin[i] = 32767; vmax[i] = -32768; }
    if (hist && i < total) hist[i] = 0;
}

// entry 0: below lo; 1 + (hu - lo) / width inside; nbins + 1: at or above lo + nbins * width.  The below-range test comes first,
// so the dividend is never negative; as unsigned the difference is exact whatever lo is.
__device__ __forceinline__ int dens_bin(int hu, int lo, unsigned width, int nbins) {
    if (hu < lo) return 0;
    const unsigned d = (unsigned)hu - (unsigned)lo;
    const unsigned b = width == 1u ? d : d / width;
    return b < (unsigned)nbins ? 1 + (int)b : nbins + 1;
}

// The moments of the voxels of one label that a thread has seen since the label last changed.
struct DensRun {
    int label;                               // 0: nothing pending
    unsigned cnt;
    long long sum;
    unsigned long long sq;
    int mn, mx;
    __device__ __forceinline__ void reset(int l) { label = l; cnt = 0; sum = 0; sq = 0; mn = 32767; mx = -32768; }
    __device__ __forceinline__ void add(int hu) {
        ++cnt;
        sum += hu;
        sq += (unsigned)(hu * hu);           // at most 2^30
        mn = hu < mn ? hu : mn;
        mx = hu > mx ? hu : mx;
    }
};

extern __shared__ unsigned long long dens_lds[];

// DENS_LDS: the block's table {sum[n], sumsq[n] (64-bit), count[n], min[n], max[n], hist[n][nbins + 2] (32-bit)}.  A block covers
// at most 2^23 voxels (see the launch), so the 32-bit counts cannot wrap.
struct DensLdsAcc {
    unsigned long long *lsum, *lsq;
    unsigned* lcnt;
    int *lmn, *lmx;
    unsigned* lhist;
    int n, lo, nbins, row;
    unsigned width;
    DensRun run;
    __device__ __forceinline__ DensLdsAcc(const DensArgs& a) : n(a.n), lo(a.lo), nbins(a.nbins), row(a.nbins + 2), width(a.width) {
        lsum = dens_lds;
        lsq = lsum + n;
        lcnt = reinterpret_cast<unsigned*>(lsq + n);
        lmn = reinterpret_cast<int*>(lcnt + n);
        lmx = lmn + n;
        lhist = reinterpret_cast<unsigned*>(lmx + n);
        const int words = n * (DENS_MOM_WORDS + (a.hist ? row : 0));
        unsigned* w = reinterpret_cast<unsigned*>(dens_lds);
        for (int k = threadIdx.x; k < words; k += blockDim.x) w[k] = 0;
        __syncthreads();
        for (int k = threadIdx.x; k < n; k += blockDim.x) { lmn[k] = 32767; lmx[k] = -32768; }
        __syncthreads();
        run.reset(0);
    }
    __device__ __forceinline__ void flush() {
        if (run.label > 0) {
            const int k = run.label - 1;
            atomicAdd(&lcnt[k], run.cnt);
            atomicAdd(&lsum[k], (unsigned long long)run.sum);
            atomicAdd(&lsq[k], run.sq);
            atomicMin(&lmn[k], run.mn);
            atomicMax(&lmx[k], run.mx);
        }
    }
    template <bool HIST>
    __device__ __forceinline__ void add(int l, int hu) {
        if (l < 1 || l > n) return;
        if (l != run.label) { flush(); run.reset(l); }
        run.add(hu);
        if (HIST) atomicAdd(&lhist[(l - 1) * row + dens_bin(hu, lo, width, nbins)], 1u);
    }
    __device__ __forceinline__ void end_lap() {}
    __device__ __forceinline__ void finish(const DensArgs& a) {
        flush();
        __syncthreads();
        for (int k = threadIdx.x; k < n; k += blockDim.x) {
            const unsigned c = lcnt[k];
            if (c) {
                atomicAdd(&a.count[k], (unsigned long long)c);
                if (lsum[k]) atomicAdd(&a.sum[k], lsum[k]);
                atomicAdd(&a.sumsq[k], lsq[k]);
                atomicMin(&a.vmin[k], lmn[k]);
                atomicMax(&a.vmax[k], lmx[k]);
            }
        }
        if (a.hist) {
            for (int e = threadIdx.x; e < n * row; e += blockDim.x) {
                const unsigned c = lhist[e];
                if (c) atomicAdd(&a.hist[e], (unsigned long long)c);
            }
        }
    }
};

// DENS_WAVE: runs in registers, one set of global atomics per label and wave at the end of a lap.
struct DensWaveAcc {
    const DensArgs& a;
    int n, lo, nbins, row;
    unsigned width;
    DensRun run;
    int hcur;                                // pending histogram entry, -1: none
    unsigned hcnt;
    __device__ __forceinline__ DensWaveAcc(const DensArgs& a_) : a(a_), n(a_.n), lo(a_.lo), nbins(a_.nbins), row(a_.nbins + 2), width(a_.width) {
        run.reset(0);
        hcur = -1;
        hcnt = 0;
    }
    __device__ __forceinline__ void send(int label, unsigned cnt, long long sum, unsigned long long sq, int mn, int mx) {
        const int k = label - 1;
        atomicAdd(&a.count[k], (unsigned long long)cnt);
        if (sum) atomicAdd(&a.sum[k], (unsigned long long)sum);
        atomicAdd(&a.sumsq[k], sq);
        atomicMin(&a.vmin[k], mn);
        atomicMax(&a.vmax[k], mx);
    }
    __device__ __forceinline__ void flush_hist() {
        if (hcur >= 0) atomicAdd(&a.hist[hcur], (unsigned long long)hcnt);
        hcur = -1;
        hcnt = 0;
    }
    template <bool HIST>
    __device__ __forceinline__ void add(int l, int hu) {
        if (l < 1 || l > n) return;
        if (l != run.label) {
            if (run.label > 0) send(run.label, run.cnt, run.sum, run.sq, run.mn, run.mx);
            run.reset(l);
        }
        run.add(hu);
        if (HIST) {
            const int h = (l - 1) * row + dens_bin(hu, lo, width, nbins);
            if (h != hcur) { flush_hist(); hcur = h; }
            ++hcnt;
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
                if (mine) send(lead, run.cnt, run.sum, run.sq, run.mn, run.mx);
            } else {
                unsigned c = mine ? run.cnt : 0u;
                long long s = mine ? run.sum : 0;
                unsigned long long q = mine ? run.sq : 0ull;
                int mn = mine ? run.mn : 32767, mx = mine ? run.mx : -32768;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    c += __shfl_xor(c, o, 64);
                    s += __shfl_xor(s, o, 64);
                    q += __shfl_xor(q, o, 64);
                    const int tn = __shfl_xor(mn, o, 64), tx = __shfl_xor(mx, o, 64);
                    mn = tn < mn ? tn : mn;
                    mx = tx > mx ? tx : mx;
                }
                if (lane == __ffsll((long long)m) - 1) send(lead, c, s, q, mn, mx);
            }
            todo &= ~m;
        }
        run.reset(0);
        flush_hist();
    }
    __device__ __forceinline__ void finish(const DensArgs&) {}
};

template <class LabelT>
__device__ __forceinline__ bool dens_labels16(const LabelT* labels, long long g, int (&l)[16]);

// false: all 16 are zero
template <>
__device__ __forceinline__ bool dens_labels16<uint8_t>(const uint8_t* labels, long long g, int (&l)[16]) {
    const uint4 v = reinterpret_cast<const uint4*>(labels)[g];
    if ((v.x | v.y | v.z | v.w) == 0) return false;
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 16; ++k) l[k] = (int)((w[k >> 2] >> (8 * (k & 3))) & 0xffu);
    return true;
}

template <>
__device__ __forceinline__ bool dens_labels16<int32_t>(const int32_t* labels, long long g, int (&l)[16]) {
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
// all 64 lanes together.
template <class Acc, class LabelT, bool HIST>
__global__ __launch_bounds__(1024) void label_density_kernel(const DensArgs a) {
    Acc acc(a);
    const LabelT* labels = static_cast<const LabelT*>(a.labels);
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * blockDim.x, t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (long long base = t0 - lane; base < a.groups; base += stride) {
        const long long g = base + lane;
        int l[16];
        if (g < a.groups && dens_labels16<LabelT>(labels, g, l)) {
            bool some = true;
            if (a.mask) {
                const uint4 mv = reinterpret_cast<const uint4*>(a.mask)[g];
                const unsigned mw[4] = {mv.x, mv.y, mv.z, mv.w};
                some = (mv.x | mv.y | mv.z | mv.w) != 0;
#pragma unroll
                for (int k = 0; k < 16; ++k) l[k] = ((mw[k >> 2] >> (8 * (k & 3))) & 0xffu) ? l[k] : 0;
            }
            if (some) {
                const uint4 s0 = reinterpret_cast<const uint4*>(a.scan)[g * 2], s1 = reinterpret_cast<const uint4*>(a.scan)[g * 2 + 1];
                const unsigned sw[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
#pragma unroll
                for (int k = 0; k < 16; ++k) acc.template add<HIST>(l[k], (int)(int16_t)((sw[k >> 1] >> (16 * (k & 1))) & 0xffffu));
            }
        }
        acc.end_lap();
    }
    for (long long base = a.groups * 16 + t0 - lane; base < a.nvox; base += stride) {
        const long long e = base + lane;
        if (e < a.nvox) {
            const int l = (int)labels[e];
            if (l != 0 && (!a.mask || a.mask[e])) acc.template add<HIST>(l, (int)a.scan[e]);
        }
        acc.end_lap();
    }
    acc.finish(a);
}

static inline bool dens_shape_ok(int label_kind, int n, int nbins) {
    return (label_kind == 0 || label_kind == 1) && n >= 1 && !(label_kind == 0 && n > 255) && nbins >= 0 && nbins <= DENS_MAX_BINS &&
           (int64_t)n * (nbins + 2) < (1LL << 31);
}

static inline int dens_regime(int n, int nbins) {
    return (int64_t)n * (DENS_MOM_WORDS + (nbins > 0 ? nbins + 2 : 0)) <= DENS_LDS_WORDS ? DENS_LDS : DENS_WAVE;
}

static inline bool dens_range_ok(int lo, int width, int nbins) {
    if (nbins > 0 && width < 1) return false;
    const int64_t top = (int64_t)lo + (int64_t)nbins * (nbins > 0 ? width : 0);
    return top <= INT32_MAX;
}

template <class Acc, class LabelT>
static int dens_launch(const DensArgs& a, unsigned grid, unsigned threads, size_t lds, hipStream_t st, const char* who) {
    if (a.hist) {
        if (lds > 65536) {
            static LdsAttrOnce once;
            const int rc = ensure_dynamic_lds((const void*)label_density_kernel<Acc, LabelT, true>, lds, once, who);
            if (rc != DRAM_OK) return rc;
        }
        hipLaunchKernelGGL((label_density_kernel<Acc, LabelT, true>), dim3(grid), dim3(threads), lds, st, a);
    } else {
        if (lds > 65536) {
            static LdsAttrOnce once;
            const int rc = ensure_dynamic_lds((const void*)label_density_kernel<Acc, LabelT, false>, lds, once, who);
            if (rc != DRAM_OK) return rc;
        }
        hipLaunchKernelGGL((label_density_kernel<Acc, LabelT, false>), dim3(grid), dim3(threads), lds, st, a);
    }
    return DRAM_OK;
}

// ---- histogram rows -> percentiles and band counts
struct HistSummaryArgs {
    int q[16];
    int edge_bin[15];                        // an edge lo + j * width as the first in-range bin j + 1 of the band above it
    int nq, ne, lo, width, nbins;
};

// One block per row.  A thread owns a contiguous piece of the row: the pieces are summed, the sums scanned over the block
// (exclusive, int64: exact), and every thread then walks its piece with the running count.  The entry at which the running count
// first reaches a rank is unique (it is non-empty), so exactly one thread writes each percentile.
__global__ __launch_bounds__(256) void hist_summary_kernel(const long long* __restrict__ hist, const HistSummaryArgs s,
                                                           int* __restrict__ pct, long long* __restrict__ bands) {
    __shared__ long long wsum[4];
    __shared__ unsigned long long bsum[16];
    const int row = s.nbins + 2, per = (row + 255) / 256;
    const long long* h = hist + (size_t)blockIdx.x * row;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int e0 = threadIdx.x * per, e1 = e0 + per < row ? e0 + per : row;
    if (threadIdx.x < 16) bsum[threadIdx.x] = 0;
    long long mine = 0;
    for (int e = e0; e < e1; ++e) mine += h[e];
    long long sc = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long t = __shfl_up(sc, o, 64);
        if (lane >= o) sc += t;
    }
    if (lane == 63) wsum[w] = sc;
    __syncthreads();
    long long before = sc - mine, total = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < w) before += wsum[k];
        total += wsum[k];
    }
    if (total == 0 && threadIdx.x < s.nq) pct[(size_t)blockIdx.x * s.nq + threadIdx.x] = INT32_MAX;
    int band = 0;
    long long run = before, in_band = 0;
    for (int e = e0; e < e1; ++e) {
        const long long c = h[e];
        if (c == 0) continue;
        // band of the entry: the edges at or below its lower edge; the underflow entry is in band 0, the overflow entry in ne
        int b = 0;
        if (e == row - 1) b = s.ne;
        else if (e >= 1)
            for (int i = 0; i < s.ne; ++i) b += s.edge_bin[i] <= e;
        if (b != band) {
            if (in_band) atomicAdd(&bsum[band], (unsigned long long)in_band);
            band = b;
            in_band = 0;
        }
        in_band += c;
        for (int i = 0; i < s.nq; ++i) {
            long long rank = ((long long)s.q[i] * total + 999) / 1000;
            rank = rank < 1 ? 1 : rank;
            if (run < rank && rank <= run + c)
                pct[(size_t)blockIdx.x * s.nq + i] = e == 0 ? INT32_MIN : (e == row - 1 ? INT32_MAX : s.lo + (e - 1) * s.width);
        }
        run += c;
    }
    if (in_band) atomicAdd(&bsum[band], (unsigned long long)in_band);
    __syncthreads();
    if (threadIdx.x <= s.ne && bands) bands[(size_t)blockIdx.x * (s.ne + 1) + threadIdx.x] = (long long)bsum[threadIdx.x];
}

}  // namespace dram

using namespace dram;

extern "C" int dram_label_density_plan(int label_kind, int n, int nbins) {
    DRAM_REQUIRE(dens_shape_ok(label_kind, n, nbins),
                 "label_density: label_kind 0 (uint8, n <= 255) or 1 (int32), n >= 1, nbins in 0..%d, n * (nbins + 2) < 2^31", DENS_MAX_BINS);
    return dens_regime(n, nbins);
}

extern "C" int dram_label_density(const int16_t* scan, const void* labels, int label_kind, const uint8_t* mask, int n, int64_t* count,
                                  int64_t* sum, int64_t* sumsq, int32_t* vmin, int32_t* vmax, int64_t* hist, int lo, int width,
                                  int nbins, int64_t nvox, void* stream) {
    DRAM_REQUIRE(scan && labels && count && sum && sumsq && vmin && vmax, "label_density: null pointer");
    DRAM_REQUIRE(nvox > 0 && nvox < (1LL << 31), "label_density: nvox must be in 1 .. 2^31 - 1");
    DRAM_REQUIRE(dens_shape_ok(label_kind, n, nbins),
                 "label_density: label_kind 0 (uint8, n <= 255) or 1 (int32), n >= 1, nbins in 0..%d, n * (nbins + 2) < 2^31", DENS_MAX_BINS);
    DRAM_REQUIRE((hist == nullptr) == (nbins == 0), "label_density: hist and nbins go together (NULL iff 0)");
    DRAM_REQUIRE(dens_range_ok(lo, width, nbins), "label_density: width >= 1 and lo + nbins * width within int32");
    DRAM_REQUIRE(((uintptr_t)scan & 1) == 0 && (label_kind == 0 || ((uintptr_t)labels & 3) == 0), "label_density: misaligned scan or labels");
    hipStream_t st = (hipStream_t)stream;
    const int total = n * (nbins + 2);
    hipLaunchKernelGGL(dens_init_kernel, dim3((unsigned)cdiv64(hist ? total : n, 256)), dim3(256), 0, st, (unsigned long long*)count,
                       (unsigned long long*)sum, (unsigned long long*)sumsq, vmin, vmax, (unsigned long long*)hist, n, total);
    const bool vec = aligned16(scan) && aligned16(labels) && (!mask || aligned16(mask));
    DensArgs a{scan, labels, mask, (unsigned long long*)count, (unsigned long long*)sum, (unsigned long long*)sumsq, vmin, vmax,
               (unsigned long long*)hist, n, lo, nbins, (unsigned)(nbins > 0 ? width : 1), (long long)nvox, vec ? nvox / 16 : 0};
    const int64_t work = a.groups > 0 ? a.groups : nvox;
    int rc;
    if (dens_regime(n, nbins) == DENS_LDS) {
        // 32-bit LDS counts: a block covers at most cdiv(2^31, grid * threads) laps of threads voxels (16 * threads voxels over
        // 2^27 groups), 2^23 voxels at the 256 blocks of 1024 threads and 2^20 at the 2048 blocks of 256
        const size_t lds = (size_t)n * (DENS_MOM_WORDS + (nbins > 0 ? nbins + 2 : 0)) * 4;
        const bool big = lds > (size_t)DENS_BIG_BYTES;
        const unsigned threads = big ? 1024 : 256;
        const int64_t want = cdiv64(work, threads * 4), cap = big ? 256 : 2048;
        const unsigned grid = (unsigned)(want > cap ? cap : want);
        rc = label_kind == 0 ? dens_launch<DensLdsAcc, uint8_t>(a, grid, threads, lds, st, "label_density")
                             : dens_launch<DensLdsAcc, int32_t>(a, grid, threads, lds, st, "label_density");
    } else {
        const int64_t want = cdiv64(work, 256 * 4);
        const unsigned grid = (unsigned)(want > 4096 ? 4096 : want);
        rc = label_kind == 0 ? dens_launch<DensWaveAcc, uint8_t>(a, grid, 256, 0, st, "label_density")
                             : dens_launch<DensWaveAcc, int32_t>(a, grid, 256, 0, st, "label_density");
    }
    if (rc != DRAM_OK) return rc;
    return check_launch("label_density");
}

extern "C" int dram_hist_summary(const int64_t* hist, int n, int lo, int width, int nbins, const int32_t* q_permille, int nq,
                                 const int32_t* edges, int ne, int32_t* pct, int64_t* bands, void* stream) {
    DRAM_REQUIRE(hist, "hist_summary: null pointer");
    DRAM_REQUIRE(n >= 1 && nbins >= 0 && nbins <= DENS_MAX_BINS && (int64_t)n * (nbins + 2) < (1LL << 31),
                 "hist_summary: n >= 1, nbins in 0..%d, n * (nbins + 2) < 2^31", DENS_MAX_BINS);
    DRAM_REQUIRE(dens_range_ok(lo, width, nbins), "hist_summary: width >= 1 and lo + nbins * width within int32");
    DRAM_REQUIRE(nq >= 0 && nq <= 16 && ne >= 0 && ne <= 15, "hist_summary: nq in 0..16, ne in 0..15");
    DRAM_REQUIRE((nq == 0 || (q_permille && pct)) && (ne == 0 || (edges && bands)), "hist_summary: null pointer");
    HistSummaryArgs s{};
    s.nq = nq; s.ne = ne; s.lo = lo; s.width = nbins > 0 ? width : 1; s.nbins = nbins;
    for (int i = 0; i < nq; ++i) {
        DRAM_REQUIRE(q_permille[i] >= 0 && q_permille[i] <= 1000, "hist_summary: percentiles are per mille, 0..1000");
        s.q[i] = q_permille[i];
    }
    for (int i = 0; i < ne; ++i) {
        const int64_t d = (int64_t)edges[i] - lo;
        DRAM_REQUIRE(d >= 0 && d % s.width == 0 && d / s.width <= nbins, "hist_summary: an edge must be lo + j * width, 0 <= j <= nbins");
        DRAM_REQUIRE(i == 0 || edges[i] > edges[i - 1], "hist_summary: edges must ascend strictly");
        s.edge_bin[i] = (int)(d / s.width) + 1;
    }
    if (nq == 0 && !bands) return DRAM_OK;
    hipLaunchKernelGGL(hist_summary_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, (const long long*)hist, s, pct, (long long*)bands);
    return check_launch("hist_summary");
}
