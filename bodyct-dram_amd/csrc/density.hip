// Lesion density report at inference (gfx950): per-label moments and histograms of an int16 scan in one pass, and the reduction
// of those histograms to percentiles and band counts.  Everything is integers, so no result depends on the order in which the
// atomics land (the same bits every run).
//
// dram_label_density is a streaming report of label_stream.h, which describes its two regimes; dram_label_density_plan chooses
// between them from (label_kind, n, nbins) alone: the table of a call is n * (7 + nbins + 2) 32-bit words.
#include "label_stream.h"

namespace dram {

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

// Per label: count, minimum and maximum HU, the sums {HU (two's complement), HU^2}, and one count table, the histogram.
struct DensPolicy {
    using Args = DensArgs;
    using Value = int;
    static constexpr int SUMS = 2, TABLES = 1, MIN0 = 32767, MAX0 = -32768;
    __device__ __forceinline__ static int row(const DensArgs& a, int) { return a.hist ? a.nbins + 2 : 0; }
    __device__ __forceinline__ static unsigned long long* table(const DensArgs& a, int) { return a.hist; }
    template <class Moments>
    __device__ __forceinline__ static void send(const DensArgs& a, int label, const Moments& m) {
        const int k = label - 1;
        atomicAdd(&a.count[k], (unsigned long long)m.cnt);
        if (m.s[0]) atomicAdd(&a.sum[k], m.s[0]);
        atomicAdd(&a.sumsq[k], m.s[1]);
        atomicMin(&a.vmin[k], m.mn);
        atomicMax(&a.vmax[k], m.mx);
    }
};

template <class Acc, class LabelT, bool HIST>
__global__ __launch_bounds__(1024) void label_density_kernel(const DensArgs a) {
    Acc acc(a);
    const auto add = [&](int l, int hu) {
        if (!acc.enter(l)) return;
        acc.m.see(hu);
        acc.m.s[0] += (unsigned long long)(long long)hu;
        acc.m.s[1] += (unsigned)(hu * hu);   // at most 2^30
        if (HIST) acc.count(0, (l - 1) * (a.nbins + 2) + dens_bin(hu, a.lo, a.width, a.nbins));
    };
    stream_labels<LabelT>(
        a.labels, a.mask, a.groups, a.nvox, acc,
        [&](long long g, const int (&l)[16]) {
            const uint4 s0 = reinterpret_cast<const uint4*>(a.scan)[g * 2], s1 = reinterpret_cast<const uint4*>(a.scan)[g * 2 + 1];
            const unsigned sw[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
#pragma unroll
            for (int k = 0; k < 16; ++k) add(l[k], (int)(int16_t)((sw[k >> 1] >> (16 * (k & 1))) & 0xffffu));
        },
        [&](long long e, int l) { add(l, (int)a.scan[e]); });
}

static inline bool dens_shape_ok(int label_kind, int n, int nbins) { return label_kind_ok(label_kind, n) && hist_shape_ok(n, nbins); }

static inline int64_t dens_table_words(int n, int nbins) {
    return (int64_t)n * (label_moment_words<DensPolicy>() + (nbins > 0 ? nbins + 2 : 0));
}

static inline bool dens_range_ok(int lo, int width, int nbins) {
    if (nbins > 0 && width < 1) return false;
    const int64_t top = (int64_t)lo + (int64_t)nbins * (nbins > 0 ? width : 0);
    return top <= INT32_MAX;
}

template <class Acc>
static int dens_launch(const DensArgs& a, int label_kind, const StreamLaunch& g, hipStream_t st) {
    const char* who = "label_density";
    if (label_kind == 0)
        return a.hist ? launch_stream<label_density_kernel<Acc, uint8_t, true>>(a, g, st, who)
                      : launch_stream<label_density_kernel<Acc, uint8_t, false>>(a, g, st, who);
    return a.hist ? launch_stream<label_density_kernel<Acc, int32_t, true>>(a, g, st, who)
                  : launch_stream<label_density_kernel<Acc, int32_t, false>>(a, g, st, who);
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
                 "label_density: label_kind 0 (uint8, n <= 255) or 1 (int32), n >= 1, nbins in 0..%d, n * (nbins + 2) < 2^31", LABEL_MAX_BINS);
    return label_regime(dens_table_words(n, nbins));
}

extern "C" int dram_label_density(const int16_t* scan, const void* labels, int label_kind, const uint8_t* mask, int n, int64_t* count,
                                  int64_t* sum, int64_t* sumsq, int32_t* vmin, int32_t* vmax, int64_t* hist, int lo, int width,
                                  int nbins, int64_t nvox, void* stream) {
    DRAM_REQUIRE(scan && labels && count && sum && sumsq && vmin && vmax, "label_density: null pointer");
    DRAM_REQUIRE(nvox > 0 && nvox < (1LL << 31), "label_density: nvox must be in 1 .. 2^31 - 1");
    DRAM_REQUIRE(dens_shape_ok(label_kind, n, nbins),
                 "label_density: label_kind 0 (uint8, n <= 255) or 1 (int32), n >= 1, nbins in 0..%d, n * (nbins + 2) < 2^31", LABEL_MAX_BINS);
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
    const int64_t words = dens_table_words(n, nbins);
    const StreamLaunch g = stream_geometry(words, nvox, a.groups, 4096);
    const int rc = label_regime(words) == LABEL_LDS ? dens_launch<LdsLabelAcc<DensPolicy>>(a, label_kind, g, st)
                                                    : dens_launch<WaveLabelAcc<DensPolicy>>(a, label_kind, g, st);
    if (rc != DRAM_OK) return rc;
    return check_launch("label_density");
}

extern "C" int dram_hist_summary(const int64_t* hist, int n, int lo, int width, int nbins, const int32_t* q_permille, int nq,
                                 const int32_t* edges, int ne, int32_t* pct, int64_t* bands, void* stream) {
    DRAM_REQUIRE(hist, "hist_summary: null pointer");
    DRAM_REQUIRE(n >= 1 && hist_shape_ok(n, nbins),
                 "hist_summary: n >= 1, nbins in 0..%d, n * (nbins + 2) < 2^31", LABEL_MAX_BINS);
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
