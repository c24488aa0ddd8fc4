// Heat-map evaluation curves at inference (gfx950): the joint histogram of score bin x class x region in one pass over the fp32
// heat map, the reference mask and the lobe map, with an optional gate and an optional fixed-point sum of the scores per entry
// (for calibration).  ROC, precision / recall, the Dice sweep and the calibration table are host arithmetic on that table
// (dram_amd/curves.py).  Everything is integers, accumulated by integer atomics and integer reductions: the same bits every run.
//
// dram_score_hist serves two regimes, chosen by dram_score_hist_plan from (nregions, nbins, with_conf) alone:
//   CURVES_LDS     the table of the call -- nregions * 2 * (nbins + 1) entries of one 32-bit count and, with conf, one 64-bit sum --
//                  fits in LABEL_LDS_WORDS of LDS (5 lobes at 1024 bins with conf are 120 KiB).  One table per block; at the end
//                  one 64-bit global atomic per occupied entry.
//   CURVES_GLOBAL  it does not fit (5 lobes at 4096 bins): the same aggregated updates go to global memory as 64-bit atomics.
// What keeps either from serialising on the few low-score bins that hold almost every lung voxel is done before the atomic, in two
// steps.  A thread keeps the run of its current key (entry index) in registers -- count and sum -- across its 16 voxels AND across
// its laps, and sends it only when the key changes: on a map that sits in one bin a thread sends one update per call.  When
// lanes of a wave do send at the same voxel position, the lanes that hold the leader's key are summed by shuffles and the leader
// sends one update (up to CURVES_PEEL keys, each only if at least CURVES_GROUP lanes share it: a shuffle reduction costs about
// as much as a handful of colliding lanes, so smaller groups go to the atomic unit as they are).  That is enough for
// CURVES_LDS, which runs at the same speed on a peaked map as on a uniform one; CURVES_GLOBAL still sends about one global
// atomic per lung voxel where neighbouring voxels differ by a bin and is several times slower there (DESIGN.md has the figures).
// 16 voxels per thread with 16-byte loads where score, ref, region and gate are 16-byte aligned; one voxel per thread otherwise
// and for the last nvox % 16 voxels.  A group of 16 whose region bytes are all zero (outside the lungs: most of a scan) costs
// its 16 region bytes and nothing else.
#include "label_stream.h"

namespace dram {

constexpr int CURVES_LDS = 0, CURVES_GLOBAL = 1;
static_assert(CURVES_LDS == LABEL_LDS && CURVES_GLOBAL == LABEL_WAVE, "label_regime and stream_geometry (label_stream.h) decide between them");
constexpr int CURVES_MAX_BINS = 4096;
constexpr int CURVES_PEEL = 2;               // keys per send that are looked at for a wave-wide sum
constexpr int CURVES_GROUP = 8;              // lanes that must share a key for the sum to pay

struct CurveArgs {
    const float* score;
    const uint8_t *ref, *region, *gate;
    unsigned long long *hist, *conf;
    int nregions, nbins, row;                // row = nbins + 1
    float fbins;
    long long nvox, groups;                  // groups of 16 voxels taken with 16-byte loads; the rest goes voxel by voxel
};

__global__ __launch_bounds__(256) void curves_init_kernel(unsigned long long* __restrict__ hist, unsigned long long* __restrict__ conf,
                                                          int total) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < total) {
        hist[i] = 0;
        if (conf) conf[i] = 0;
    }
}

// bin 0: gate off, or a score that is not >= 0 (NaN, negative; -0.0f passes); bin nbins: score >= 1 (+inf too); else
// 1 + floor(score * nbins), the product exact because nbins is a power of two.
__device__ __forceinline__ int curves_bin(float s, bool gate_on, int nbins, float fbins) {
    if (!gate_on || !(s >= 0.0f)) return 0;
    if (s >= 1.0f) return nbins;
    return 1 + (int)(s * fbins);
}

// the fixed-point confidence of a voxel of bin >= 1: exact product, truncated, at most 2^24
__device__ __forceinline__ unsigned curves_q(float s) { return (unsigned)(fminf(s, 1.0f) * 16777216.0f); }

extern __shared__ unsigned long long curves_lds[];

// CURVES_LDS: the block's table {conf[E] (64-bit, only with conf), count[E] (32-bit)}.
template <bool CONF>
struct CurveLdsTable {
    unsigned long long* lconf;
    unsigned* lcnt;
    int entries;
    __device__ __forceinline__ CurveLdsTable(const CurveArgs& a) : entries(a.nregions * 2 * a.row) {
        lconf = curves_lds;
        lcnt = reinterpret_cast<unsigned*>(curves_lds + (CONF ? entries : 0));
        const int words = entries * (CONF ? 3 : 1);
        unsigned* w = reinterpret_cast<unsigned*>(curves_lds);
        for (int k = threadIdx.x; k < words; k += blockDim.x) w[k] = 0;
        __syncthreads();
    }
    __device__ __forceinline__ void add(int key, unsigned cnt, unsigned long long conf) {
        atomicAdd(&lcnt[key], cnt);
        if (CONF && conf) atomicAdd(&lconf[key], conf);
    }
    __device__ __forceinline__ void finish(const CurveArgs& a) {
        __syncthreads();
        for (int e = threadIdx.x; e < entries; e += blockDim.x) {
            const unsigned c = lcnt[e];
            if (c) {
                atomicAdd(&a.hist[e], (unsigned long long)c);
                if (CONF && lconf[e]) atomicAdd(&a.conf[e], lconf[e]);
            }
        }
    }
};

// CURVES_GLOBAL: the same updates as 64-bit global atomics.
template <bool CONF>
struct CurveGlobalTable {
    unsigned long long *hist, *gconf;
    __device__ __forceinline__ CurveGlobalTable(const CurveArgs& a) : hist(a.hist), gconf(a.conf) {}
    __device__ __forceinline__ void add(int key, unsigned cnt, unsigned long long conf) {
        atomicAdd(&hist[key], (unsigned long long)cnt);
        if (CONF && conf) atomicAdd(&gconf[key], conf);
    }
    __device__ __forceinline__ void finish(const CurveArgs&) {}
};

// The voxels of one key that a thread has seen since its key last changed.
struct CurveRun {
    int key;                                 // -1: nothing pending
    unsigned cnt;
    unsigned long long conf;
};

// Called by all 64 lanes of a wave together; the lanes with `send` hold a finished run.  Up to CURVES_PEEL times the lanes that
// hold the key of the first sending lane are summed and that lane sends the sum, as long as such a group has at least
// CURVES_GROUP lanes; whoever is left sends its own run.
template <bool CONF, class Table>
__device__ __forceinline__ void curves_wave_send(Table& t, bool send, const CurveRun& run) {
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(send);
#pragma unroll
    for (int round = 0; round < CURVES_PEEL; ++round) {
        if (!todo) break;                                              // wave-uniform
        const int first = __ffsll((long long)todo) - 1;
        const int lead = __shfl(run.key, first, 64);
        const bool mine = send && run.key == lead;
        const unsigned long long m = __ballot(mine);
        if (__popcll(m) < CURVES_GROUP) break;                         // wave-uniform
        unsigned c = mine ? run.cnt : 0u;
        unsigned long long q = (CONF && mine) ? run.conf : 0ull;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            c += __shfl_xor(c, o, 64);
            if (CONF) q += __shfl_xor(q, o, 64);
        }
        if (lane == first) t.add(lead, c, q);
        send = send && !mine;
        todo &= ~m;
    }
    if (send) t.add(run.key, run.cnt, run.conf);
}

// One voxel position of every lane of the wave: `valid` lanes hold a voxel of entry `key` with confidence q.
template <bool CONF, class Table>
__device__ __forceinline__ void curves_step(Table& t, CurveRun& run, bool valid, int key, unsigned q) {
    const bool change = valid && key != run.key;
    const bool send = change && run.cnt > 0;
    if (__any(send)) curves_wave_send<CONF>(t, send, run);             // wave-uniform
    if (change) { run.key = key; run.cnt = 0; run.conf = 0; }
    if (valid) {
        ++run.cnt;
        if (CONF) run.conf += q;
    }
}

// The lap bounds of both loops are wave-uniform, as those of stream_labels (label_stream.h) are, and every cross-lane step sits
// under wave-uniform conditions only.
template <class Table, bool CONF>
__global__ __launch_bounds__(1024) void score_hist_kernel(const CurveArgs a) {
    Table table(a);
    CurveRun run{-1, 0u, 0ull};
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * blockDim.x, t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (long long base = t0 - lane; base < a.groups; base += stride) {
        const long long g = base + lane;
        bool live = g < a.groups;
        uint4 rv = make_uint4(0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u);     // region == NULL: every voxel in region 1
        if (live && a.region) {
            rv = reinterpret_cast<const uint4*>(a.region)[g];
            live = (rv.x | rv.y | rv.z | rv.w) != 0;
        }
        float4 s[4] = {};
        uint4 cv = make_uint4(0, 0, 0, 0), gv = cv;
        if (live) {
#pragma unroll
            for (int j = 0; j < 4; ++j) s[j] = reinterpret_cast<const float4*>(a.score)[g * 4 + j];
            cv = reinterpret_cast<const uint4*>(a.ref)[g];
            if (a.gate) gv = reinterpret_cast<const uint4*>(a.gate)[g];
        }
        if (!__any(live)) continue;                                    // wave-uniform
        const float sc[16] = {s[0].x, s[0].y, s[0].z, s[0].w, s[1].x, s[1].y, s[1].z, s[1].w,
                              s[2].x, s[2].y, s[2].z, s[2].w, s[3].x, s[3].y, s[3].z, s[3].w};
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int r = (int)byte_of(rv, k);
            const bool valid = live && r >= 1 && r <= a.nregions;
            const bool on = !a.gate || byte_of(gv, k) != 0;
            const int b = curves_bin(sc[k], on, a.nbins, a.fbins);
            const int key = ((r - 1) * 2 + (byte_of(cv, k) != 0 ? 1 : 0)) * a.row + b;
            curves_step<CONF>(table, run, valid, key, (CONF && b > 0) ? curves_q(sc[k]) : 0u);
        }
    }
    for (long long base = a.groups * 16 + t0 - lane; base < a.nvox; base += stride) {
        const long long e = base + lane;
        bool valid = e < a.nvox;
        int key = 0;
        unsigned q = 0;
        if (valid) {
            const int r = a.region ? (int)a.region[e] : 1;
            valid = r >= 1 && r <= a.nregions;
            if (valid) {
                const float sv = a.score[e];
                const int b = curves_bin(sv, !a.gate || a.gate[e] != 0, a.nbins, a.fbins);
                key = ((r - 1) * 2 + (a.ref[e] != 0 ? 1 : 0)) * a.row + b;
                q = (CONF && b > 0) ? curves_q(sv) : 0u;
            }
        }
        curves_step<CONF>(table, run, valid, key, q);
    }
    curves_wave_send<CONF>(table, run.cnt > 0, run);
    table.finish(a);
}

static inline bool curves_shape_ok(int nregions, int nbins) {
    return nregions >= 1 && nregions <= 255 && nbins >= 2 && nbins <= CURVES_MAX_BINS && (nbins & (nbins - 1)) == 0;
}

static inline int64_t curves_lds_words(int nregions, int nbins, bool conf) {
    return (int64_t)nregions * 2 * (nbins + 1) * (conf ? 3 : 1);
}

static inline int curves_regime(int nregions, int nbins, bool conf) { return label_regime(curves_lds_words(nregions, nbins, conf)); }

}  // namespace dram

using namespace dram;

#define CURVES_SHAPE_MSG "score_hist: 1 <= nregions <= 255, nbins a power of two in 2..%d"

extern "C" int dram_score_hist_plan(int nregions, int nbins, int with_conf) {
    DRAM_REQUIRE(curves_shape_ok(nregions, nbins), CURVES_SHAPE_MSG, CURVES_MAX_BINS);
    return curves_regime(nregions, nbins, with_conf != 0);
}

extern "C" int dram_score_hist(const float* score, const uint8_t* ref, const uint8_t* region, const uint8_t* gate, int nregions,
                               int nbins, int64_t* hist, int64_t* conf, int64_t nvox, void* stream) {
    DRAM_REQUIRE(score && ref && hist, "score_hist: null pointer");
    DRAM_REQUIRE(nvox > 0 && nvox < (1LL << 31), "score_hist: nvox must be in 1 .. 2^31 - 1");
    DRAM_REQUIRE(curves_shape_ok(nregions, nbins), CURVES_SHAPE_MSG, CURVES_MAX_BINS);
    DRAM_REQUIRE(region || nregions == 1, "score_hist: without a region map there is one region (nregions == 1)");
    DRAM_REQUIRE(((uintptr_t)score & 3) == 0, "score_hist: misaligned score");
    hipStream_t st = (hipStream_t)stream;
    const int total = nregions * 2 * (nbins + 1);
    hipLaunchKernelGGL(curves_init_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, st, (unsigned long long*)hist,
                       (unsigned long long*)conf, total);
    const bool vec = aligned16(score) && aligned16(ref) && (!region || aligned16(region)) && (!gate || aligned16(gate));
    CurveArgs a{score, ref, region, gate, (unsigned long long*)hist, (unsigned long long*)conf, nregions, nbins, nbins + 1,
                (float)nbins, (long long)nvox, vec ? nvox / 16 : 0};
    const bool with_conf = conf != nullptr;
    const StreamLaunch g = stream_geometry(curves_lds_words(nregions, nbins, with_conf), nvox, a.groups, 2048);
    const char* who = "score_hist";
    int rc;
    if (curves_regime(nregions, nbins, with_conf) == CURVES_LDS)
        rc = with_conf ? launch_stream<score_hist_kernel<CurveLdsTable<true>, true>>(a, g, st, who)
                       : launch_stream<score_hist_kernel<CurveLdsTable<false>, false>>(a, g, st, who);
    else
        rc = with_conf ? launch_stream<score_hist_kernel<CurveGlobalTable<true>, true>>(a, g, st, who)
                       : launch_stream<score_hist_kernel<CurveGlobalTable<false>, false>>(a, g, st, who);
    if (rc != DRAM_OK) return rc;
    return check_launch("score_hist");
}
