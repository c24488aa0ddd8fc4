// What the per-label report kernels share (gfx950): density.hip, distribution.hip, curves.hip, shape.hip and the statistics
// kernels of components.hip.  Each reduces a volume into a small table per label, everything in integers: sums by integer
// atomics, minima and maxima by integer atomics, so no result depends on the order in which they land.
//
// A streaming report (density, distribution) serves two regimes, chosen by its *_plan entry from the size of the call's table
// alone (label_regime):
//   LABEL_LDS   the whole table fits in LABEL_LDS_WORDS of LDS (the lobe map: 5 labels with a 4096-bin histogram are 82 KiB).
//               One table per block (LdsLabelAcc): a thread keeps the moments of its current label in registers and goes to LDS
//               when the label changes; a count of a histogram or zone table is one 32-bit LDS atomic; at the end one set of
//               64-bit global atomics per occupied entry.
//   LABEL_WAVE  the table does not fit (component labels, or many labels with a histogram).  A thread folds its 16 voxels into
//               the run of its current label (WaveLabelAcc); at the end of a lap the lanes of a wave that hold the same label
//               are reduced together (wave_reduce_by_key) and the group's first lane sends one set of global atomics: a
//               component costs one set per wave and 1024 voxels, not one per voxel.  A label change inside a thread's 16
//               voxels sends the finished run directly.  Table counts go to global memory, equal consecutive entries of a
//               thread merged into one add.
// Both stream 16 voxels per thread with 16-byte loads where every input is 16-byte aligned, and fall back to one voxel per
// thread otherwise and for the last nvox % 16 voxels (stream_labels).
//
// Every call covers fewer than 2^31 voxels, so no 32-bit count kept in LDS or in a register can wrap, whatever the launch
// geometry.
#pragma once
#include "common.h"

namespace dram {

constexpr int LABEL_LDS = 0, LABEL_WAVE = 1;
constexpr int LABEL_MAX_BINS = 4096;
constexpr int LABEL_LDS_WORDS = 32768;       // 128 of the CU's 160 KiB
constexpr int LABEL_BIG_BYTES = 16384;       // a table above this: 1024 threads and one block per CU instead of 256 and eight

// ---- unpacking 16 voxels from 16-byte loads
__device__ __forceinline__ unsigned byte_of(const uint4& v, int k) {
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
    return (w[k >> 2] >> (8 * (k & 3))) & 0xffu;
}

// the labels of group g; false: all 16 are zero
template <class LabelT>
__device__ __forceinline__ bool labels16(const LabelT* labels, long long g, int (&l)[16]);

template <>
__device__ __forceinline__ bool labels16<uint8_t>(const uint8_t* labels, long long g, int (&l)[16]) {
    const uint4 v = reinterpret_cast<const uint4*>(labels)[g];
    // unpacked before the test, as the int32 labels are: an l[] that is written on one path only is carried round the lap loop
    // in 16 registers
#pragma unroll
    for (int k = 0; k < 16; ++k) l[k] = (int)byte_of(v, k);
    return (v.x | v.y | v.z | v.w) != 0;
}

template <>
__device__ __forceinline__ bool labels16<int32_t>(const int32_t* labels, long long g, int (&l)[16]) {
    int any = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int4 v = reinterpret_cast<const int4*>(labels)[g * 4 + j];
        l[4 * j] = v.x; l[4 * j + 1] = v.y; l[4 * j + 2] = v.z; l[4 * j + 3] = v.w;
        any |= v.x | v.y | v.z | v.w;
    }
    return any != 0;
}

// zeroes the labels of group g that the mask leaves out; false: it leaves out all 16
__device__ __forceinline__ bool mask16(const uint8_t* mask, long long g, int (&l)[16]) {
    const uint4 v = reinterpret_cast<const uint4*>(mask)[g];
#pragma unroll
    for (int k = 0; k < 16; ++k) l[k] = byte_of(v, k) ? l[k] : 0;
    return (v.x | v.y | v.z | v.w) != 0;
}

// ---- the streaming scaffold
// group(g, l) takes the 16 voxels of group g with their labels l (masked-out ones zeroed; never all zero), element(e, l) the
// voxel e with its label l != 0; both load their own second stream.  Both loops run a wave-uniform number of laps (the bound is
// tested on the wave's first index), so that acc.end_lap() is reached by all 64 lanes together.  Every index read lies below
// nvox: g < groups <= nvox / 16 in the first loop, e < nvox in the second.
template <class LabelT, class Acc, class Group, class Element>
__device__ __forceinline__ void stream_labels(const void* label_volume, const uint8_t* mask, long long groups, long long nvox, Acc& acc,
                                              Group&& group, Element&& element) {
    const LabelT* labels = static_cast<const LabelT*>(label_volume);
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * blockDim.x, t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (long long base = t0 - lane; base < groups; base += stride) {
        const long long g = base + lane;
        int l[16];
        if (g < groups && labels16<LabelT>(labels, g, l) && (!mask || mask16(mask, g, l))) group(g, l);
        acc.end_lap();
    }
    for (long long base = groups * 16 + t0 - lane; base < nvox; base += stride) {
        const long long e = base + lane;
        if (e < nvox) {
            const int l = (int)labels[e];
            if (l != 0 && (!mask || mask[e])) element(e, l);
        }
        acc.end_lap();
    }
    acc.finish();
}

// ---- the keyed wave reduction
// Called by all 64 lanes of a wave together.  For each distinct key among the pending lanes the payloads of the lanes that hold
// it are combined and send(key, combined) runs on the first of them; a lane alone with its key sends its own payload without
// the butterfly.  Every round serves the lanes that hold the key of the first lane still to do and clears at least that lane's
// bit, so the loop ends after at most 64 rounds.  A Payload has identity(), combine(other) and map(f); map applies f to every
// member and exists only so that __shfl_xor can be applied to each of them.  The payload is taken by value, which keeps the
// caller's own copy out of the loop (and out of its registers).
template <class Payload, class Send>
__device__ __forceinline__ void wave_reduce_by_key(bool pending, int key, const Payload p, Send&& send) {
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(pending);
    while (todo) {                                         // wave-uniform
        const int lead = __shfl(key, __ffsll((long long)todo) - 1, 64);
        const bool mine = pending && key == lead;
        const unsigned long long m = __ballot(mine);
        Payload r = p;                                     // a group of one: its first lane is the holder itself
        if (__popcll(m) > 1) {                             // wave-uniform
            r = mine ? p : Payload::identity();
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) r.combine(r.map([o](auto v) { return __shfl_xor(v, o, 64); }));
        }
        if (lane == __ffsll((long long)m) - 1) send(lead, r);          // one send site: two cost registers in every caller
        todo &= ~m;
    }
}

// N sums of type T as a payload
template <class T, int N>
struct WaveSums {
    T v[N];
    __device__ __forceinline__ static WaveSums identity() {
        WaveSums r;
#pragma unroll
        for (int e = 0; e < N; ++e) r.v[e] = 0;
        return r;
    }
    __device__ __forceinline__ void combine(const WaveSums& o) {
#pragma unroll
        for (int e = 0; e < N; ++e) v[e] += o.v[e];
    }
    template <class F>
    __device__ __forceinline__ WaveSums map(F f) const {
        WaveSums r;
#pragma unroll
        for (int e = 0; e < N; ++e) r.v[e] = f(v[e]);
        return r;
    }
};

// ---- the label-table accumulators
// A report's policy P supplies
//   Args                        the kernel's arguments, with the number of labels n
//   Value, MIN0, MAX0           the type of the minimum and maximum (int or unsigned) and what they start from
//   SUMS, TABLES                how many 64-bit sums a label has and how many 32-bit count tables the report keeps
//   row(a, t)                   the entries per label of count table t, 0 where the call has none
//   table(a, t)                 that table in global memory
//   send(a, label, moments)     the global atomics of one set of moments
// and the report's kernel adds a voxel by enter(label), then updating m and count(t, entry) for the tables it has.
template <class P>
struct LabelMoments {
    unsigned cnt;
    typename P::Value mn, mx;
    unsigned long long s[P::SUMS];
    __device__ __forceinline__ static LabelMoments identity() {
        LabelMoments r;
        r.cnt = 0; r.mn = P::MIN0; r.mx = P::MAX0;
#pragma unroll
        for (int j = 0; j < P::SUMS; ++j) r.s[j] = 0;
        return r;
    }
    __device__ __forceinline__ void see(typename P::Value v) {
        ++cnt;
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
    }
    __device__ __forceinline__ void combine(const LabelMoments& o) {
        cnt += o.cnt;
        mn = o.mn < mn ? o.mn : mn;
        mx = o.mx > mx ? o.mx : mx;
#pragma unroll
        for (int j = 0; j < P::SUMS; ++j) s[j] += o.s[j];
    }
    template <class F>
    __device__ __forceinline__ LabelMoments map(F f) const {
        LabelMoments r;
        r.cnt = f(cnt); r.mn = f(mn); r.mx = f(mx);
#pragma unroll
        for (int j = 0; j < P::SUMS; ++j) r.s[j] = f(s[j]);
        return r;
    }
};

// 32-bit words of a label's moments in LDS
template <class P>
constexpr int label_moment_words() { return 2 * P::SUMS + 3; }

extern __shared__ unsigned long long label_lds[];

// LABEL_LDS: the block's table {sums[SUMS][n] (64-bit), count[n], min[n], max[n], then the count tables (32-bit)}.
template <class P>
struct LdsLabelAcc {
    using Moments = LabelMoments<P>;
    const typename P::Args& a;
    unsigned long long* lsum;
    unsigned* lcnt;
    typename P::Value *lmn, *lmx;
    unsigned* ltab[P::TABLES];
    int n, label;                            // label 0: nothing pending
    Moments m;                               // of the voxels of `label` seen since the label last changed
    __device__ __forceinline__ LdsLabelAcc(const typename P::Args& a_) : a(a_), n(a_.n), label(0), m(Moments::identity()) {
        lsum = label_lds;
        lcnt = reinterpret_cast<unsigned*>(lsum + P::SUMS * n);
        lmn = reinterpret_cast<typename P::Value*>(lcnt + n);
        lmx = lmn + n;
        int words = n * label_moment_words<P>();
        unsigned* w = reinterpret_cast<unsigned*>(label_lds);
#pragma unroll
        for (int t = 0; t < P::TABLES; ++t) {
            ltab[t] = w + words;
            words += n * P::row(a, t);
        }
        for (int k = threadIdx.x; k < words; k += blockDim.x) w[k] = 0;
        __syncthreads();
        for (int k = threadIdx.x; k < n; k += blockDim.x) { lmn[k] = P::MIN0; lmx[k] = P::MAX0; }
        __syncthreads();
    }
    __device__ __forceinline__ void flush() {
        if (label > 0) {
            const int k = label - 1;
            atomicAdd(&lcnt[k], m.cnt);
            atomicMin(&lmn[k], m.mn);
            atomicMax(&lmx[k], m.mx);
#pragma unroll
            for (int j = 0; j < P::SUMS; ++j) atomicAdd(&lsum[j * n + k], m.s[j]);
        }
    }
    // false: a label outside 1..n, which touches nothing
    __device__ __forceinline__ bool enter(int l) {
        if (l < 1 || l > n) return false;
        if (l != label) { flush(); label = l; m = Moments::identity(); }
        return true;
    }
    __device__ __forceinline__ void count(int t, int entry) { atomicAdd(&ltab[t][entry], 1u); }
    __device__ __forceinline__ void end_lap() {}
    __device__ __forceinline__ void finish() {
        flush();
        __syncthreads();
        for (int k = threadIdx.x; k < n; k += blockDim.x) {
            Moments e;
            e.cnt = lcnt[k];
            if (e.cnt) {
                e.mn = lmn[k]; e.mx = lmx[k];
#pragma unroll
                for (int j = 0; j < P::SUMS; ++j) e.s[j] = lsum[j * n + k];
                P::send(a, k + 1, e);
            }
        }
#pragma unroll
        for (int t = 0; t < P::TABLES; ++t) {
            unsigned long long* out = P::table(a, t);
            for (int e = threadIdx.x; e < n * P::row(a, t); e += blockDim.x) {
                const unsigned c = ltab[t][e];
                if (c) atomicAdd(&out[e], (unsigned long long)c);
            }
        }
    }
};

// LABEL_WAVE: runs in registers, one set of global atomics per label and wave at the end of a lap.
template <class P>
struct WaveLabelAcc {
    using Moments = LabelMoments<P>;
    const typename P::Args& a;
    int n, label;                            // label 0: nothing pending
    Moments m;
    int pending[P::TABLES];                  // per count table the entry with adds not yet sent, -1: none
    unsigned pcnt[P::TABLES];
    __device__ __forceinline__ WaveLabelAcc(const typename P::Args& a_) : a(a_), n(a_.n), label(0), m(Moments::identity()) {
#pragma unroll
        for (int t = 0; t < P::TABLES; ++t) { pending[t] = -1; pcnt[t] = 0; }
    }
    __device__ __forceinline__ bool enter(int l) {
        if (l < 1 || l > n) return false;
        if (l != label) {
            if (label > 0) P::send(a, label, m);
            label = l;
            m = Moments::identity();
        }
        return true;
    }
    __device__ __forceinline__ void flush_table(int t) {
        if (pending[t] >= 0) atomicAdd(&P::table(a, t)[pending[t]], (unsigned long long)pcnt[t]);
        pending[t] = -1;
        pcnt[t] = 0;
    }
    __device__ __forceinline__ void count(int t, int entry) {
        if (entry != pending[t]) { flush_table(t); pending[t] = entry; }
        ++pcnt[t];
    }
    __device__ __forceinline__ void end_lap() {
        wave_reduce_by_key(label > 0, label, m, [&](int key, const Moments& r) { P::send(a, key, r); });
        label = 0;
        m = Moments::identity();
#pragma unroll
        for (int t = 0; t < P::TABLES; ++t) flush_table(t);
    }
    __device__ __forceinline__ void finish() {}
};

// ---- host side
inline bool label_kind_ok(int label_kind, int n) { return (label_kind == 0 || label_kind == 1) && n >= 1 && !(label_kind == 0 && n > 255); }

// rows of nbins + 2 entries (dram_hist_summary's layout) for n labels
inline bool hist_shape_ok(int n, int nbins) { return nbins >= 0 && nbins <= LABEL_MAX_BINS && (int64_t)n * (nbins + 2) < (1LL << 31); }

inline int label_regime(int64_t table_words) { return table_words <= LABEL_LDS_WORDS ? LABEL_LDS : LABEL_WAVE; }

// 16 voxels per thread where the inputs allow groups, and about four laps: one block per CU of 1024 threads for a large LDS
// table, eight of 256 for a small one, and up to wave_cap blocks of 256 threads without one.
struct StreamLaunch {
    unsigned grid, threads;
    size_t lds;
};
inline StreamLaunch stream_geometry(int64_t table_words, int64_t nvox, int64_t groups, int64_t wave_cap) {
    const bool in_lds = label_regime(table_words) == LABEL_LDS;
    const size_t lds = in_lds ? (size_t)table_words * 4 : 0;
    const bool big = lds > (size_t)LABEL_BIG_BYTES;
    const unsigned threads = big ? 1024 : 256;
    const int64_t want = cdiv64(groups > 0 ? groups : nvox, threads * 4), cap = !in_lds ? wave_cap : (big ? 256 : 2048);
    return {(unsigned)(want > cap ? cap : want), threads, lds};
}

// One LdsAttrOnce per kernel instantiation.
template <auto Kernel, class Args>
static int launch_stream(const Args& a, const StreamLaunch& g, hipStream_t st, const char* who) {
    if (g.lds > 65536) {
        static LdsAttrOnce once;
        const int rc = ensure_dynamic_lds((const void*)Kernel, g.lds, once, who);
        if (rc != DRAM_OK) return rc;
    }
    hipLaunchKernelGGL(Kernel, dim3(g.grid), dim3(g.threads), g.lds, st, a);
    return DRAM_OK;
}

}  // namespace dram
