// The training losses and their targets on the device, gfx950.  In this order: the pieces every section shares; the fused
// IntRegRefineLoss; the pieces of the affine-consistency losses; IntRegLoss (the hinge with an
// entropy term instead of the pseudo-label term); the two voxel-wise segmentation losses on a target that is given
// (BootBinCrossEntropy, BinaryCrossEntropySmooth) and the per-sample Tversky + focal loss on logits (SegOverlap); the regression
// targets of a batch; the C entry points.
//
// Every loss is a streaming pass that leaves one tuple of partial sums per block, a one-block kernel that adds the partials
// in a fixed order and forms the scalars, and a streaming backward.  No atomics anywhere: the same input gives the same
// bits.  The shared pieces, each defined once below:
//   stream_packs<V>     the grid-stride walk of one sample over two tensors, ENC_UNROLL 16-byte (V = 4) or 4-byte (V = 1)
//                       loads of each in flight per lane; all-or-nothing alignment, chosen on the host (enc_vec4)
//   block_partials<NS>  NS fp64 sums of every lane -> one tuple per block: butterfly per wave, then the four waves in order
//   block_totals<NS>    the same combine, read side: the result stays in registers of the one finishing block
//   sample_totals<NS>   one wave adds the tuples of one sample: lanes stride over the blocks, then a butterfly
//   Hinge               the interval hinge of one sample: its value in fp64 (finalise kernels), its gradient factor in fp32
//   seg_load_groups     the groups of four elements a lane of a segmentation kernel owns, by element index, with a per-tensor
//                       alignment flag and a ragged tail (seg_load4 / seg_store4)
// loss_partial_kernel and the masked smooth-L1 kernels predate these and keep their fp32 chunk sums (block_sum_256).
#include <cmath>
#include <type_traits>

#include "common.h"

namespace dram {

constexpr int LCHUNK = 8192;
constexpr int NSUM = 8;   // per (sample, chunk): sp, nm, so, no, T, A, B, Bo
constexpr float LEPS = 1e-7f;

// p = sigmoid(d) and q = 1 - p, each to full fp32 relative accuracy (the reference forms 1 - p from a rounded
// p, which loses every digit once p > 1 - 1e-6; the fp64 oracle is what the tests compare against)
__device__ __forceinline__ void sigmoid_pq(float d, float& p, float& q) {
    const float e = expf(-fabsf(d));
    const float r = 1.f / (1.f + e);
    const float hi = r, lo = e * r;
    p = d >= 0.f ? hi : lo;
    q = d >= 0.f ? lo : hi;
}
__device__ __forceinline__ float nlog_clamped(float v) { return -logf(fminf(fmaxf(v, LEPS), 1.f - LEPS)); }

// ---- shared pieces -------------------------------------------------------------------------------------------------------
constexpr int ENC_UNROLL = 4;          // loads of each tensor a lane has in flight

template <int V> struct EncPack;
template <> struct EncPack<4> { using type = float4; };
template <> struct EncPack<1> { using type = float; };
__device__ __forceinline__ float enc_lane(const float4& v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }
__device__ __forceinline__ float enc_lane(const float& v, int) { return v; }
__device__ __forceinline__ void enc_set(float4& v, int i, float x) { (i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w) = x; }
__device__ __forceinline__ void enc_set(float& v, int, float x) { v = x; }

// What a lane holds in one step of stream_packs: pack u is pack base + u * 256 + threadIdx.x of the sample, where ok[u].
template <int V> struct PackStep {
    typename EncPack<V>::type a[ENC_UNROLL], b[ENC_UNROLL];
    bool ok[ENC_UNROLL];
    int64_t base;
    // elem(k, a, b) for every element the lane holds, in (u, k) order; done(pack index) after the elements of each pack
    template <class Elem, class Done>
    __device__ __forceinline__ void each(Elem&& elem, Done&& done) const {
#pragma unroll
        for (int u = 0; u < ENC_UNROLL; ++u) {
            if (!ok[u]) continue;
#pragma unroll
            for (int k = 0; k < V; ++k) elem(k, enc_lane(a[u], k), enc_lane(b[u], k));
            done(base + u * 256 + threadIdx.x);
        }
    }
    template <class Elem>
    __device__ __forceinline__ void each(Elem&& elem) const { each(elem, [](int64_t) {}); }
};
// The nblk blocks of a sample walk its S / V packs of a[] and b[] with a grid stride; step(PackStep) once per step.
// V = 4: S is a multiple of 4 and both bases are 16-byte aligned, so every sample starts on a 16-byte boundary and a pack is
// inside [0, S) whenever its first element is.  V = 1: any S, any alignment.
template <int V, class Step>
__device__ __forceinline__ void stream_packs(const float* __restrict__ a, const float* __restrict__ b, int64_t S, int nblk,
                                             Step&& step) {
    using T = typename EncPack<V>::type;
    const T* pa = reinterpret_cast<const T*>(a);
    const T* pb = reinterpret_cast<const T*>(b);
    const int64_t packs = S / V;                             // packs of this sample
    const int64_t stride = (int64_t)nblk * 256 * ENC_UNROLL;   // packs all blocks of the sample cover per step
    for (int64_t base = (int64_t)blockIdx.x * 256 * ENC_UNROLL; base < packs; base += stride) {
        PackStep<V> st;
        st.base = base;
#pragma unroll
        for (int u = 0; u < ENC_UNROLL; ++u) {
            const int64_t i = base + u * 256 + threadIdx.x;
            st.ok[u] = i < packs;
            if (st.ok[u]) { st.a[u] = pa[i]; st.b[u] = pb[i]; }
        }
        step(st);
    }
}

// acc[NS] of every lane -> dst[q]: butterfly per wave, then the four waves in order
template <int NS>
__device__ __forceinline__ void block_partials(const double (&acc)[NS], double (*red)[4], double* __restrict__ dst) {
#pragma unroll
    for (int q = 0; q < NS; ++q) {
        const double s = wave_sum_d(acc[q]);
        if ((threadIdx.x & 63) == 0) red[q][threadIdx.x >> 6] = s;
    }
    __syncthreads();
    if (threadIdx.x < NS)
        dst[threadIdx.x] = ((red[threadIdx.x][0] + red[threadIdx.x][1]) + red[threadIdx.x][2]) + red[threadIdx.x][3];
}
// the same combine with the result in tot[] of every thread
template <int NS>
__device__ __forceinline__ void block_totals(const double (&s)[NS], double (*red)[4], double (&tot)[NS]) {
#pragma unroll
    for (int q = 0; q < NS; ++q) {
        const double w = wave_sum_d(s[q]);
        if ((threadIdx.x & 63) == 0) red[q][threadIdx.x >> 6] = w;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NS; ++q) tot[q] = ((red[q][0] + red[q][1]) + red[q][2]) + red[q][3];
}
// s[q] = sum over the nblk tuples part[(n * nblk + b) * NS + q] of sample n, in every lane of the calling wave
template <int NS>
__device__ __forceinline__ void sample_totals(const double* __restrict__ part, int n, int nblk, double (&s)[NS]) {
#pragma unroll
    for (int q = 0; q < NS; ++q) s[q] = 0.0;
    for (int b = threadIdx.x & 63; b < nblk; b += 64)
#pragma unroll
        for (int q = 0; q < NS; ++q) s[q] += part[((size_t)n * nblk + b) * NS + q];
#pragma unroll
    for (int q = 0; q < NS; ++q) s[q] = wave_sum_d(s[q]);
}

// The interval hinge of sample n, max((r - c)^2 - K, 0) / w with c = (lo + hi) / 2 and K = (hi - lo)^2 / 4, of the lobe's
// mean probability r = sum_v p m / nm.
struct Hinge {
    float lo, hi, w;
    __device__ __forceinline__ Hinge(const float* __restrict__ targets, const float* __restrict__ weight, int n)
        : lo(targets[2 * n]), hi(targets[2 * n + 1]), w(weight[n]) {}
    __device__ __forceinline__ double value(double r) const {
        const double l = lo, h = hi;
        const double K = 0.25 * (h - l) * (h - l);
        const double v = (r - 0.5 * (h + l)) * (r - 0.5 * (h + l)) - K;
        return (v > 0.0 ? v : 0.0) / (double)w;
    }
    // g0 * d value / d p_v for a lobe voxel v
    __device__ __forceinline__ float grad(float r, float nm, float g0) const {
        const float c = 0.5f * (hi + lo), K = 0.25f * (hi - lo) * (hi - lo);
        const float hinge = ((r - c) * (r - c) - K) > 0.f ? 1.f : 0.f;
        return g0 * hinge * 2.f * (r - c) / (w * nm);
    }
};


// ---- IntRegRefineLoss, fused ------------------------------------------------------------------------------------------------
// Replaces the ~30 element-wise / reduction ATen dispatches -- and the per-sample host round trips --
// of the reference's training loss, dram/metrics.py: IntRegLoss.compute_reg_loss_with_probs (158-177),
// IntRegRefineLoss.compute_seg_loss (331-358) with BootBinCrossEntropy (17-51), __call__ (360-373).
//
//   p      = sigmoid(refined), pd = sigmoid(dense)   (DC3D: refined is dense; DC3DATGeneric: the PCM output)
//   reg    = sum_n max((r_n - c_n)^2 - K_n, 0) / w_n,   r_n = sum_v pd m / sum_v m   (m = lobe mask)
//   t      = [pd > 0.5] [m] [lesion > 0] keep_n          (pseudo label, no gradient)
//   seg    = mean_{m=0} -log(1-p)  +  (1-s) * (alpha A + (1-alpha) B) / (alpha T + (1-alpha)(n_in - T))  +  s * mean_{m=1} -log(max(p,1-p))
//            A = sum_{t=1} -log p,  B = sum_{m=1,t=0} -log(1-p),  T = sum t,  alpha = clamp(1 - T/n_in, .25, .75)
//            (all logs of values clamped to [eps, 1-eps], eps = 1e-7, as torch.clamp: zero gradient outside)
// One streaming pass produces every sum (HBM-bound: 12 B/voxel read), a one-block fp64 finalise turns
// them into the two scalars, and the backward is one more streaming pass (12 B read + 4 B written).
__global__ __launch_bounds__(256) void loss_partial_kernel(const float* __restrict__ dense, const float* __restrict__ refined,
                                                           const float* __restrict__ lobes,
                                                           const float* __restrict__ lesions, const float* __restrict__ keep,
                                                           float* __restrict__ part, int64_t S, int nchunks) {
    __shared__ float red[4];
    const int n = blockIdx.y, chunk = blockIdx.x;
    const int64_t beg = (int64_t)chunk * LCHUNK;
    const int len = (int)((S - beg) < LCHUNK ? (S - beg) : LCHUNK);
    const float kp = keep[n];
    const float* pd = dense + (int64_t)n * S + beg;
    const float* pr = refined + (int64_t)n * S + beg;
    const bool same = dense == refined;
    const float* pm = lobes + (int64_t)n * S + beg;
    const float* pl = lesions + (int64_t)n * S + beg;
    float acc[NSUM] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int e = threadIdx.x; e < len; e += 256) {
        float p, q, pden, qden;
        const float dv = pd[e];
        sigmoid_pq(dv, pden, qden);
        if (same) { p = pden; q = qden; }
        else sigmoid_pq(pr[e], p, q);
        const bool in = pm[e] > 0.f;
        if (in) {
            acc[0] += pden;
            acc[1] += 1.f;
            const bool t = (pden > 0.5f) && (pl[e] > 0.f) && (kp > 0.f);
            if (t) { acc[4] += 1.f; acc[5] += nlog_clamped(p); }
            else acc[6] += nlog_clamped(q);
            acc[7] += nlog_clamped(fmaxf(p, q));
        } else {
            acc[2] += nlog_clamped(q);
            acc[3] += 1.f;
        }
    }
    float* o = part + ((size_t)n * nchunks + chunk) * NSUM;
#pragma unroll
    for (int q = 0; q < NSUM; ++q) {
        const float s = block_sum_256(acc[q], red);
        if (threadIdx.x == 0) o[q] = s;
    }
}

// state: [0] alpha, [1] wsum, [2] n_in, [3] n_out, then per sample {r_n, nm_n}
// Deterministic: per-sample sums in fp64 by one thread each (fixed chunk order), then thread 0 combines the
// samples in index order.
// An empty sum contributes 0 (tests/test_gpu_refine_loss_kernels.py):
//   no outside voxel in the batch   the outside mean is 0 and so is its gradient (torch: the mean of an empty tensor, NaN)
//   no inside voxel in the batch    the inside terms are 0, alpha = 0, wsum = 1 (the reference's `if tf.sum() > 0`)
//   a sample with an empty lobe     adds 0 to reg whatever its targets (NaN included, which Batch.on_device gives such a
//                                   sample); its nm_n is 0 and its r_n is NaN, which the backward reads into a factor that
//                                   no voxel uses.  Every other state entry, both losses and every gradient stay finite.
__global__ __launch_bounds__(256) void loss_finalize_kernel(const float* __restrict__ part, double* __restrict__ ssum,
                                                            const float* __restrict__ targets,
                                                            const float* __restrict__ weight, float smoothing, int N,
                                                            int nchunks, float* __restrict__ out, float* __restrict__ state) {
    for (int n = threadIdx.x; n < N; n += 256) {
        double s[NSUM] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int c = 0; c < nchunks; ++c)
            for (int q = 0; q < NSUM; ++q) s[q] += part[((size_t)n * nchunks + c) * NSUM + q];
        for (int q = 0; q < NSUM; ++q) ssum[(size_t)n * NSUM + q] = s[q];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot[NSUM] = {0, 0, 0, 0, 0, 0, 0, 0};
        double regs = 0.0;
        for (int n = 0; n < N; ++n) {
            const double* s = ssum + (size_t)n * NSUM;
            const double r = s[0] / s[1];
            state[4 + 2 * n] = (float)r;
            state[5 + 2 * n] = (float)s[1];
            regs += Hinge(targets, weight, n).value(r);
            for (int q = 0; q < NSUM; ++q) tot[q] += s[q];
        }
        const double n_in = tot[1], n_out = tot[3], T = tot[4];
        double seg = n_out > 0 ? tot[2] / n_out : 0.0;     // torch: mean of an empty tensor is nan; callers always have an outside
        double alpha = 0.0, wsum = 1.0;
        if (n_in > 0) {
            alpha = 1.0 - T / n_in;
            alpha = alpha < 0.25 ? 0.25 : (alpha > 0.75 ? 0.75 : alpha);
            wsum = alpha * T + (1.0 - alpha) * (n_in - T);
            seg += (1.0 - smoothing) * (alpha * tot[5] + (1.0 - alpha) * tot[6]) / wsum + smoothing * tot[7] / n_in;
        }
        out[0] = (float)regs;
        out[1] = (float)seg;
        state[0] = (float)alpha; state[1] = (float)wsum; state[2] = (float)n_in; state[3] = (float)n_out;
    }
}

// d(g0*reg + g1*seg)/d dense
__global__ __launch_bounds__(256) void loss_bwd_kernel(const float* __restrict__ dense, const float* __restrict__ refined,
                                                       const float* __restrict__ lobes,
                                                       const float* __restrict__ lesions, const float* __restrict__ keep,
                                                       const float* __restrict__ targets, const float* __restrict__ weight,
                                                       const float* __restrict__ state, const float* __restrict__ gout,
                                                       float smoothing, float* __restrict__ ddense,
                                                       float* __restrict__ drefined, int64_t S) {
    const int n = blockIdx.y;
    const float g0 = gout[0], g1 = gout[1];
    const float alpha = state[0], wsum = state[1], n_in = state[2], n_out = state[3];
    const float r = state[4 + 2 * n], nm = state[5 + 2 * n];
    const float greg = Hinge(targets, weight, n).grad(r, nm, g0);          // d reg / d p_v for m_v = 1
    const float kp = keep[n];
    const float c_out = n_out > 0.f ? g1 / n_out : 0.f;
    const float c_a = n_in > 0.f ? g1 * (1.f - smoothing) * alpha / wsum : 0.f;
    const float c_b = n_in > 0.f ? g1 * (1.f - smoothing) * (1.f - alpha) / wsum : 0.f;
    const float c_boot = n_in > 0.f ? g1 * smoothing / n_in : 0.f;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < S; e += stride) {
        const int64_t o = (int64_t)n * S + e;
        float p, q, pden, qden;
        sigmoid_pq(dense[o], pden, qden);
        if (drefined) sigmoid_pq(refined[o], p, q);
        else { p = pden; q = qden; }
        // d(-log(clamp(v)))/dv = -1/v inside [eps, 1-eps], 0 outside; p in [eps, 1-eps] <=> q in [eps, 1-eps]
        const bool live = p >= LEPS && q >= LEPS;
        const float dlp = live ? -1.f / p : 0.f;      // of -log p      w.r.t. p
        const float dlq = live ? 1.f / q : 0.f;       // of -log(1-p)   w.r.t. p
        float gseg, gr = 0.f;
        if (lobes[o] > 0.f) {
            const bool t = (pden > 0.5f) && (lesions[o] > 0.f) && (kp > 0.f);
            gr = greg;
            gseg = (t ? c_a * dlp : c_b * dlq) + c_boot * (p > 0.5f ? dlp : dlq);
        } else {
            gseg = c_out * dlq;
        }
        if (drefined) {
            ddense[o] = gr * pden * qden;
            drefined[o] = gseg * p * q;
        } else {
            ddense[o] = (gr + gseg) * p * q;
        }
    }
}


// ---- pieces of the affine-consistency losses (IntRegAffRefineLoss, dram/metrics.py:376-462) -----------------------
// F.sigmoid as its own differentiable op (the consistency term compares probabilities), and
// F.smooth_l1_loss(a[m > 0], b[m > 0]) (beta = 1, mean) with the mask m[N,1,S] expanded over the C channels of a, b.
__global__ void sigmoid_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
        float p, q;
        sigmoid_pq(x[e], p, q);
        y[e] = p;
    }
}
__global__ void sigmoid_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ dx, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
        float p, q;
        sigmoid_pq(x[e], p, q);          // p * (1 - p) with 1 - p at full relative accuracy
        dx[e] = dy[e] * p * q;
    }
}

// part[(row*nchunks + chunk)*2] = {sum of the smooth-L1 terms over masked elements, number of masked elements}
__global__ __launch_bounds__(256) void masked_smooth_l1_partial_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                       const float* __restrict__ mask, float* __restrict__ part,
                                                                       int C, int64_t S, int nchunks) {
    __shared__ float red[4];
    const int64_t row = blockIdx.y;            // n*C + c
    const int n = (int)(row / C);
    const int64_t beg = (int64_t)blockIdx.x * LCHUNK;
    const int len = (int)((S - beg) < LCHUNK ? (S - beg) : LCHUNK);
    const float* pa = a + row * S + beg;
    const float* pb = b + row * S + beg;
    const float* pm = mask + (int64_t)n * S + beg;
    float s = 0.f, cnt = 0.f;
    for (int e = threadIdx.x; e < len; e += 256) {
        if (pm[e] > 0.f) {
            const float d = fabsf(pa[e] - pb[e]);
            s += d < 1.f ? 0.5f * d * d : d - 0.5f;
            cnt += 1.f;
        }
    }
    s = block_sum_256(s, red);
    cnt = block_sum_256(cnt, red);
    if (threadIdx.x == 0) {
        part[((size_t)row * nchunks + blockIdx.x) * 2] = s;
        part[((size_t)row * nchunks + blockIdx.x) * 2 + 1] = cnt;
    }
}
// out[0] = mean, out[1] = count; fixed-order fp64 sum by one block
__global__ __launch_bounds__(256) void masked_smooth_l1_finalize_kernel(const float* __restrict__ part, int64_t items,
                                                                        float* __restrict__ out) {
    __shared__ double red[2][4];
    double s[2] = {0.0, 0.0}, tot[2];
    for (int64_t i = threadIdx.x; i < items; i += 256) { s[0] += part[2 * i]; s[1] += part[2 * i + 1]; }
    block_totals<2>(s, red, tot);
    if (threadIdx.x == 0) {
        out[0] = (float)(tot[0] / tot[1]);          // an empty selection gives nan, like torch's mean of an empty tensor
        out[1] = (float)tot[1];
    }
}
__global__ void masked_smooth_l1_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                            const float* __restrict__ mask, const float* __restrict__ out,
                                            const float* __restrict__ gout, float* __restrict__ da, float* __restrict__ db,
                                            int C, int64_t S) {
    const int64_t row = blockIdx.y;
    const int n = (int)(row / C);
    const float g = gout[0] / out[1];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < S; e += stride) {
        float v = 0.f;
        if (mask[(int64_t)n * S + e] > 0.f) {
            const float d = a[row * S + e] - b[row * S + e];
            v = g * fminf(fmaxf(d, -1.f), 1.f);      // d/dd of the smooth-L1 term: d inside (-1,1), sign(d) outside
        }
        if (da) da[row * S + e] = v;
        if (db) db[row * S + e] = -v;
    }
}

static inline int loss_chunks(int64_t S) { return (int)cdiv64(S, LCHUNK); }


// ---- IntRegLoss / IntRegAffLoss (dram/metrics.py:75-308): the interval hinge with an entropy term --------------------
//   p   = sigmoid(dense)
//   reg = sum_n max((r_n - c_n)^2 - K_n, 0) / w_n,  r_n = sum_v p m / sum_v m       (compute_reg_loss_with_probs, 158-177)
//   enc = mean over all N*S elements of  -p log(p + 1e-7) + (p - 1) log(1 - p + 1e-7)        (compute_enc_loss, 154-156)
// The entropy is evaluated as the reference's fp32 expression evaluates it: 1 - p is formed from the ROUNDED p (it is
// exactly 0 once p rounds to 1) and the 1e-7 is added after, so every logarithm sees at least 1e-7 and no finite logit
// gives a non-finite value.  The lesion mask does not enter: it reaches the loss through the regression band `targets`
// only (get_labels, 122-138), which the caller computes with the batch.
// Forward: one pass over dense and lobes (8 B/voxel, stream_packs); a block keeps its three sums in fp64 across steps and
// writes one fp64 partial triple; one block then adds the partials in a fixed order.
// Backward: one pass, 8 B/voxel read and 4 B/voxel written.
constexpr int ENC_NSUM = 3;            // per (sample, block): sum of p inside the lobe, lobe voxels, sum of the entropy terms
constexpr int ENC_MAX_BLOCKS = 2048;   // blocks of one launch (about 8 per CU), shared between the samples

__device__ __forceinline__ float enc_term(float p) {
    const float q = 1.f - p;
    return -p * logf(p + LEPS) + (p - 1.f) * logf(q + LEPS);
}
// d enc_term / dp
__device__ __forceinline__ float enc_term_dp(float p) {
    const float q = 1.f - p;
    return -logf(p + LEPS) - p / (p + LEPS) + logf(q + LEPS) + q / (q + LEPS);
}

template <int V>
__global__ __launch_bounds__(256) void enc_partial_kernel(const float* __restrict__ dense, const float* __restrict__ lobes,
                                                          double* __restrict__ part, int64_t S, int nblk) {
    __shared__ double red[ENC_NSUM][4];
    const int n = blockIdx.y;
    double acc[ENC_NSUM] = {0.0, 0.0, 0.0};
    stream_packs<V>(dense + (int64_t)n * S, lobes + (int64_t)n * S, S, nblk, [&](const PackStep<V>& st) {
        float sp = 0.f, nm = 0.f, ent = 0.f;
        st.each([&](int, float d, float m) {
            float p, q;
            sigmoid_pq(d, p, q);
            if (m > 0.f) { sp += p; nm += 1.f; }
            ent += enc_term(p);
        });
        acc[0] += sp; acc[1] += nm; acc[2] += ent;
    });
    block_partials<ENC_NSUM>(acc, red, part + ((size_t)n * nblk + blockIdx.x) * ENC_NSUM);
}

// state: per sample {r_n, nm_n}.  One wave per sample adds that sample's partials, thread 0 combines the samples in index
// order.
__global__ __launch_bounds__(256) void enc_finalize_kernel(const double* __restrict__ part, double* __restrict__ ssum,
                                                           const float* __restrict__ targets, const float* __restrict__ weight,
                                                           int N, int64_t S, int nblk, float* __restrict__ out,
                                                           float* __restrict__ state) {
    for (int n = threadIdx.x >> 6; n < N; n += 4) {
        double s[ENC_NSUM];
        sample_totals<ENC_NSUM>(part, n, nblk, s);
        if ((threadIdx.x & 63) == 0)
            for (int q = 0; q < ENC_NSUM; ++q) ssum[(size_t)n * ENC_NSUM + q] = s[q];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double regs = 0.0, ent = 0.0;
        for (int n = 0; n < N; ++n) {
            const double* s = ssum + (size_t)n * ENC_NSUM;
            const double r = s[0] / s[1];
            state[2 * n] = (float)r;
            state[2 * n + 1] = (float)s[1];
            regs += Hinge(targets, weight, n).value(r);
            ent += s[2];
        }
        out[0] = (float)regs;
        out[1] = (float)(ent / ((double)N * (double)S));
    }
}

// d(g0*reg + g1*enc)/d dense; d p / d dense = p (1 - p) with the rounded p, as autograd's sigmoid backward forms it
template <int V>
__global__ __launch_bounds__(256) void enc_bwd_kernel(const float* __restrict__ dense, const float* __restrict__ lobes,
                                                      const float* __restrict__ targets, const float* __restrict__ weight,
                                                      const float* __restrict__ state, const float* __restrict__ gout,
                                                      float* __restrict__ ddense, int N, int64_t S) {
    using T = typename EncPack<V>::type;
    const int n = blockIdx.y;
    const float g0 = gout[0], g1 = gout[1];
    const float r = state[2 * n], nm = state[2 * n + 1];
    const float greg = Hinge(targets, weight, n).grad(r, nm, g0);          // d reg / d p_v for m_v = 1
    const float genc = (float)((double)g1 / ((double)N * (double)S));
    const bool with_enc = g1 != 0.f;                         // the transformed batch of IntRegAffLoss takes reg alone
    T* po = reinterpret_cast<T*>(ddense + (int64_t)n * S);
    stream_packs<V>(dense + (int64_t)n * S, lobes + (int64_t)n * S, S, (int)gridDim.x, [&](const PackStep<V>& st) {
        T g;
        st.each(
            [&](int k, float d, float m) {
                float p, q;
                sigmoid_pq(d, p, q);
                float gp = m > 0.f ? greg : 0.f;
                if (with_enc) gp += genc * enc_term_dp(p);
                enc_set(g, k, gp * p * (1.f - p));
            },
            [&](int64_t i) { po[i] = g; });
    });
}

static inline int enc_blocks(int N, int64_t S, int V) {      // blocks per sample: a function of (N, S, V) alone
    const int64_t want = cdiv64(S / V, 256 * ENC_UNROLL), cap = cdiv64(ENC_MAX_BLOCKS, N);
    return (int)(want < cap ? want : cap);
}
static inline int enc_blocks_max(int N, int64_t S) { return enc_blocks(N, S, 1); }
// whether a launch over these tensors may take V = 4
template <class... P>
static inline bool enc_vec4(int64_t S, const P*... tensor) { return S % 4 == 0 && ((... | (uintptr_t)tensor) & 15) == 0; }


// ---- BootBinCrossEntropy (dram/metrics.py:10-51) and BinaryCrossEntropySmooth (53-72) with a target that is GIVEN ------
//   nll     = -log(clamp(p t + (1 - p)(1 - t), eps, 1 - eps)),  nll_hat the same with t_hat = [p > 0.5],  eps = 1e-7
//   boot    = mean_{voi < 1e-7} nll  +  (1 - s) (alpha A + (1 - alpha) B) / (alpha T + (1 - alpha)(n_in - T))  +  s mean_{voi > 0} nll_hat
//             A = sum_{voi > 0} t nll,  B = sum_{voi > 0} (1 - t) nll,  T = sum_{voi > 0} t,  alpha = clamp(1 - T / n_in, .25, .75)
//   smooth  = -s (alpha P1 + (1 - alpha) P2) / (alpha T + (1 - alpha)(n - T)),   alpha = clamp(1 - T / n, .3, .7)
//             P1 = sum t log pc,  P2 = sum (1 - t) log(1 - pc),  pc = clamp(p, 1e-6, 1 - 1e-6)
// alpha is a function of the sums alone, so sum nll w = alpha A + (1 - alpha) B needs no second pass over the tensor.
// Forward: block b owns elements [b SEG_CHUNK, (b + 1) SEG_CHUNK) and writes ONE fp64 partial tuple; lane l of step u owns
// the four elements from (u 256 + l) 4 of that range.  The ownership is by element INDEX, never by address, and every sum
// is added in one fixed order (four elements in fp32, steps in fp64, butterfly, four waves), so the bits do not depend on
// grid size, alignment or mask type.  A tensor whose base allows it is read with one 16-byte load per lane and step (one
// 4-byte load for a uint8 mask); a tensor that is not aligned, and the last group where n is no multiple of 4, with
// element loads.  One block then adds the partials in a fixed order and takes the reference's `tf.sum() > 0` branch.
// Backward: one pass, the same ownership, dp written with 16-byte stores where dp allows it.
constexpr int SEG_CHUNK = 4096;        // elements per block = per partial tuple
constexpr int SEG_UNROLL = SEG_CHUNK / (256 * 4);      // 16-byte loads of each tensor a lane has in flight
constexpr int BOOT_NSUM = 7;           // n_out, sum_out nll, n_in, T, A, B, sum_in nll_hat
constexpr int SMOOTH_NSUM = 3;         // T, P1, P2
constexpr int SEG_TOTALS = 8;          // doubles at the head of the workspace: the totals, then the partials
constexpr int SEG_STATE = 8;           // floats of the state the backward reads
constexpr float SEPS = 1e-6f;

template <int KIND> struct SegMask;
template <> struct SegMask<0> { using type = uint8_t; };
template <> struct SegMask<2> { using type = float; };

// the (up to) four elements from b[i]; vec: b is aligned for one access of the whole group
__device__ __forceinline__ void seg_load4(const float* b, int64_t i, bool vec, int cnt, float (&v)[4]) {
    if (vec && cnt == 4) {
        const float4 q = *reinterpret_cast<const float4*>(b + i);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = e < cnt ? b[i + e] : 0.f;
    }
}
__device__ __forceinline__ void seg_load4(const uint8_t* b, int64_t i, bool vec, int cnt, float (&v)[4]) {
    if (vec && cnt == 4) {
        const uchar4 q = *reinterpret_cast<const uchar4*>(b + i);
        v[0] = (float)q.x; v[1] = (float)q.y; v[2] = (float)q.z; v[3] = (float)q.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = e < cnt ? (float)b[i + e] : 0.f;
    }
}
__device__ __forceinline__ void seg_store4(float* b, int64_t i, bool vec, int cnt, const float (&v)[4]) {
    if (vec && cnt == 4) {
        *reinterpret_cast<float4*>(b + i) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < cnt) b[i + e] = v[e];
    }
}
// elements of group (u, lane) of block `blk` that lie inside [0, n): 0 .. 4
__device__ __forceinline__ int seg_group(int64_t n, int u, int64_t& i) {
    i = (int64_t)blockIdx.x * SEG_CHUNK + (int64_t)(u * 256 + threadIdx.x) * 4;
    const int64_t left = n - i;
    return left >= 4 ? 4 : (left > 0 ? (int)left : 0);
}

// One tensor of a segmentation kernel: its base, whether the base allows one access per group, and where its values go
template <class T> struct SegSrc {
    const T* b;
    int vec;
    float (*v)[4];
    __device__ __forceinline__ SegSrc(const T* b_, int vec_, float (*v_)[4]) : b(b_), vec(vec_), v(v_) {}
};
// The groups of this lane: cnt[u] elements from index at[u], and their values of every tensor in src (read in that order)
template <class... T>
__device__ __forceinline__ void seg_load_groups(int64_t n, int (&cnt)[SEG_UNROLL], int64_t (&at)[SEG_UNROLL], SegSrc<T>... src) {
#pragma unroll
    for (int u = 0; u < SEG_UNROLL; ++u) {
        cnt[u] = seg_group(n, u, at[u]);
        if (cnt[u] > 0) (seg_load4(src.b, at[u], src.vec != 0, cnt[u], src.v[u]), ...);
    }
}

// tot[q] = sum of part[b * NS + q] over the nblk blocks (lanes stride over the blocks, then block_totals)
template <int NS>
__device__ __forceinline__ void seg_total(const double* __restrict__ part, int64_t nblk, double (*red)[4], double (&tot)[NS]) {
    double s[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) s[q] = 0.0;
    for (int64_t b = threadIdx.x; b < nblk; b += 256)
#pragma unroll
        for (int q = 0; q < NS; ++q) s[q] += part[(size_t)b * NS + q];
    block_totals<NS>(s, red, tot);
}

template <int KT, int KV>
__global__ __launch_bounds__(256) void boot_bce_partial_kernel(const float* __restrict__ p,
                                                               const typename SegMask<KT>::type* __restrict__ t,
                                                               const typename SegMask<KV>::type* __restrict__ voi,
                                                               double* __restrict__ part, int64_t n, int vecp, int vect,
                                                               int vecv) {
    __shared__ double red[BOOT_NSUM][4];
    float pv[SEG_UNROLL][4], tv[SEG_UNROLL][4], vv[SEG_UNROLL][4];
    int cnt[SEG_UNROLL];
    int64_t at[SEG_UNROLL];
    seg_load_groups(n, cnt, at, SegSrc(p, vecp, pv), SegSrc(t, vect, tv), SegSrc(voi, vecv, vv));
    double acc[BOOT_NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int u = 0; u < SEG_UNROLL; ++u) {
        float s[BOOT_NSUM] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (e >= cnt[u]) continue;
            const float pe = pv[u][e], te = tv[u][e], ve = vv[u][e];
            const float nll = nlog_clamped(pe * te + (1.f - pe) * (1.f - te));
            if (ve < LEPS) { s[0] += 1.f; s[1] += nll; }
            if (ve > 0.f) {
                s[2] += 1.f;
                s[3] += te;
                s[4] += te * nll;
                s[5] += (1.f - te) * nll;
                s[6] += nlog_clamped(pe > 0.5f ? pe : 1.f - pe);
            }
        }
#pragma unroll
        for (int q = 0; q < BOOT_NSUM; ++q) acc[q] += s[q];
    }
    block_partials<BOOT_NSUM>(acc, red, part + (size_t)blockIdx.x * BOOT_NSUM);
}

// tot (8 doubles): the seven totals.  state: [0] 1 / n_out (0 without an outside), [1] alpha, [2] 1 / sum w, [3] 1 / n_in,
// [4] 1 if the inside part exists, else 0 (and [1..3] are 0).
__global__ __launch_bounds__(256) void boot_bce_finish_kernel(const double* __restrict__ part, int64_t nblk, double smoothing,
                                                              double* __restrict__ tot_out, float* __restrict__ out,
                                                              float* __restrict__ state) {
    __shared__ double red[BOOT_NSUM][4];
    double tot[BOOT_NSUM];
    seg_total<BOOT_NSUM>(part, nblk, red, tot);
    if (threadIdx.x != 0) return;
    const double n_out = tot[0], n_in = tot[2], T = tot[3];
    double loss = tot[1] / n_out;          // no outside: 0 / 0 = nan, torch's mean of an empty tensor
    double alpha = 0.0, inv_w = 0.0, inv_in = 0.0;
    const bool inside = n_in > 0.0;        // the reference's `if tf.sum() > 0`, taken here
    if (inside) {
        alpha = 1.0 - T / n_in;
        alpha = alpha < 0.25 ? 0.25 : (alpha > 0.75 ? 0.75 : alpha);
        inv_w = 1.0 / (alpha * T + (1.0 - alpha) * (n_in - T));
        inv_in = 1.0 / n_in;
        loss += (1.0 - smoothing) * (alpha * tot[4] + (1.0 - alpha) * tot[5]) * inv_w + smoothing * tot[6] * inv_in;
    }
    out[0] = (float)loss;
#pragma unroll
    for (int q = 0; q < BOOT_NSUM; ++q) tot_out[q] = tot[q];
    tot_out[BOOT_NSUM] = 0.0;
    state[0] = n_out > 0.0 ? (float)(1.0 / n_out) : 0.f;
    state[1] = (float)alpha; state[2] = (float)inv_w; state[3] = (float)inv_in; state[4] = inside ? 1.f : 0.f;
    state[5] = 0.f; state[6] = 0.f; state[7] = 0.f;
}

// dp = gout * d loss / d p.  torch.clamp passes the gradient where eps <= x <= 1 - eps, bounds included, and gives 0
// outside; t_hat and alpha are constants; the upstream gradient multiplies last, so it scales every element exactly.
template <int KT, int KV>
__global__ __launch_bounds__(256) void boot_bce_bwd_kernel(const float* __restrict__ p,
                                                           const typename SegMask<KT>::type* __restrict__ t,
                                                           const typename SegMask<KV>::type* __restrict__ voi,
                                                           const float* __restrict__ state, const float* __restrict__ gout,
                                                           float smoothing, float* __restrict__ dp, int64_t n, int vecp,
                                                           int vect, int vecv, int vecd) {
    const float g = gout[0];
    const float inv_out = state[0], alpha = state[1], inv_w = state[2], inv_in = state[3];
    const bool inside = state[4] > 0.f;
    const float ca = (1.f - smoothing) * alpha * inv_w, cb = (1.f - smoothing) * (1.f - alpha) * inv_w;
    const float ch = smoothing * inv_in;
    float pv[SEG_UNROLL][4], tv[SEG_UNROLL][4], vv[SEG_UNROLL][4];
    int cnt[SEG_UNROLL];
    int64_t at[SEG_UNROLL];
    seg_load_groups(n, cnt, at, SegSrc(p, vecp, pv), SegSrc(t, vect, tv), SegSrc(voi, vecv, vv));
#pragma unroll
    for (int u = 0; u < SEG_UNROLL; ++u) {
        if (cnt[u] == 0) continue;
        float d[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (e >= cnt[u]) continue;
            const float pe = pv[u][e], te = tv[u][e], ve = vv[u][e];
            const float pt = pe * te + (1.f - pe) * (1.f - te);
            const float dnll = (pt >= LEPS && pt <= 1.f - LEPS) ? (1.f - 2.f * te) / pt : 0.f;     // d pt / d p = 2 t - 1
            float v = 0.f;
            if (ve < LEPS) v = inv_out * dnll;
            if (inside && ve > 0.f) {
                const bool up = pe > 0.5f;
                const float ph = up ? pe : 1.f - pe;
                const float dh = (ph >= LEPS && ph <= 1.f - LEPS) ? (up ? -1.f : 1.f) / ph : 0.f;
                v += (ca * te + cb * (1.f - te)) * dnll + ch * dh;
            }
            d[e] = __fmul_rn(g, v);
        }
        seg_store4(dp, at[u], vecd != 0, cnt[u], d);
    }
}

template <int KT>
__global__ __launch_bounds__(256) void bce_smooth_partial_kernel(const float* __restrict__ p,
                                                                 const typename SegMask<KT>::type* __restrict__ t,
                                                                 double* __restrict__ part, int64_t n, int vecp, int vect) {
    __shared__ double red[SMOOTH_NSUM][4];
    float pv[SEG_UNROLL][4], tv[SEG_UNROLL][4];
    int cnt[SEG_UNROLL];
    int64_t at[SEG_UNROLL];
    seg_load_groups(n, cnt, at, SegSrc(p, vecp, pv), SegSrc(t, vect, tv));
    double acc[SMOOTH_NSUM] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int u = 0; u < SEG_UNROLL; ++u) {
        float s[SMOOTH_NSUM] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (e >= cnt[u]) continue;
            const float te = tv[u][e];
            const float pc = fminf(fmaxf(pv[u][e], SEPS), 1.f - SEPS);
            s[0] += te;
            s[1] += te * logf(pc);
            s[2] += (1.f - te) * logf(1.f - pc);
        }
#pragma unroll
        for (int q = 0; q < SMOOTH_NSUM; ++q) acc[q] += s[q];
    }
    block_partials<SMOOTH_NSUM>(acc, red, part + (size_t)blockIdx.x * SMOOTH_NSUM);
}

// tot (8 doubles): T, P1, P2.  state: [0] alpha, [1] 1 / sum w.
__global__ __launch_bounds__(256) void bce_smooth_finish_kernel(const double* __restrict__ part, int64_t nblk, int64_t n,
                                                                double smooth, double* __restrict__ tot_out,
                                                                float* __restrict__ out, float* __restrict__ state) {
    __shared__ double red[SMOOTH_NSUM][4];
    double tot[SMOOTH_NSUM];
    seg_total<SMOOTH_NSUM>(part, nblk, red, tot);
    if (threadIdx.x != 0) return;
    const double T = tot[0];
    double alpha = 1.0 - T / (double)n;
    alpha = alpha < 0.3 ? 0.3 : (alpha > 0.7 ? 0.7 : alpha);
    const double inv_w = 1.0 / (alpha * T + (1.0 - alpha) * ((double)n - T));
    out[0] = (float)(-smooth * (alpha * tot[1] + (1.0 - alpha) * tot[2]) * inv_w);
#pragma unroll
    for (int q = 0; q < SEG_TOTALS; ++q) tot_out[q] = q < SMOOTH_NSUM ? tot[q] : 0.0;
    state[0] = (float)alpha; state[1] = (float)inv_w;
#pragma unroll
    for (int q = 2; q < SEG_STATE; ++q) state[q] = 0.f;
}

template <int KT>
__global__ __launch_bounds__(256) void bce_smooth_bwd_kernel(const float* __restrict__ p,
                                                             const typename SegMask<KT>::type* __restrict__ t,
                                                             const float* __restrict__ state, const float* __restrict__ gout,
                                                             float smooth, float* __restrict__ dp, int64_t n, int vecp,
                                                             int vect, int vecd) {
    const float g = gout[0];
    const float alpha = state[0];
    const float c = -smooth * state[1];
    float pv[SEG_UNROLL][4], tv[SEG_UNROLL][4];
    int cnt[SEG_UNROLL];
    int64_t at[SEG_UNROLL];
    seg_load_groups(n, cnt, at, SegSrc(p, vecp, pv), SegSrc(t, vect, tv));
#pragma unroll
    for (int u = 0; u < SEG_UNROLL; ++u) {
        if (cnt[u] == 0) continue;
        float d[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (e >= cnt[u]) continue;
            const float pe = pv[u][e], te = tv[u][e];
            float v = 0.f;
            if (pe >= SEPS && pe <= 1.f - SEPS)         // pe is its own clamped value here
                v = c * (alpha * te + (1.f - alpha) * (1.f - te)) * (te / pe - (1.f - te) / (1.f - pe));
            d[e] = __fmul_rn(g, v);
        }
        seg_store4(dp, at[u], vecd != 0, cnt[u], d);
    }
}

static inline int64_t seg_blocks(int64_t n) { return cdiv64(n, SEG_CHUNK); }
static inline bool seg_kind_ok(int kind) { return kind == DRAM_SEG_MASK_U8 || kind == DRAM_SEG_MASK_F32; }
// whether a tensor of this kind may be read one group (four elements) per access
__host__ __device__ static inline int seg_vec(const void* b, int kind) {
    return ((uintptr_t)b & (kind == DRAM_SEG_MASK_U8 ? 3 : 15)) == 0;
}


// ---- SegOverlap: per-sample Tversky + focal loss on LOGITS with a target that is given (no reference counterpart) ---------
//   p = sigmoid(z),  -log p = softplus(-z),  -log(1 - p) = softplus(z);  1 - p is never formed by subtraction
//   per sample n, V = {voi set} (every voxel without a voi):  TP = sum_V p [t],  SP = sum_V p,  ST = sum_V [t],  M = |V|
//   TI = (TP + s) / ((1 - a - b) TP + a SP + b ST + s),   F = (1 / M) sum_V alpha_t (1 - p_t)^gamma (-log p_t)
//   out[0] = sum_n (1 - TI_n),  out[1] = (1 / N) sum_n F_n;  M = 0: TI = 1, F = 0
// With u = -z where t is set and u = z elsewhere (the logit of the WRONG class): -log p_t = softplus(u), -log(1 - p_t) =
// softplus(-u), so one voxel costs one expf (e = exp(-|z|), shared by the sigmoid and both softplus: softplus(x) = max(x, 0)
// + log1p(e)), one log1pf and one expf for the power.
// Forward: the layout of the BCE pair above, once per sample: grid (blocks of SEG_CHUNK elements, N), so a block never
// leaves its sample; the groups a lane owns are counted from the SAMPLE's first element and the per-tensor alignment flag
// is that of the sample's base, so any S and any base address give the same bits.  One fp64 tuple per block; one block
// then adds each sample's tuples (one wave per sample, sample_totals) and the per-sample terms in index order.
// Backward: one pass with the same ownership; per sample it reads the three coefficients the finish kernel left in `state`.
constexpr int OVL_NSUM = 5;            // per (sample, block): TP, SP, ST, M, sum of the focal terms
constexpr int OVL_STATE = 5;           // floats per sample: 1 - TI, F, then the backward's c_set, c_unset, 1 / (N M)

// One voxel: p q = d p / d z, p, the focal term f and d f / d z.  a1 = alpha, a0 = 1 - alpha.
__device__ __forceinline__ void ovl_voxel(float z, bool set, float a1, float a0, float gamma, float& pq, float& p, float& f,
                                          float& dfz) {
    float q;
    sigmoid_pq(z, p, q);
    pq = p * q;
    const float l = log1pf(expf(-fabsf(z)));             // softplus(-|z|)
    const float u = set ? -z : z;
    const float nlp = fmaxf(u, 0.f) + l;                 // -log p_t       = softplus(u)
    const float nlq = fmaxf(-u, 0.f) + l;                // -log(1 - p_t)  = softplus(-u)
    const float w = (set ? a1 : a0) * expf(-gamma * nlq);     // alpha_t (1 - p_t)^gamma
    f = w * nlp;
    // d f / d u = alpha_t (1 - p_t)^gamma (gamma p_t (-log p_t) + (1 - p_t)),  d u / d z = -+ 1
    const float dfu = w * (gamma * (set ? p : q) * nlp + (set ? q : p));
    dfz = set ? -dfu : dfu;
}

// KV and voi are not used where HV is false (no volume of interest: every voxel counts)
template <int KT, int KV, bool HV>
__global__ __launch_bounds__(256) void seg_overlap_partial_kernel(const float* __restrict__ z,
                                                                  const typename SegMask<KT>::type* __restrict__ t,
                                                                  const typename SegMask<KV>::type* __restrict__ voi,
                                                                  double* __restrict__ part, int64_t S, float a1, float a0,
                                                                  float gamma) {
    __shared__ double red[OVL_NSUM][4];
    const int64_t base = (int64_t)blockIdx.y * S;
    z += base; t += base; voi += base;
    float zv[SEG_UNROLL][4], tv[SEG_UNROLL][4], vv[SEG_UNROLL][4];
    int cnt[SEG_UNROLL];
    int64_t at[SEG_UNROLL];
    if constexpr (HV)
        seg_load_groups(S, cnt, at, SegSrc(z, seg_vec(z, DRAM_SEG_MASK_F32), zv), SegSrc(t, seg_vec(t, KT), tv),
                        SegSrc(voi, seg_vec(voi, KV), vv));
    else
        seg_load_groups(S, cnt, at, SegSrc(z, seg_vec(z, DRAM_SEG_MASK_F32), zv), SegSrc(t, seg_vec(t, KT), tv));
    double acc[OVL_NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int u = 0; u < SEG_UNROLL; ++u) {
        float s[OVL_NSUM] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (e >= cnt[u]) continue;
            if constexpr (HV)
                if (vv[u][e] == 0.f) continue;
            const bool set = tv[u][e] != 0.f;
            float pq, p, f, dfz;
            ovl_voxel(zv[u][e], set, a1, a0, gamma, pq, p, f, dfz);
            s[0] += set ? p : 0.f;
            s[1] += p;
            s[2] += set ? 1.f : 0.f;
            s[3] += 1.f;
            s[4] += f;
        }
#pragma unroll
        for (int q = 0; q < OVL_NSUM; ++q) acc[q] += s[q];
    }
    block_partials<OVL_NSUM>(acc, red, part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * OVL_NSUM);
}

// tot (SEG_TOTALS doubles per sample): TP, SP, ST, M, the focal sum, 1 - TI, F, 0.  state: OVL_STATE floats per sample.
// 1 - TI = (a (SP - TP) + b (ST - TP)) / denominator: the difference of the two, formed without the cancellation near TI = 1.
__global__ __launch_bounds__(256) void seg_overlap_finish_kernel(const double* __restrict__ part, int N, int nblk, double a,
                                                                 double b, double smooth, double* __restrict__ tot,
                                                                 float* __restrict__ out, float* __restrict__ state) {
    __shared__ double red[2][4];
    for (int n = threadIdx.x >> 6; n < N; n += 4) {
        double v[OVL_NSUM];
        sample_totals<OVL_NSUM>(part, n, nblk, v);
        if ((threadIdx.x & 63) != 0) continue;
        const double TP = v[0], SP = v[1], ST = v[2], M = v[3];
        const double num = TP + smooth, den = (1.0 - a - b) * TP + a * SP + b * ST + smooth;      // den >= num > 0
        const bool any = M > 0.0;
        const double loss = (a * (SP - TP) + b * (ST - TP)) / den, F = any ? v[4] / M : 0.0;
        double* o = tot + (size_t)n * SEG_TOTALS;
#pragma unroll
        for (int q = 0; q < OVL_NSUM; ++q) o[q] = v[q];
        o[5] = loss; o[6] = F; o[7] = 0.0;
        float* c = state + (size_t)n * OVL_STATE;
        c[0] = (float)loss; c[1] = (float)F;
        c[2] = (float)(-(den - num * (1.0 - b)) / (den * den));       // d (1 - TI) / d TP + d (1 - TI) / d SP: t set
        c[3] = (float)(num * a / (den * den));                        // d (1 - TI) / d SP: t not set
        c[4] = any ? (float)(1.0 / ((double)N * M)) : 0.f;
    }
    __syncthreads();
    double s[2] = {0.0, 0.0}, r[2];
    for (int n = threadIdx.x; n < N; n += 256) {
        s[0] += tot[(size_t)n * SEG_TOTALS + 5];
        s[1] += tot[(size_t)n * SEG_TOTALS + 6];
    }
    block_totals<2>(s, red, r);
    if (threadIdx.x == 0) { out[0] = (float)r[0]; out[1] = (float)(r[1] / (double)N); }
}

// dz = gout[0] d out[0] / dz + gout[1] d out[1] / dz: each product with gout last (one rounding each), then one addition;
// exactly +0 outside the volume of interest.
template <int KT, int KV, bool HV>
__global__ __launch_bounds__(256) void seg_overlap_bwd_kernel(const float* __restrict__ z,
                                                              const typename SegMask<KT>::type* __restrict__ t,
                                                              const typename SegMask<KV>::type* __restrict__ voi,
                                                              const float* __restrict__ state, const float* __restrict__ gout,
                                                              float* __restrict__ dz, int64_t S, float a1, float a0,
                                                              float gamma) {
    const int64_t base = (int64_t)blockIdx.y * S;
    z += base; t += base; voi += base; dz += base;
    const float g0 = gout[0], g1 = gout[1];
    const float* c = state + (size_t)blockIdx.y * OVL_STATE;
    const float cset = c[2], cunset = c[3], cf = c[4];
    float zv[SEG_UNROLL][4], tv[SEG_UNROLL][4], vv[SEG_UNROLL][4];
    int cnt[SEG_UNROLL];
    int64_t at[SEG_UNROLL];
    if constexpr (HV)
        seg_load_groups(S, cnt, at, SegSrc(z, seg_vec(z, DRAM_SEG_MASK_F32), zv), SegSrc(t, seg_vec(t, KT), tv),
                        SegSrc(voi, seg_vec(voi, KV), vv));
    else
        seg_load_groups(S, cnt, at, SegSrc(z, seg_vec(z, DRAM_SEG_MASK_F32), zv), SegSrc(t, seg_vec(t, KT), tv));
    const bool vecd = seg_vec(dz, DRAM_SEG_MASK_F32) != 0;
#pragma unroll
    for (int u = 0; u < SEG_UNROLL; ++u) {
        if (cnt[u] == 0) continue;
        float d[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (e >= cnt[u]) continue;
            if constexpr (HV)
                if (vv[u][e] == 0.f) continue;
            const bool set = tv[u][e] != 0.f;
            float pq, p, f, dfz;
            ovl_voxel(zv[u][e], set, a1, a0, gamma, pq, p, f, dfz);
            {
#pragma clang fp contract(off)         // two rounded products, then their sum: no fma may merge a product into the sum
                const float d0 = g0 * (pq * (set ? cset : cunset)), d1 = g1 * (cf * dfz);
                d[e] = d0 + d1;
            }
        }
        seg_store4(dz, at[u], vecd, cnt[u], d);
    }
}


// ---- regression targets of a batch (IntRegLoss.get_labels, dram/metrics.py:122-138; weight 172-174; keep 326-327) --------
//   ratio_n   = fp32( sum_v lesion m ) / fp32( sum_v m )                  one fp32 division (the lesion-ratio upper bound)
//   [lb, ub]  = [max(0, ratio - bw), min(1, ratio + bw)]                  in fp64, as the host loop's Python floats
//   band      = [max(c_lb, lb), min(c_ub, ub)], (c_lb, c_ub) the ratio interval of the sample's CT severity score;
//               where the two do not overlap: [lb, ub] if it lies below the class interval, the class interval if above
//   targets_n = band rounded once to fp32,  weight_n = clamp(freq[ctss_n], 0.2, 0.8),  keep_n = ctss_n > 0
// One pass over the two masks (8 B/voxel, stream_packs), per step the products of a lane in fp32 (at most 16 of them: exact
// for 0/1 masks), steps and lanes in fp64, one fp64 partial pair per block; one wave per sample then adds the partials and
// its lane 0 does the band.
// An empty lobe (0/0) gives NaN targets for that sample, a score outside 0..5 NaN targets and a NaN weight.
constexpr int TGT_NSUM = 2;            // per (sample, block): sum of lesion * lobe, sum of lobe
struct TargetsArgs {
    float freq[6];
    double band_width;
};

template <int V>
__global__ __launch_bounds__(256) void targets_partial_kernel(const float* __restrict__ lobes, const float* __restrict__ lesions,
                                                              double* __restrict__ part, int64_t S, int nblk) {
    __shared__ double red[TGT_NSUM][4];
    const int n = blockIdx.y;
    double acc[TGT_NSUM] = {0.0, 0.0};
    stream_packs<V>(lobes + (int64_t)n * S, lesions + (int64_t)n * S, S, nblk, [&](const PackStep<V>& st) {
        float sl = 0.f, sm = 0.f;
        st.each([&](int, float m, float l) {
            sl += __fmul_rn(l, m);
            sm += m;
        });
        acc[0] += sl; acc[1] += sm;
    });
    block_partials<TGT_NSUM>(acc, red, part + ((size_t)n * nblk + blockIdx.x) * TGT_NSUM);
}

__global__ __launch_bounds__(256) void targets_finalize_kernel(const double* __restrict__ part, const int* __restrict__ ctss,
                                                               TargetsArgs a, int N, int nblk, float* __restrict__ targets,
                                                               float* __restrict__ weight, float* __restrict__ keep) {
    // IntRegLoss.ctss_ratio_map (metrics.py:76-83)
    const double c_lo[6] = {0.0, 0.001, 0.01, 0.05, 0.35, 0.5}, c_hi[6] = {0.001, 0.01, 0.05, 0.35, 0.5, 1.00001};
    for (int n = threadIdx.x >> 6; n < N; n += 4) {
        double s[TGT_NSUM];
        sample_totals<TGT_NSUM>(part, n, nblk, s);
        if ((threadIdx.x & 63) != 0) continue;
        const int c = ctss[n];
        const bool known = c >= 0 && c <= 5;
        const float ratio = __fdiv_rn((float)s[0], (float)s[1]);
        const float nan = __builtin_nanf("");
        float lo = nan, hi = nan;
        if (known && ratio == ratio) {
            const double lp = (double)ratio;
            const double lb = (lp - a.band_width) > 0.0 ? lp - a.band_width : 0.0;
            const double ub = (lp + a.band_width) < 1.0 ? lp + a.band_width : 1.0;
            double b0 = lb > c_lo[c] ? lb : c_lo[c], b1 = ub < c_hi[c] ? ub : c_hi[c];
            if (b1 < b0) {
                if (ub <= c_lo[c]) { b0 = lb; b1 = ub; }
                else { b0 = c_lo[c]; b1 = c_hi[c]; }     // lb >= c_hi: the third case cannot occur (lb <= ub, c_lo < c_hi)
            }
            lo = (float)b0; hi = (float)b1;
        }
        targets[2 * n] = lo;
        targets[2 * n + 1] = hi;
        const float f = known ? a.freq[c] : nan;
        weight[n] = f != f ? f : fminf(fmaxf(f, 0.2f), 0.8f);
        keep[n] = c > 0 ? 1.f : 0.f;
    }
}

}  // namespace dram

using namespace dram;

// ---- C entry points --------------------------------------------------------------------------------------------------------
// Checks the entry points share (`who` is a string literal).  Every check comes before the first launch.
static inline bool rows_ok(int N, int64_t S) { return N > 0 && N <= 65535 && S > 0; }      // one grid.y row per sample
#define LOSS_REQUIRE_WS(who, ws, align, have, need)                                                                 \
    do {                                                                                                            \
        DRAM_REQUIRE(((uintptr_t)(ws) & ((align) - 1)) == 0, who ": workspace must be " #align "-byte aligned");    \
        if ((have) < (need)) {                                                                                      \
            set_error(who ": workspace too small");                                                                 \
            return DRAM_EWS;                                                                                        \
        }                                                                                                           \
    } while (0)

// launch(Int<4>) or launch(Int<1>): the instantiation of a stream_packs kernel
template <int K> using Int = std::integral_constant<int, K>;
template <class F> static inline void with_pack_width(bool v4, F&& launch) {
    if (v4) launch(Int<4>());
    else launch(Int<1>());
}
// launch(Int<KIND>, typed pointer): the instantiation of a segmentation kernel for one mask; nests for two masks
template <class F> static inline void with_mask(const void* m, int kind, F&& launch) {
    if (kind == DRAM_SEG_MASK_U8) launch(Int<DRAM_SEG_MASK_U8>(), (const uint8_t*)m);
    else launch(Int<DRAM_SEG_MASK_F32>(), (const float*)m);
}

extern "C" size_t dram_intreg_loss_ws_bytes(int N, int64_t S) {
    if (N <= 0 || S <= 0) return 0;
    return align_up((size_t)N * loss_chunks(S) * NSUM * sizeof(float), 256) + (size_t)N * NSUM * sizeof(double);
}

extern "C" int dram_intreg_loss_state_floats(int N) { return 4 + 2 * (N > 0 ? N : 0); }

extern "C" int dram_intreg_loss_fwd(const float* dense, const float* refined, const float* lobes, const float* lesions,
                                    const float* keep, const float* targets, const float* weight, float smoothing,
                                    float* out, float* state, void* ws, size_t ws_bytes, int N, int64_t S, void* stream) {
    if (!refined) refined = dense;
    DRAM_REQUIRE(dense && lobes && lesions && keep && targets && weight && out && state && ws, "intreg_loss_fwd: null pointer");
    DRAM_REQUIRE(rows_ok(N, S), "intreg_loss_fwd: bad dimensions");
    LOSS_REQUIRE_WS("intreg_loss_fwd", ws, 8, ws_bytes, dram_intreg_loss_ws_bytes(N, S));      // fp64 sums at a multiple of 256 bytes
    hipStream_t st = (hipStream_t)stream;
    const int nch = loss_chunks(S);
    hipLaunchKernelGGL(loss_partial_kernel, dim3(nch, N), dim3(256), 0, st, dense, refined, lobes, lesions, keep, (float*)ws, S, nch);
    double* ssum = (double*)((char*)ws + align_up((size_t)N * nch * NSUM * sizeof(float), 256));
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(256), 0, st, (const float*)ws, ssum, targets, weight, smoothing, N, nch, out, state);
    return check_launch("intreg_loss_fwd");
}

extern "C" int dram_intreg_loss_bwd(const float* dense, const float* refined, const float* lobes, const float* lesions,
                                    const float* keep, const float* targets, const float* weight, const float* state,
                                    const float* gout, float smoothing, float* ddense, float* drefined, int N, int64_t S,
                                    void* stream) {
    if (!refined || refined == dense) { refined = dense; drefined = nullptr; }
    else DRAM_REQUIRE(drefined, "intreg_loss_bwd: drefined is required when refined differs from dense");
    DRAM_REQUIRE(dense && lobes && lesions && keep && targets && weight && state && gout && ddense, "intreg_loss_bwd: null pointer");
    DRAM_REQUIRE(rows_ok(N, S), "intreg_loss_bwd: bad dimensions");
    const unsigned gx = (unsigned)(cdiv64(S, 256 * 8) < 4096 ? cdiv64(S, 256 * 8) : 4096);
    hipLaunchKernelGGL(loss_bwd_kernel, dim3(gx, N), dim3(256), 0, (hipStream_t)stream, dense, refined, lobes, lesions, keep,
                       targets, weight, state, gout, smoothing, ddense, drefined, S);
    return check_launch("intreg_loss_bwd");
}

extern "C" size_t dram_intreg_enc_loss_ws_bytes(int N, int64_t S) {
    if (N <= 0 || S <= 0) return 0;
    return ((size_t)N * enc_blocks_max(N, S) + (size_t)N) * ENC_NSUM * sizeof(double);
}

extern "C" int dram_intreg_enc_loss_state_floats(int N) { return 2 * (N > 0 ? N : 0); }

extern "C" int dram_intreg_enc_loss_fwd(const float* dense, const float* lobes, const float* targets, const float* weight,
                                        float* out, float* state, void* ws, size_t ws_bytes, int N, int64_t S,
                                        void* stream) {
    DRAM_REQUIRE(dense && lobes && targets && weight && out && state && ws, "intreg_enc_loss_fwd: null pointer");
    DRAM_REQUIRE(rows_ok(N, S), "intreg_enc_loss_fwd: bad dimensions");
    LOSS_REQUIRE_WS("intreg_enc_loss_fwd", ws, 8, ws_bytes, dram_intreg_enc_loss_ws_bytes(N, S));
    hipStream_t st = (hipStream_t)stream;
    const bool v4 = enc_vec4(S, dense, lobes);
    const int nblk = enc_blocks(N, S, v4 ? 4 : 1);
    double* part = (double*)ws;
    double* ssum = part + (size_t)N * nblk * ENC_NSUM;
    with_pack_width(v4, [&](auto V) {
        hipLaunchKernelGGL(enc_partial_kernel<V.value>, dim3(nblk, N), dim3(256), 0, st, dense, lobes, part, S, nblk);
    });
    hipLaunchKernelGGL(enc_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)part, ssum, targets, weight, N, S, nblk,
                       out, state);
    return check_launch("intreg_enc_loss_fwd");
}

extern "C" int dram_intreg_enc_loss_bwd(const float* dense, const float* lobes, const float* targets, const float* weight,
                                        const float* state, const float* gout, float* ddense, int N, int64_t S,
                                        void* stream) {
    DRAM_REQUIRE(dense && lobes && targets && weight && state && gout && ddense, "intreg_enc_loss_bwd: null pointer");
    DRAM_REQUIRE(rows_ok(N, S), "intreg_enc_loss_bwd: bad dimensions");
    const bool v4 = enc_vec4(S, dense, lobes, ddense);
    const int nblk = enc_blocks(N, S, v4 ? 4 : 1);
    with_pack_width(v4, [&](auto V) {
        hipLaunchKernelGGL(enc_bwd_kernel<V.value>, dim3(nblk, N), dim3(256), 0, (hipStream_t)stream, dense, lobes, targets,
                           weight, state, gout, ddense, N, S);
    });
    return check_launch("intreg_enc_loss_bwd");
}

extern "C" int dram_sigmoid_fwd(const float* x, float* y, int64_t n, void* stream) {
    DRAM_REQUIRE(x && y && n > 0, "sigmoid_fwd: bad arguments");
    const unsigned grid = (unsigned)(cdiv64(n, 256) < 8192 ? cdiv64(n, 256) : 8192);
    hipLaunchKernelGGL(sigmoid_fwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, y, n);
    return check_launch("sigmoid_fwd");
}

extern "C" int dram_sigmoid_bwd(const float* dy, const float* x, float* dx, int64_t n, void* stream) {
    DRAM_REQUIRE(dy && x && dx && n > 0, "sigmoid_bwd: bad arguments");
    const unsigned grid = (unsigned)(cdiv64(n, 256) < 8192 ? cdiv64(n, 256) : 8192);
    hipLaunchKernelGGL(sigmoid_bwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, dy, x, dx, n);
    return check_launch("sigmoid_bwd");
}

extern "C" size_t dram_masked_smooth_l1_ws_bytes(int N, int C, int64_t S) {
    if (N <= 0 || C <= 0 || S <= 0) return 0;
    return (size_t)N * C * loss_chunks(S) * 2 * sizeof(float);
}

extern "C" int dram_masked_smooth_l1_fwd(const float* a, const float* b, const float* mask, float* out, void* ws,
                                         size_t ws_bytes, int N, int C, int64_t S, void* stream) {
    DRAM_REQUIRE(a && b && mask && out && ws, "masked_smooth_l1_fwd: null pointer");
    DRAM_REQUIRE(N > 0 && C > 0 && S > 0 && (int64_t)N * C <= 65535, "masked_smooth_l1_fwd: bad dimensions");
    LOSS_REQUIRE_WS("masked_smooth_l1_fwd", ws, 4, ws_bytes, dram_masked_smooth_l1_ws_bytes(N, C, S));
    hipStream_t st = (hipStream_t)stream;
    const int nch = loss_chunks(S);
    hipLaunchKernelGGL(masked_smooth_l1_partial_kernel, dim3(nch, N * C), dim3(256), 0, st, a, b, mask, (float*)ws, C, S, nch);
    hipLaunchKernelGGL(masked_smooth_l1_finalize_kernel, dim3(1), dim3(256), 0, st, (const float*)ws, (int64_t)N * C * nch, out);
    return check_launch("masked_smooth_l1_fwd");
}

extern "C" int dram_masked_smooth_l1_bwd(const float* a, const float* b, const float* mask, const float* out,
                                         const float* gout, float* da, float* db, int N, int C, int64_t S, void* stream) {
    DRAM_REQUIRE(a && b && mask && out && gout && (da || db), "masked_smooth_l1_bwd: null pointer");
    DRAM_REQUIRE(N > 0 && C > 0 && S > 0 && (int64_t)N * C <= 65535, "masked_smooth_l1_bwd: bad dimensions");
    const unsigned gx = (unsigned)(cdiv64(S, 256) < 2048 ? cdiv64(S, 256) : 2048);
    hipLaunchKernelGGL(masked_smooth_l1_bwd_kernel, dim3(gx, N * C), dim3(256), 0, (hipStream_t)stream, a, b, mask, out, gout,
                       da, db, C, S);
    return check_launch("masked_smooth_l1_bwd");
}

extern "C" size_t dram_seg_loss_ws_bytes(int64_t n) {
    if (n <= 0) return 0;
    return ((size_t)SEG_TOTALS + (size_t)seg_blocks(n) * BOOT_NSUM) * sizeof(double);
}

extern "C" int dram_seg_loss_state_floats(void) { return SEG_STATE; }

extern "C" int dram_seg_loss_chunk(void) { return SEG_CHUNK; }

#define SEG_REQUIRE_COMMON(who, n)                                                                   \
    DRAM_REQUIRE((n) >= 0, who ": negative element count");                                          \
    DRAM_REQUIRE((n) <= ((int64_t)1 << 40), who ": more than 2^40 elements") /* one block per 4096 elements, grid.x < 2^31 */

extern "C" int dram_boot_bce_fwd(const float* p, const void* t, const void* voi, int t_kind, int voi_kind, int64_t n,
                                 double smoothing, float* out, float* state, void* ws, size_t ws_bytes, void* stream) {
    SEG_REQUIRE_COMMON("boot_bce_fwd", n);
    DRAM_REQUIRE(seg_kind_ok(t_kind) && seg_kind_ok(voi_kind), "boot_bce_fwd: mask kind must be 0 (uint8) or 2 (float32)");
    if (n == 0) return DRAM_OK;
    DRAM_REQUIRE(p && t && voi && out && state && ws, "boot_bce_fwd: null pointer");
    LOSS_REQUIRE_WS("boot_bce_fwd", ws, 8, ws_bytes, dram_seg_loss_ws_bytes(n));
    hipStream_t st = (hipStream_t)stream;
    const int64_t nblk = seg_blocks(n);
    double* tot = (double*)ws;
    double* part = tot + SEG_TOTALS;
    with_mask(t, t_kind, [&](auto KT, auto tp) {
        with_mask(voi, voi_kind, [&](auto KV, auto vp) {
            hipLaunchKernelGGL((boot_bce_partial_kernel<KT.value, KV.value>), dim3((unsigned)nblk), dim3(256), 0, st, p, tp, vp, part,
                               n, seg_vec(p, DRAM_SEG_MASK_F32), seg_vec(t, t_kind), seg_vec(voi, voi_kind));
        });
    });
    hipLaunchKernelGGL(boot_bce_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)part, nblk, smoothing, tot, out, state);
    return check_launch("boot_bce_fwd");
}

extern "C" int dram_boot_bce_bwd(const float* p, const void* t, const void* voi, int t_kind, int voi_kind, int64_t n,
                                 double smoothing, const float* state, const float* gout, float* dp, void* stream) {
    SEG_REQUIRE_COMMON("boot_bce_bwd", n);
    DRAM_REQUIRE(seg_kind_ok(t_kind) && seg_kind_ok(voi_kind), "boot_bce_bwd: mask kind must be 0 (uint8) or 2 (float32)");
    if (n == 0) return DRAM_OK;
    DRAM_REQUIRE(p && t && voi && state && gout && dp, "boot_bce_bwd: null pointer");
    with_mask(t, t_kind, [&](auto KT, auto tp) {
        with_mask(voi, voi_kind, [&](auto KV, auto vp) {
            hipLaunchKernelGGL((boot_bce_bwd_kernel<KT.value, KV.value>), dim3((unsigned)seg_blocks(n)), dim3(256), 0,
                               (hipStream_t)stream, p, tp, vp, state, gout, (float)smoothing, dp, n, seg_vec(p, DRAM_SEG_MASK_F32),
                               seg_vec(t, t_kind), seg_vec(voi, voi_kind), seg_vec(dp, DRAM_SEG_MASK_F32));
        });
    });
    return check_launch("boot_bce_bwd");
}

extern "C" int dram_bce_smooth_fwd(const float* p, const void* t, int t_kind, int64_t n, double smooth, float* out,
                                   float* state, void* ws, size_t ws_bytes, void* stream) {
    SEG_REQUIRE_COMMON("bce_smooth_fwd", n);
    DRAM_REQUIRE(seg_kind_ok(t_kind), "bce_smooth_fwd: target kind must be 0 (uint8) or 2 (float32)");
    if (n == 0) return DRAM_OK;
    DRAM_REQUIRE(p && t && out && state && ws, "bce_smooth_fwd: null pointer");
    LOSS_REQUIRE_WS("bce_smooth_fwd", ws, 8, ws_bytes, dram_seg_loss_ws_bytes(n));
    hipStream_t st = (hipStream_t)stream;
    const int64_t nblk = seg_blocks(n);
    double* tot = (double*)ws;
    double* part = tot + SEG_TOTALS;
    with_mask(t, t_kind, [&](auto KT, auto tp) {
        hipLaunchKernelGGL(bce_smooth_partial_kernel<KT.value>, dim3((unsigned)nblk), dim3(256), 0, st, p, tp, part, n,
                           seg_vec(p, DRAM_SEG_MASK_F32), seg_vec(t, t_kind));
    });
    hipLaunchKernelGGL(bce_smooth_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)part, nblk, n, smooth, tot, out, state);
    return check_launch("bce_smooth_fwd");
}

extern "C" int dram_bce_smooth_bwd(const float* p, const void* t, int t_kind, int64_t n, double smooth, const float* state,
                                   const float* gout, float* dp, void* stream) {
    SEG_REQUIRE_COMMON("bce_smooth_bwd", n);
    DRAM_REQUIRE(seg_kind_ok(t_kind), "bce_smooth_bwd: target kind must be 0 (uint8) or 2 (float32)");
    if (n == 0) return DRAM_OK;
    DRAM_REQUIRE(p && t && state && gout && dp, "bce_smooth_bwd: null pointer");
    with_mask(t, t_kind, [&](auto KT, auto tp) {
        hipLaunchKernelGGL(bce_smooth_bwd_kernel<KT.value>, dim3((unsigned)seg_blocks(n)), dim3(256), 0, (hipStream_t)stream, p, tp,
                           state, gout, (float)smooth, dp, n, seg_vec(p, DRAM_SEG_MASK_F32), seg_vec(t, t_kind),
                           seg_vec(dp, DRAM_SEG_MASK_F32));
    });
    return check_launch("bce_smooth_bwd");
}

extern "C" size_t dram_seg_overlap_ws_bytes(int N, int64_t S) {
    if (N <= 0 || S <= 0) return 0;
    return ((size_t)N * SEG_TOTALS + (size_t)N * seg_blocks(S) * OVL_NSUM) * sizeof(double);
}

extern "C" int dram_seg_overlap_state_floats(int N) { return OVL_STATE * (N > 0 ? N : 0); }

// launch(Int<KT>, Int<KV>, has-voi, typed t, typed voi): the instantiation of a SegOverlap kernel; without a voi the
// target stands in for the pointer nobody reads
template <class F> static inline void with_overlap_masks(const void* t, int t_kind, const void* voi, int voi_kind, F&& launch) {
    with_mask(t, t_kind, [&](auto KT, auto tp) {
        if (!voi) launch(KT, KT, std::false_type(), tp, tp);
        else with_mask(voi, voi_kind, [&](auto KV, auto vp) { launch(KT, KV, std::true_type(), tp, vp); });
    });
}

#define OVL_REQUIRE_COMMON(who)                                                                                          \
    DRAM_REQUIRE(N >= 0 && S >= 0, who ": negative dimension");                                                          \
    DRAM_REQUIRE(N <= 65535 && S <= ((int64_t)1 << 40), who ": more than 65535 samples or 2^40 elements per sample");    \
    DRAM_REQUIRE(seg_kind_ok(t_kind) && (!voi || seg_kind_ok(voi_kind)), who ": mask kind must be 0 (uint8) or 2 (float32)"); \
    DRAM_REQUIRE(alpha >= 0.0 && alpha <= 1.0, who ": alpha must lie in [0, 1]");                                       \
    DRAM_REQUIRE(gamma >= 0.0 && std::isfinite(gamma), who ": gamma must be finite and not negative")

extern "C" int dram_seg_overlap_fwd(const float* z, const void* t, const void* voi, int t_kind, int voi_kind, int N,
                                    int64_t S, double a, double b, double smooth, double alpha, double gamma, float* out,
                                    float* state, void* ws, size_t ws_bytes, void* stream) {
    OVL_REQUIRE_COMMON("seg_overlap_fwd");
    DRAM_REQUIRE(a >= 0.0 && b >= 0.0 && std::isfinite(a) && std::isfinite(b), "seg_overlap_fwd: a and b must be finite and not negative");
    DRAM_REQUIRE(smooth > 0.0 && std::isfinite(smooth), "seg_overlap_fwd: the smoothing term must be finite and positive");
    if (N == 0 || S == 0) return DRAM_OK;
    DRAM_REQUIRE(z && t && out && state && ws, "seg_overlap_fwd: null pointer");
    LOSS_REQUIRE_WS("seg_overlap_fwd", ws, 8, ws_bytes, dram_seg_overlap_ws_bytes(N, S));
    hipStream_t st = (hipStream_t)stream;
    const int nblk = (int)seg_blocks(S);
    double* tot = (double*)ws;
    double* part = tot + (size_t)N * SEG_TOTALS;
    with_overlap_masks(t, t_kind, voi, voi_kind, [&](auto KT, auto KV, auto HV, auto tp, auto vp) {
        hipLaunchKernelGGL((seg_overlap_partial_kernel<KT.value, KV.value, HV.value>), dim3(nblk, N), dim3(256), 0, st, z, tp, vp,
                           part, S, (float)alpha, (float)(1.0 - alpha), (float)gamma);
    });
    hipLaunchKernelGGL(seg_overlap_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)part, N, nblk, a, b, smooth, tot, out,
                       state);
    return check_launch("seg_overlap_fwd");
}

extern "C" int dram_seg_overlap_bwd(const float* z, const void* t, const void* voi, int t_kind, int voi_kind, int N,
                                    int64_t S, double alpha, double gamma, const float* state, const float* gout, float* dz,
                                    void* stream) {
    OVL_REQUIRE_COMMON("seg_overlap_bwd");
    if (N == 0 || S == 0) return DRAM_OK;
    DRAM_REQUIRE(z && t && state && gout && dz, "seg_overlap_bwd: null pointer");
    with_overlap_masks(t, t_kind, voi, voi_kind, [&](auto KT, auto KV, auto HV, auto tp, auto vp) {
        hipLaunchKernelGGL((seg_overlap_bwd_kernel<KT.value, KV.value, HV.value>), dim3((unsigned)seg_blocks(S), N), dim3(256), 0,
                           (hipStream_t)stream, z, tp, vp, state, gout, dz, S, (float)alpha, (float)(1.0 - alpha), (float)gamma);
    });
    return check_launch("seg_overlap_bwd");
}

extern "C" size_t dram_intreg_targets_ws_bytes(int N, int64_t S) {
    if (N <= 0 || S <= 0) return 0;
    return (size_t)N * enc_blocks_max(N, S) * TGT_NSUM * sizeof(double);
}

extern "C" int dram_intreg_targets(const float* lobes, const float* lesions, const int* ctss, const float* freq,
                                   double band_width, float* targets, float* weight, float* keep, void* ws,
                                   size_t ws_bytes, int N, int64_t S, void* stream) {
    DRAM_REQUIRE(lobes && lesions && ctss && freq && targets && weight && keep && ws, "intreg_targets: null pointer");
    DRAM_REQUIRE(rows_ok(N, S), "intreg_targets: bad dimensions");
    LOSS_REQUIRE_WS("intreg_targets", ws, 8, ws_bytes, dram_intreg_targets_ws_bytes(N, S));
    hipStream_t st = (hipStream_t)stream;
    TargetsArgs a;
    for (int k = 0; k < 6; ++k) a.freq[k] = freq[k];
    a.band_width = band_width;
    const bool v4 = enc_vec4(S, lobes, lesions);
    const int nblk = enc_blocks(N, S, v4 ? 4 : 1);
    double* part = (double*)ws;
    with_pack_width(v4, [&](auto V) {
        hipLaunchKernelGGL(targets_partial_kernel<V.value>, dim3(nblk, N), dim3(256), 0, st, lobes, lesions, part, S, nblk);
    });
    hipLaunchKernelGGL(targets_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)part, ctss, a, N, nblk, targets, weight,
                       keep);
    return check_launch("intreg_targets");
}
