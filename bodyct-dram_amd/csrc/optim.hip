// The optimiser update of the training step (st_dram_ref.py: torch.optim.Adam; the SGD-with-momentum, AdaBound and RAdam lines
// commented out beside it), gfx950: multi-tensor Adam / AdamW / SGD / RAdam / AdaBound, one launch per table of up to
// DRAM_OPTIM_TABLE_CAPACITY tensors.
//
// The table travels in the kernel arguments (no device buffer, no copy, nothing to keep alive; the gradient pointers change
// every step, so the host rebuilds it each step anyway).  The host gives every tensor cdiv(n, OCHUNK) consecutive blocks and
// records the first one; a block finds its tensor by bisecting those starts (wave-uniform, scalar loads of the arguments).
// A tensor whose pointers are all 16-byte aligned moves its whole groups of four as 16-byte accesses (span<true>) and its last
// n % 4 elements one by one (span<false>); a tensor with any misaligned pointer -- a gradient that is a view into a flat
// all-reduce bucket at an arbitrary offset -- takes span<false> throughout: one dword per lane, consecutive lanes on
// consecutive addresses.  Each element is read and written by exactly one lane: no atomics, no LDS, deterministic.
// HBM traffic per element: Adam, RAdam and AdaBound 16 B read + 12 B written (amsgrad / amsbound: +4 +4); SGD with momentum
// 12 B + 8 B.
//
// Every product, sum, quotient and root below is one IEEE fp32 operation (fmaf: one rounding for a*b+c); the count of
// roundings per quantity is what tests/optim_restatement.py bounds.
//
// Global-norm gradient clipping (torch.nn.utils.clip_grad_norm_) rides on the same table and block mapping:
//   grad_norm_kernel    one partial per block -- the fp64 sum of the block's exact squares (2-norm), or its max |g| with NaN kept
//                       (inf-norm) -- each written by exactly one block into its own slot: no atomics, deterministic;
//   grad_norm_finish    one block adds (or maxes) every partial in a fixed order and writes {total_norm, clip_coef};
//   optim_kernel        takes `gscale`, a device pointer to that clip_coef (NULL: no scaling), read once per block, and multiplies
//                       it into g before anything else: the gradients are read once and never written;
//   grad_scale_kernel   g *= gscale[0] in place, for the stand-alone clip_grad_norm_.
// Only the gradient pointer decides between the 16-byte and the one-dword instantiation in the two gradient-only kernels.
#include "common.h"

namespace dram {

constexpr int OCHUNK = 4096;   // elements per block: 256 lanes x 4 groups of 4

struct OptimEntry {            // 56 bytes
    float* p;
    const float* g;
    float* m;                  // Adam: exp_avg; SGD: momentum_buffer (NULL without momentum)
    float* v;                  // Adam: exp_avg_sq
    float* vmax;               // Adam with amsgrad, AdaBound with amsbound: max_exp_avg_sq, else NULL
    unsigned n, first_block;
    float s0, s1;              // Adam: lr / bc1, sqrt(bc2); SGD: s0 != 0 on the tensor's first step (buf = g');
                               // RAdam: the whole step factor, s1 != 0 when rectified; AdaBound: lr sqrt(bc2) / bc1
};
struct OptimTable {
    OptimEntry e[DRAM_OPTIM_TABLE_CAPACITY];
    int count;
};
static_assert(sizeof(OptimEntry) == 56, "OptimEntry layout");
static_assert(sizeof(OptimEntry) == sizeof(dram_optim_tensor), "the launch copies dram_optim_tensor field by field into this");
static_assert(sizeof(OptimTable) + 64 <= 4096, "table and scalars must fit a 4 KiB kernel-argument block");

struct AdamScalars {
    float beta1, omb1, beta2, omb2, eps, wd, decay;   // omb = 1 - beta; decay = 1 - lr * wd (AdamW)
    int decoupled, amsgrad, maximize;
};
struct SgdScalars {
    float lr, mu, omd, wd;                            // omd = 1 - dampening
    int nesterov, maximize;
};

struct AdamRule {
    AdamScalars a;
    float step_size, bc2_sqrt, gscale;
    bool has_vmax, scaled;                            // scaled, gscale: set by optim_kernel
    __device__ __forceinline__ void load(const OptimEntry& e) { step_size = e.s0; bc2_sqrt = e.s1; has_vmax = a.amsgrad != 0; }
    __device__ __forceinline__ bool reads_m() const { return true; }
    __device__ __forceinline__ bool uses_m() const { return true; }
    __device__ __forceinline__ bool uses_v() const { return true; }
    __device__ __forceinline__ bool uses_vmax() const { return has_vmax; }
    __device__ __forceinline__ void apply(float& p, float g, float& m, float& v, float& vmax) const {
        if (scaled) g = __fmul_rn(g, gscale);
        if (a.maximize) g = -g;
        if (a.decoupled) p = __fmul_rn(p, a.decay);
        else if (a.wd != 0.f) g = fmaf(a.wd, p, g);
        m = fmaf(a.beta1, m, __fmul_rn(a.omb1, g));
        v = fmaf(a.beta2, v, __fmul_rn(a.omb2, __fmul_rn(g, g)));
        float vuse = v;
        if (has_vmax) { vmax = fmaxf(vmax, v); vuse = vmax; }
        const float den = __fadd_rn(__fdiv_rn(__fsqrt_rn(vuse), bc2_sqrt), a.eps);
        p = fmaf(-step_size, __fdiv_rn(m, den), p);
    }
};

struct SgdRule {
    SgdScalars a;
    float gscale;
    bool first, has_buf, scaled;                      // scaled, gscale: set by optim_kernel
    __device__ __forceinline__ void load(const OptimEntry& e) { first = e.s0 != 0.f; has_buf = e.m != nullptr; }
    __device__ __forceinline__ bool reads_m() const { return has_buf && !first; }
    __device__ __forceinline__ bool uses_m() const { return has_buf; }
    __device__ __forceinline__ bool uses_v() const { return false; }
    __device__ __forceinline__ bool uses_vmax() const { return false; }
    __device__ __forceinline__ void apply(float& p, float g, float& m, float&, float&) const {
        if (scaled) g = __fmul_rn(g, gscale);
        if (a.maximize) g = -g;
        if (a.wd != 0.f) g = fmaf(a.wd, p, g);
        if (has_buf) {
            m = first ? g : fmaf(a.mu, m, __fmul_rn(a.omd, g));
            g = a.nesterov ? fmaf(a.mu, m, g) : m;
        }
        p = fmaf(-a.lr, g, p);
    }
};

// RAdam (torch.optim.RAdam; the RAdam line of st_dram_ref.py's OPTIMIZER block).  Whether a tensor is rectified depends on its
// step count alone, so the host decides and folds the whole step factor into s0; eps joins the RAW root, not Adam's
// sqrt(v) / sqrt(bc2).
struct RAdamScalars {
    float beta1, omb1, beta2, omb2, eps, wd, decay;   // as AdamScalars
    int decoupled, maximize;
};
struct RAdamRule {
    RAdamScalars a;
    float step, gscale;
    bool rect, scaled;                                // scaled, gscale: set by optim_kernel
    __device__ __forceinline__ void load(const OptimEntry& e) { step = e.s0; rect = e.s1 != 0.f; }
    __device__ __forceinline__ bool reads_m() const { return true; }
    __device__ __forceinline__ bool uses_m() const { return true; }
    __device__ __forceinline__ bool uses_v() const { return true; }
    __device__ __forceinline__ bool uses_vmax() const { return false; }
    __device__ __forceinline__ void apply(float& p, float g, float& m, float& v, float&) const {
        if (scaled) g = __fmul_rn(g, gscale);
        if (a.maximize) g = -g;
        if (a.decoupled) p = __fmul_rn(p, a.decay);
        else if (a.wd != 0.f) g = fmaf(a.wd, p, g);
        m = fmaf(a.beta1, m, __fmul_rn(a.omb1, g));
        v = fmaf(a.beta2, v, __fmul_rn(a.omb2, __fmul_rn(g, g)));
        const float upd = rect ? __fdiv_rn(m, __fadd_rn(__fsqrt_rn(v), a.eps)) : m;
        p = fmaf(-step, upd, p);
    }
};

// AdaBound (Luo et al. 2019; the adabound.AdaBound line of st_dram_ref.py's OPTIMIZER block).  lower and upper depend on the
// step count and travel as launch scalars: the host issues one launch per distinct step count.  The clamp is written as two
// comparisons so that a NaN quotient stays a NaN, as torch.clamp leaves it.
struct AdaBoundScalars {
    float beta1, omb1, beta2, omb2, eps, wd, lower, upper;
    int amsbound;
};
struct AdaBoundRule {
    AdaBoundScalars a;
    float step_size, gscale;
    bool has_vmax, scaled;                            // scaled, gscale: set by optim_kernel
    __device__ __forceinline__ void load(const OptimEntry& e) { step_size = e.s0; has_vmax = a.amsbound != 0; }
    __device__ __forceinline__ bool reads_m() const { return true; }
    __device__ __forceinline__ bool uses_m() const { return true; }
    __device__ __forceinline__ bool uses_v() const { return true; }
    __device__ __forceinline__ bool uses_vmax() const { return has_vmax; }
    __device__ __forceinline__ void apply(float& p, float g, float& m, float& v, float& vmax) const {
        if (scaled) g = __fmul_rn(g, gscale);
        if (a.wd != 0.f) g = fmaf(a.wd, p, g);
        m = fmaf(a.beta1, m, __fmul_rn(a.omb1, g));
        v = fmaf(a.beta2, v, __fmul_rn(a.omb2, __fmul_rn(g, g)));
        float vuse = v;
        if (has_vmax) { vmax = fmaxf(vmax, v); vuse = vmax; }
        float rate = __fdiv_rn(step_size, __fadd_rn(__fsqrt_rn(vuse), a.eps));
        rate = rate < a.lower ? a.lower : rate;
        rate = rate > a.upper ? a.upper : rate;
        p = fmaf(-rate, m, p);
    }
};

template <bool VEC>
__device__ __forceinline__ void optim_ld(const float* a, unsigned i, float* o) {
    if (VEC) {
        const float4 q = *reinterpret_cast<const float4*>(a + i);
        o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
    } else {
        o[0] = a[i];
    }
}
template <bool VEC>
__device__ __forceinline__ void optim_st(float* a, unsigned i, const float* o) {
    if (VEC) *reinterpret_cast<float4*>(a + i) = make_float4(o[0], o[1], o[2], o[3]);
    else a[i] = o[0];
}

// Elements [beg, end) of one tensor; VEC: beg and end - beg are multiples of 4 and every pointer is 16-byte aligned.
template <bool VEC, class Rule>
__device__ __forceinline__ void optim_span(const OptimEntry& e, const Rule& r, unsigned beg, unsigned end) {
    constexpr unsigned W = VEC ? 4 : 1;
    for (unsigned i = beg + threadIdx.x * W; i < end; i += 256 * W) {
        float p[W], g[W], m[W], v[W], x[W];
#pragma unroll
        for (unsigned k = 0; k < W; ++k) m[k] = v[k] = x[k] = 0.f;
        optim_ld<VEC>(e.p, i, p);
        optim_ld<VEC>(e.g, i, g);
        if (r.reads_m()) optim_ld<VEC>(e.m, i, m);
        if (r.uses_v()) optim_ld<VEC>(e.v, i, v);
        if (r.uses_vmax()) optim_ld<VEC>(e.vmax, i, x);
#pragma unroll
        for (unsigned k = 0; k < W; ++k) r.apply(p[k], g[k], m[k], v[k], x[k]);
        optim_st<VEC>(e.p, i, p);
        if (r.uses_m()) optim_st<VEC>(e.m, i, m);
        if (r.uses_v()) optim_st<VEC>(e.v, i, v);
        if (r.uses_vmax()) optim_st<VEC>(e.vmax, i, x);
    }
}

// The last tensor whose first block is <= this block (first_block is increasing, e[0].first_block == 0).
__device__ __forceinline__ int optim_find(const OptimTable& t) {
    int lo = 0, hi = t.count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (t.e[mid].first_block <= blockIdx.x) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// gscale: NULL, or the device scalar every gradient is multiplied by (the clip coefficient grad_norm_finish wrote).
template <class Rule, class Scalars>
__global__ __launch_bounds__(256) void optim_kernel(const OptimTable t, const Scalars s, const float* __restrict__ gscale) {
    const OptimEntry e = t.e[optim_find(t)];
    Rule r;
    r.a = s;
    r.scaled = gscale != nullptr;
    r.gscale = r.scaled ? gscale[0] : 1.f;                             // wave-uniform: one load per block
    r.load(e);
    const unsigned beg = (blockIdx.x - e.first_block) * OCHUNK;        // < n: the host gave this tensor cdiv(n, OCHUNK) blocks
    const unsigned end = e.n - beg < (unsigned)OCHUNK ? e.n : beg + OCHUNK;
    const uintptr_t bits = (uintptr_t)e.p | (uintptr_t)e.g | (uintptr_t)e.m | (uintptr_t)e.v | (uintptr_t)e.vmax;
    unsigned vend = beg;
    if ((bits & 15) == 0) {
        vend = beg + ((end - beg) & ~3u);
        optim_span<true>(e, r, beg, vend);
    }
    optim_span<false>(e, r, vend, end);
}

// ---- gradient norm, clip coefficient, in-place scale
// The 2-norm accumulates exact squares (the product of two fp32 numbers is exact in fp64) in fp64; the inf-norm keeps a NaN
// once it has met one, as torch.max does (fmaxf would drop it).
struct SumSq {
    static __device__ __forceinline__ double zero() { return 0.0; }
    static __device__ __forceinline__ double take(double a, float g) { return a + (double)g * (double)g; }
    static __device__ __forceinline__ double join(double a, double b) { return a + b; }
};
struct MaxAbs {
    static __device__ __forceinline__ double zero() { return 0.0; }
    static __device__ __forceinline__ double join(double a, double b) { return (b > a || b != b) ? b : a; }
    static __device__ __forceinline__ double take(double a, float g) { return join(a, (double)fabsf(g)); }
};

// Every lane's value joined over the 256 lanes of the block, in a fixed order; valid in thread 0.  red: 4 doubles of LDS.
template <class Op>
__device__ __forceinline__ double grad_block_join(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = Op::join(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return Op::join(Op::join(red[0], red[1]), Op::join(red[2], red[3]));
}

template <class Op>
__global__ __launch_bounds__(256) void grad_norm_kernel(const OptimTable t, double* __restrict__ partials) {
    __shared__ double red[4];
    const OptimEntry e = t.e[optim_find(t)];
    const unsigned beg = (blockIdx.x - e.first_block) * OCHUNK;
    const unsigned end = e.n - beg < (unsigned)OCHUNK ? e.n : beg + OCHUNK;
    double acc = Op::zero();
    unsigned vend = beg;
    if (((uintptr_t)e.g & 15) == 0) {
        vend = beg + ((end - beg) & ~3u);
        for (unsigned i = beg + threadIdx.x * 4; i < vend; i += 256 * 4) {
            float g[4];
            optim_ld<true>(e.g, i, g);
#pragma unroll
            for (int k = 0; k < 4; ++k) acc = Op::take(acc, g[k]);
        }
    }
    for (unsigned i = vend + threadIdx.x; i < end; i += 256) acc = Op::take(acc, e.g[i]);
    acc = grad_block_join<Op>(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

// out[0] = the norm, out[1] = min(1, max_norm / (norm + 1e-6)) evaluated in fp32 as torch.nn.utils.clip_grad_norm_ does, a NaN
// kept (c > 1 is false for it; fminf would drop it).
template <class Op, bool ROOT>
__global__ __launch_bounds__(256) void grad_norm_finish(const double* __restrict__ partials, long long n, float max_norm,
                                                        float* __restrict__ out) {
    __shared__ double red[4];
    double acc = Op::zero();
    for (long long i = threadIdx.x; i < n; i += 256) acc = Op::join(acc, partials[i]);
    acc = grad_block_join<Op>(acc, red);
    if (threadIdx.x == 0) {
        const float norm = (float)(ROOT ? sqrt(acc) : acc);
        float c = __fdiv_rn(max_norm, __fadd_rn(norm, 1e-6f));
        c = c > 1.f ? 1.f : c;
        out[0] = norm;
        out[1] = c;
    }
}

template <bool VEC>
__device__ __forceinline__ void grad_scale_span(float* g, float c, unsigned beg, unsigned end) {
    constexpr unsigned W = VEC ? 4 : 1;
    for (unsigned i = beg + threadIdx.x * W; i < end; i += 256 * W) {
        float x[W];
        optim_ld<VEC>(g, i, x);
#pragma unroll
        for (unsigned k = 0; k < W; ++k) x[k] = __fmul_rn(x[k], c);
        optim_st<VEC>(g, i, x);
    }
}

__global__ __launch_bounds__(256) void grad_scale_kernel(const OptimTable t, const float* __restrict__ gscale) {
    const OptimEntry e = t.e[optim_find(t)];
    const float c = gscale[0];
    float* g = const_cast<float*>(e.g);
    const unsigned beg = (blockIdx.x - e.first_block) * OCHUNK;
    const unsigned end = e.n - beg < (unsigned)OCHUNK ? e.n : beg + OCHUNK;
    unsigned vend = beg;
    if (((uintptr_t)g & 15) == 0) {
        vend = beg + ((end - beg) & ~3u);
        grad_scale_span<true>(g, c, beg, vend);
    }
    grad_scale_span<false>(g, c, vend, end);
}

// Validates the caller's table and lays it out for the kernel; returns the number of blocks through *blocks.
static int optim_pack(const dram_optim_tensor* table, int count, bool need_m, bool need_v, bool need_vmax, const char* who,
                      OptimTable& t, unsigned* blocks) {
    DRAM_REQUIRE(table, "%s: null table", who);
    DRAM_REQUIRE(count >= 1 && count <= DRAM_OPTIM_TABLE_CAPACITY, "%s: %d tensors in one table (1..%d)", who, count,
                 DRAM_OPTIM_TABLE_CAPACITY);
    uint64_t nb = 0;
    for (int i = 0; i < count; ++i) {
        const dram_optim_tensor& s = table[i];
        DRAM_REQUIRE(s.p && s.g, "%s: tensor %d: null pointer", who, i);
        DRAM_REQUIRE(!need_m || s.m, "%s: tensor %d: null first-moment pointer", who, i);
        DRAM_REQUIRE(!need_v || s.v, "%s: tensor %d: null second-moment pointer", who, i);
        DRAM_REQUIRE(!need_vmax || s.vmax, "%s: tensor %d: null max-second-moment pointer (amsgrad)", who, i);
        DRAM_REQUIRE(s.n >= 1 && s.n < ((int64_t)1 << 31), "%s: tensor %d: element count %lld outside 1 .. 2^31 - 1", who, i,
                     (long long)s.n);
        DRAM_REQUIRE((((uintptr_t)s.p | (uintptr_t)s.g | (uintptr_t)s.m | (uintptr_t)s.v | (uintptr_t)s.vmax) & 3) == 0,
                     "%s: tensor %d: pointer not 4-byte aligned", who, i);
        OptimEntry& e = t.e[i];
        e.p = s.p; e.g = s.g; e.m = s.m; e.v = need_v ? s.v : nullptr; e.vmax = need_vmax ? s.vmax : nullptr;
        e.n = (unsigned)s.n;
        e.first_block = (unsigned)nb;
        e.s0 = s.s0; e.s1 = s.s1;
        nb += (uint64_t)cdiv64(s.n, OCHUNK);
    }
    DRAM_REQUIRE(nb < ((uint64_t)1 << 31), "%s: table needs %llu blocks (limit 2^31 - 1)", who, (unsigned long long)nb);
    for (int i = count; i < DRAM_OPTIM_TABLE_CAPACITY; ++i) t.e[i] = OptimEntry{};
    t.count = count;
    *blocks = (unsigned)nb;
    return DRAM_OK;
}

// The same for the gradient-only kernels: g and n alone are read, every other field may be anything.
static int grad_pack(const dram_optim_tensor* table, int count, const char* who, OptimTable& t, unsigned* blocks) {
    DRAM_REQUIRE(table, "%s: null table", who);
    DRAM_REQUIRE(count >= 1 && count <= DRAM_OPTIM_TABLE_CAPACITY, "%s: %d tensors in one table (1..%d)", who, count,
                 DRAM_OPTIM_TABLE_CAPACITY);
    uint64_t nb = 0;
    for (int i = 0; i < DRAM_OPTIM_TABLE_CAPACITY; ++i) t.e[i] = OptimEntry{};
    for (int i = 0; i < count; ++i) {
        const dram_optim_tensor& s = table[i];
        DRAM_REQUIRE(s.g, "%s: tensor %d: null gradient pointer", who, i);
        DRAM_REQUIRE(s.n >= 1 && s.n < ((int64_t)1 << 31), "%s: tensor %d: element count %lld outside 1 .. 2^31 - 1", who, i,
                     (long long)s.n);
        DRAM_REQUIRE(((uintptr_t)s.g & 3) == 0, "%s: tensor %d: gradient pointer not 4-byte aligned", who, i);
        t.e[i].g = s.g;
        t.e[i].n = (unsigned)s.n;
        t.e[i].first_block = (unsigned)nb;
        nb += (uint64_t)cdiv64(s.n, OCHUNK);
    }
    DRAM_REQUIRE(nb < ((uint64_t)1 << 31), "%s: table needs %llu blocks (limit 2^31 - 1)", who, (unsigned long long)nb);
    t.count = count;
    *blocks = (unsigned)nb;
    return DRAM_OK;
}

static void adam_scalars(AdamScalars& s, double lr, double beta1, double beta2, double eps, double weight_decay, int decoupled,
                         int amsgrad, int maximize) {
    s.beta1 = (float)beta1; s.omb1 = (float)(1.0 - beta1);
    s.beta2 = (float)beta2; s.omb2 = (float)(1.0 - beta2);
    s.eps = (float)eps;
    s.wd = (float)weight_decay;
    s.decay = (float)(1.0 - lr * weight_decay);
    s.decoupled = decoupled != 0 && weight_decay != 0.0;
    s.amsgrad = amsgrad != 0;
    s.maximize = maximize != 0;
}

}  // namespace dram

using namespace dram;

extern "C" int dram_optim_table_capacity(void) { return DRAM_OPTIM_TABLE_CAPACITY; }

extern "C" int dram_optim_adam_scaled(const dram_optim_tensor* table, int count, double lr, double beta1, double beta2,
                                      double eps, double weight_decay, int decoupled, int amsgrad, int maximize,
                                      const float* gscale, void* stream) {
    OptimTable t;
    unsigned blocks = 0;
    const int rc = optim_pack(table, count, true, true, amsgrad != 0, "optim_adam", t, &blocks);
    if (rc != DRAM_OK) return rc;
    DRAM_REQUIRE(((uintptr_t)gscale & 3) == 0, "optim_adam: gscale not 4-byte aligned");
    AdamScalars s;
    adam_scalars(s, lr, beta1, beta2, eps, weight_decay, decoupled, amsgrad, maximize);
    hipLaunchKernelGGL((optim_kernel<AdamRule, AdamScalars>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, t, s, gscale);
    return check_launch("optim_adam");
}

extern "C" int dram_optim_adam(const dram_optim_tensor* table, int count, double lr, double beta1, double beta2, double eps,
                               double weight_decay, int decoupled, int amsgrad, int maximize, void* stream) {
    return dram_optim_adam_scaled(table, count, lr, beta1, beta2, eps, weight_decay, decoupled, amsgrad, maximize, nullptr,
                                  stream);
}

extern "C" int dram_optim_sgd_scaled(const dram_optim_tensor* table, int count, double lr, double momentum, double dampening,
                                     double weight_decay, int nesterov, int maximize, const float* gscale, void* stream) {
    OptimTable t;
    unsigned blocks = 0;
    const int rc = optim_pack(table, count, momentum != 0.0, false, false, "optim_sgd", t, &blocks);
    if (rc != DRAM_OK) return rc;
    DRAM_REQUIRE(((uintptr_t)gscale & 3) == 0, "optim_sgd: gscale not 4-byte aligned");
    if (momentum == 0.0)
        for (int i = 0; i < count; ++i) t.e[i].m = nullptr;
    SgdScalars s;
    s.lr = (float)lr;
    s.mu = (float)momentum;
    s.omd = (float)(1.0 - dampening);
    s.wd = (float)weight_decay;
    s.nesterov = nesterov != 0;
    s.maximize = maximize != 0;
    hipLaunchKernelGGL((optim_kernel<SgdRule, SgdScalars>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, t, s, gscale);
    return check_launch("optim_sgd");
}

extern "C" int dram_optim_sgd(const dram_optim_tensor* table, int count, double lr, double momentum, double dampening,
                              double weight_decay, int nesterov, int maximize, void* stream) {
    return dram_optim_sgd_scaled(table, count, lr, momentum, dampening, weight_decay, nesterov, maximize, nullptr, stream);
}

extern "C" int dram_optim_radam_scaled(const dram_optim_tensor* table, int count, double lr, double beta1, double beta2,
                                       double eps, double weight_decay, int decoupled, int maximize, const float* gscale,
                                       void* stream) {
    OptimTable t;
    unsigned blocks = 0;
    const int rc = optim_pack(table, count, true, true, false, "optim_radam", t, &blocks);
    if (rc != DRAM_OK) return rc;
    DRAM_REQUIRE(((uintptr_t)gscale & 3) == 0, "optim_radam: gscale not 4-byte aligned");
    RAdamScalars s;
    s.beta1 = (float)beta1; s.omb1 = (float)(1.0 - beta1);
    s.beta2 = (float)beta2; s.omb2 = (float)(1.0 - beta2);
    s.eps = (float)eps;
    s.wd = (float)weight_decay;
    s.decay = (float)(1.0 - lr * weight_decay);
    s.decoupled = decoupled != 0 && weight_decay != 0.0;
    s.maximize = maximize != 0;
    hipLaunchKernelGGL((optim_kernel<RAdamRule, RAdamScalars>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, t, s, gscale);
    return check_launch("optim_radam");
}

extern "C" int dram_optim_radam(const dram_optim_tensor* table, int count, double lr, double beta1, double beta2, double eps,
                                double weight_decay, int decoupled, int maximize, void* stream) {
    return dram_optim_radam_scaled(table, count, lr, beta1, beta2, eps, weight_decay, decoupled, maximize, nullptr, stream);
}

extern "C" int dram_optim_adabound_scaled(const dram_optim_tensor* table, int count, double beta1, double beta2, double eps,
                                          double weight_decay, int amsbound, double lower, double upper, const float* gscale,
                                          void* stream) {
    OptimTable t;
    unsigned blocks = 0;
    const int rc = optim_pack(table, count, true, true, amsbound != 0, "optim_adabound", t, &blocks);
    if (rc != DRAM_OK) return rc;
    DRAM_REQUIRE(((uintptr_t)gscale & 3) == 0, "optim_adabound: gscale not 4-byte aligned");
    DRAM_REQUIRE(lower <= upper, "optim_adabound: lower bound %g above upper bound %g", lower, upper);
    AdaBoundScalars s;
    s.beta1 = (float)beta1; s.omb1 = (float)(1.0 - beta1);
    s.beta2 = (float)beta2; s.omb2 = (float)(1.0 - beta2);
    s.eps = (float)eps;
    s.wd = (float)weight_decay;
    s.lower = (float)lower;
    s.upper = (float)upper;
    s.amsbound = amsbound != 0;
    hipLaunchKernelGGL((optim_kernel<AdaBoundRule, AdaBoundScalars>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, t, s,
                       gscale);
    return check_launch("optim_adabound");
}

extern "C" int dram_optim_adabound(const dram_optim_tensor* table, int count, double beta1, double beta2, double eps,
                                   double weight_decay, int amsbound, double lower, double upper, void* stream) {
    return dram_optim_adabound_scaled(table, count, beta1, beta2, eps, weight_decay, amsbound, lower, upper, nullptr, stream);
}

extern "C" size_t dram_optim_grad_norm_partials(const dram_optim_tensor* table, int count) {
    OptimTable t;
    unsigned blocks = 0;
    return grad_pack(table, count, "optim_grad_norm_partials", t, &blocks) == DRAM_OK ? (size_t)blocks : 0;
}

static int norm_kind_ok(int kind, const char* who) {
    DRAM_REQUIRE(kind == DRAM_OPTIM_NORM_2 || kind == DRAM_OPTIM_NORM_INF, "%s: norm kind %d (2: 2-norm, %d: inf-norm)", who, kind,
                 DRAM_OPTIM_NORM_INF);
    return DRAM_OK;
}

extern "C" int dram_optim_grad_norm(const dram_optim_tensor* table, int count, int kind, double* partials,
                                    int64_t partial_offset, void* stream) {
    OptimTable t;
    unsigned blocks = 0;
    int rc = grad_pack(table, count, "optim_grad_norm", t, &blocks);
    if (rc != DRAM_OK) return rc;
    if ((rc = norm_kind_ok(kind, "optim_grad_norm")) != DRAM_OK) return rc;
    DRAM_REQUIRE(partials, "optim_grad_norm: null partials buffer");
    DRAM_REQUIRE(((uintptr_t)partials & 7) == 0, "optim_grad_norm: partials buffer not 8-byte aligned");
    DRAM_REQUIRE(partial_offset >= 0, "optim_grad_norm: negative partial_offset %lld", (long long)partial_offset);
    double* dst = partials + partial_offset;
    if (kind == DRAM_OPTIM_NORM_2)
        hipLaunchKernelGGL((grad_norm_kernel<SumSq>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, t, dst);
    else
        hipLaunchKernelGGL((grad_norm_kernel<MaxAbs>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, t, dst);
    return check_launch("optim_grad_norm");
}

extern "C" int dram_optim_grad_norm_finish(const double* partials, int64_t n_partials, int kind, double max_norm, float* out,
                                           void* stream) {
    const int rc = norm_kind_ok(kind, "optim_grad_norm_finish");
    if (rc != DRAM_OK) return rc;
    DRAM_REQUIRE(partials, "optim_grad_norm_finish: null partials buffer");
    DRAM_REQUIRE(((uintptr_t)partials & 7) == 0, "optim_grad_norm_finish: partials buffer not 8-byte aligned");
    DRAM_REQUIRE(n_partials >= 1, "optim_grad_norm_finish: %lld partials (>= 1)", (long long)n_partials);
    DRAM_REQUIRE(out, "optim_grad_norm_finish: null out");
    DRAM_REQUIRE(((uintptr_t)out & 3) == 0, "optim_grad_norm_finish: out not 4-byte aligned");
    const long long n = n_partials;
    const float mx = (float)max_norm;
    if (kind == DRAM_OPTIM_NORM_2)
        hipLaunchKernelGGL((grad_norm_finish<SumSq, true>), dim3(1), dim3(256), 0, (hipStream_t)stream, partials, n, mx, out);
    else
        hipLaunchKernelGGL((grad_norm_finish<MaxAbs, false>), dim3(1), dim3(256), 0, (hipStream_t)stream, partials, n, mx, out);
    return check_launch("optim_grad_norm_finish");
}

extern "C" int dram_optim_grad_scale(const dram_optim_tensor* table, int count, const float* gscale, void* stream) {
    OptimTable t;
    unsigned blocks = 0;
    const int rc = grad_pack(table, count, "optim_grad_scale", t, &blocks);
    if (rc != DRAM_OK) return rc;
    DRAM_REQUIRE(gscale, "optim_grad_scale: null gscale");
    DRAM_REQUIRE(((uintptr_t)gscale & 3) == 0, "optim_grad_scale: gscale not 4-byte aligned");
    hipLaunchKernelGGL(grad_scale_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, t, gscale);
    return check_launch("optim_grad_scale");
}
