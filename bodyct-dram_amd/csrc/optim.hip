// The optimiser update of the training step (st_dram_ref.py: torch.optim.Adam; the SGD-with-momentum block beside it), gfx950:
// multi-tensor Adam / AdamW / SGD, one launch per table of up to DRAM_OPTIM_TABLE_CAPACITY tensors.
//
// The table travels in the kernel arguments (no device buffer, no copy, nothing to keep alive; the gradient pointers change
// every step, so the host rebuilds it each step anyway).  The host gives every tensor cdiv(n, OCHUNK) consecutive blocks and
// records the first one; a block finds its tensor by bisecting those starts (wave-uniform, scalar loads of the arguments).
// A tensor whose pointers are all 16-byte aligned moves its whole groups of four as 16-byte accesses (span<true>) and its last
// n % 4 elements one by one (span<false>); a tensor with any misaligned pointer -- a gradient that is a view into a flat
// all-reduce bucket at an arbitrary offset -- takes span<false> throughout: one dword per lane, consecutive lanes on
// consecutive addresses.  Each element is read and written by exactly one lane: no atomics, no LDS, deterministic.
// HBM traffic per element: Adam 16 B read + 12 B written (amsgrad: +4 +4); SGD with momentum 12 B + 8 B.
//
// Every product, sum, quotient and root below is one IEEE fp32 operation (fmaf: one rounding for a*b+c); the count of
// roundings per quantity is what tests/optim_restatement.py bounds.
#include "common.h"

namespace dram {

constexpr int OCHUNK = 4096;   // elements per block: 256 lanes x 4 groups of 4

struct OptimEntry {            // 56 bytes
    float* p;
    const float* g;
    float* m;                  // Adam: exp_avg; SGD: momentum_buffer (NULL without momentum)
    float* v;                  // Adam: exp_avg_sq
    float* vmax;               // Adam with amsgrad: max_exp_avg_sq, else NULL
    unsigned n, first_block;
    float s0, s1;              // Adam: lr / bc1, sqrt(bc2); SGD: s0 != 0 on the tensor's first step (buf = g')
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
    float step_size, bc2_sqrt;
    bool has_vmax;
    __device__ __forceinline__ void load(const OptimEntry& e) { step_size = e.s0; bc2_sqrt = e.s1; has_vmax = a.amsgrad != 0; }
    __device__ __forceinline__ bool reads_m() const { return true; }
    __device__ __forceinline__ bool uses_m() const { return true; }
    __device__ __forceinline__ bool uses_v() const { return true; }
    __device__ __forceinline__ bool uses_vmax() const { return has_vmax; }
    __device__ __forceinline__ void apply(float& p, float g, float& m, float& v, float& vmax) const {
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
    bool first, has_buf;
    __device__ __forceinline__ void load(const OptimEntry& e) { first = e.s0 != 0.f; has_buf = e.m != nullptr; }
    __device__ __forceinline__ bool reads_m() const { return has_buf && !first; }
    __device__ __forceinline__ bool uses_m() const { return has_buf; }
    __device__ __forceinline__ bool uses_v() const { return false; }
    __device__ __forceinline__ bool uses_vmax() const { return false; }
    __device__ __forceinline__ void apply(float& p, float g, float& m, float&, float&) const {
        if (a.maximize) g = -g;
        if (a.wd != 0.f) g = fmaf(a.wd, p, g);
        if (has_buf) {
            m = first ? g : fmaf(a.mu, m, __fmul_rn(a.omd, g));
            g = a.nesterov ? fmaf(a.mu, m, g) : m;
        }
        p = fmaf(-a.lr, g, p);
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

template <class Rule, class Scalars>
__global__ __launch_bounds__(256) void optim_kernel(const OptimTable t, const Scalars s) {
    // the last tensor whose first block is <= this block (first_block is increasing, e[0].first_block == 0)
    int lo = 0, hi = t.count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (t.e[mid].first_block <= blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const OptimEntry e = t.e[lo];
    Rule r;
    r.a = s;
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

}  // namespace dram

using namespace dram;

extern "C" int dram_optim_table_capacity(void) { return DRAM_OPTIM_TABLE_CAPACITY; }

extern "C" int dram_optim_adam(const dram_optim_tensor* table, int count, double lr, double beta1, double beta2, double eps,
                               double weight_decay, int decoupled, int amsgrad, int maximize, void* stream) {
    OptimTable t;
    unsigned blocks = 0;
    const int rc = optim_pack(table, count, true, true, amsgrad != 0, "optim_adam", t, &blocks);
    if (rc != DRAM_OK) return rc;
    AdamScalars s;
    s.beta1 = (float)beta1; s.omb1 = (float)(1.0 - beta1);
    s.beta2 = (float)beta2; s.omb2 = (float)(1.0 - beta2);
    s.eps = (float)eps;
    s.wd = (float)weight_decay;
    s.decay = (float)(1.0 - lr * weight_decay);
    s.decoupled = decoupled != 0 && weight_decay != 0.0;
    s.amsgrad = amsgrad != 0;
    s.maximize = maximize != 0;
    hipLaunchKernelGGL((optim_kernel<AdamRule, AdamScalars>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, t, s);
    return check_launch("optim_adam");
}

extern "C" int dram_optim_sgd(const dram_optim_tensor* table, int count, double lr, double momentum, double dampening,
                              double weight_decay, int nesterov, int maximize, void* stream) {
    OptimTable t;
    unsigned blocks = 0;
    const int rc = optim_pack(table, count, momentum != 0.0, false, false, "optim_sgd", t, &blocks);
    if (rc != DRAM_OK) return rc;
    if (momentum == 0.0)
        for (int i = 0; i < count; ++i) t.e[i].m = nullptr;
    SgdScalars s;
    s.lr = (float)lr;
    s.mu = (float)momentum;
    s.omd = (float)(1.0 - dampening);
    s.wd = (float)weight_decay;
    s.nesterov = nesterov != 0;
    s.maximize = maximize != 0;
    hipLaunchKernelGGL((optim_kernel<SgdRule, SgdScalars>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, t, s);
    return check_launch("optim_sgd");
}
