// RandomAffineTransform3D and RandomRotate on a device batch (gfx950): scipy.ndimage.affine_transform / rotate with
// mode="constant", order 3 for the image and order 0 for every other "#" entry (reference: dram/data_transforms.py:995-1102).
//
// Order 3 is two steps, as in scipy.  The prefilter turns the fp32 sample into fp64 cubic B-spline coefficients: per axis in turn
// (z first) and per line, times (1 - z)(1 - 1/z) with the pole z = sqrt(3) - 2, a causal recursion c[i] += z c[i-1] started from
// the mirror sum over the whole line, and an anticausal recursion c[i] = z (c[i+1] - c[i]) started from
// c[n-1] = z / (z^2 - 1) (c[n-1] + z c[n-2]).  A line of one element is left as it is.  An affine transform filters all three
// axes; a rotation is a 2-d transform of every plane, so only the two plane axes of the sample are filtered (axes mask).
// The gather then maps every output voxel to its source coordinate x_h = off_h + sum_l M[h][l] idx_l (fp64, added left to right,
// no contraction), writes the sample's minimum where any x_h lies outside [0, n_h - 1], and otherwise adds the 4 x 4 x 4 taps
// (4 x 4 in a plane) at floor(x) - 1 .., coefficient indices mirrored with period 2n - 2, in fp64.  Order 0 reads the voxel at
// floor(x + 0.5) of the sample itself.  tests/spline_restatement.py states the same arithmetic in numpy.
//
// Per-sample flags as in augment.hip: 1 = transform, 0 = pass through (copied), < 0 = skip.  No atomics in this file; the fill
// value comes from dram_aug_minmax / dram_aug_minmax_u8 (augment.hip), whose integer atomicMin / atomicMax on order keys are
// exact and independent of arrival order.  So a repeat gives the same bits.  Nothing synchronises with the host.
#include "volume_math.h"
#include <math.h>

namespace dram {
namespace {

constexpr double SPLINE_POLE = -0.26794919243112270647;     // sqrt(3) - 2
constexpr int XP_LINES = 256;           // x pass: lines (rows of the sample) per block, one per lane
constexpr int XP_CH = 16;               // x pass: elements of every line staged at a time (128 bytes of a row)
constexpr int XP_STRIDE = XP_CH + 1;    // LDS row stride in doubles (odd: the lanes of a half wave fall on different banks)

struct SplineRec {                      // 104 bytes, mirrored by dram_amd/augment.py:SPLINE_DTYPE
    double m[9];                        // row-major 3 x 3: source = m * (z, y, x) + off
    double off[3];
    int fixed;                          // -1: a 3-d transform; 0 / 1 / 2: a plane transform that leaves this axis alone
    int pad;
};
static_assert(sizeof(SplineRec) == 104, "SplineRec is part of the ABI");

// The start of the causal recursion from the line's elements c[0 .. n-1] (already times the gain):
//   (c[0] + z^(n-1) c[n-1] + sum_{i=1}^{n-2} (z^i + z^(2n-2-i)) c[i]) / (1 - z^(2n-2)),
// the two sums kept apart: s1 with a running power (which may underflow to 0: those terms are gone anyway) and s2 by Horner's
// rule from the left, so that no power of z is ever divided by.
// ON PURPOSE NOT scipy's order of additions: scipy accumulates z^i (c[i] + z^(n-1) c[n-1-i]) in one sum, which needs the mirrored
// element c[n-1-i] beside c[i] -- a second, opposite walk of the line, and for the x pass an element of another LDS step.  The
// two orders agree to a few fp64 steps of the sum (1e-16 relative), as does the numpy restatement written in scipy's order with
// scipy's own spline_filter (5e-14 on coefficients of 70): the coefficients are scipy's to fp64 rounding, not bit for bit, and
// the fp32 result can differ from scipy's in its final rounding (one step) -- or, where the taps cancel to a result near 0, by
// that fp64 noise, which is then large relative to the value.
struct CausalSum {
    double first, last, s1, s2, zi;
    __device__ __forceinline__ void init() { first = last = s1 = s2 = 0.0; zi = 1.0; }
    __device__ __forceinline__ void add(int i, int n, double v) {
#pragma clang fp contract(off)
        if (i == 0) first = v;
        else if (i == n - 1) last = v;
        else {
            zi = zi * SPLINE_POLE;
            s1 = s1 + zi * v;
            s2 = (s2 + v) * SPLINE_POLE;
        }
    }
    __device__ __forceinline__ double start(double zn1) const {
#pragma clang fp contract(off)
        return (((first + zn1 * last) + s1) + zn1 * s2) / (1.0 - zn1 * zn1);
    }
};

__device__ __forceinline__ double spline_gain() {
#pragma clang fp contract(off)
    return (1.0 - SPLINE_POLE) * (1.0 - 1.0 / SPLINE_POLE);
}

__device__ __forceinline__ double anticausal_start(double cn2, double cn1) {
#pragma clang fp contract(off)
    return (SPLINE_POLE * cn2 + cn1) * SPLINE_POLE / (SPLINE_POLE * SPLINE_POLE - 1.0);
}

// ---------------------------------------------------------------- prefilter along z (AXIS 0) and y (AXIS 1)
// Grid (cdiv(lines, 256), N).  A lane owns one line; neighbouring lanes own neighbouring x, so every access is coalesced.  The
// z pass is the first: it reads the fp32 sample and writes the workspace, also for a sample whose z axis is not filtered (a plain
// conversion).  The y pass works in place in the workspace.  Three walks of the line: the mirror sum, the causal recursion, the
// anticausal recursion.
template <int AXIS>
__global__ __launch_bounds__(256) void spline_lines_kernel(const float* __restrict__ x, double* __restrict__ ws,
                                                           const int* __restrict__ flag, const int* __restrict__ axes, int D,
                                                           int H, int W, double zn1) {
#pragma clang fp contract(off)
    const int n = blockIdx.y;
    if (flag[n] != 1) return;
    const int len = AXIS == 0 ? D : H;
    const bool filter = ((axes[n] >> AXIS) & 1) && len > 1;
    if (AXIS != 0 && !filter) return;
    const int64_t HW = (int64_t)H * W;
    const int64_t lines = AXIS == 0 ? HW : (int64_t)D * W;
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= lines) return;
    const int64_t base = (int64_t)n * D * HW + (AXIS == 0 ? g : (g / W) * HW + g % W);
    const int64_t step = AXIS == 0 ? HW : W;
    const double gain = spline_gain();
    auto src = [&](int i) -> double { return AXIS == 0 ? (double)x[base + i * step] : ws[base + i * step]; };
    if (!filter) {
        for (int i = 0; i < len; ++i) ws[base + i * step] = src(i);
        return;
    }
    CausalSum cs;
    cs.init();
    for (int i = 0; i < len; ++i) cs.add(i, len, src(i) * gain);
    double prev = cs.start(zn1), prev2 = 0.0;
    ws[base] = prev;
    for (int i = 1; i < len; ++i) {
        const double v = src(i) * gain + SPLINE_POLE * prev;
        ws[base + i * step] = v;
        prev2 = prev;
        prev = v;
    }
    double next = anticausal_start(prev2, prev);
    ws[base + (len - 1) * step] = next;
    for (int i = len - 2; i >= 0; --i) {
        const double v = SPLINE_POLE * (next - ws[base + i * step]);
        ws[base + i * step] = v;
        next = v;
    }
}

// ---------------------------------------------------------------- prefilter along x
// Grid (cdiv(D * H, XP_LINES), N), in place in the workspace.  A lane owns one row of the sample and runs its recursions
// serially; the rows' elements go through an LDS tile of XP_LINES x XP_CH doubles, so that the global reads and writes are
// row-contiguous (16 lanes move 128 bytes of one row) while a lane walks its own row in LDS.  Three walks of the rows in steps
// of XP_CH columns, as above; the last walk runs from the right.
__device__ __forceinline__ void xp_move(double* __restrict__ rows, double* tile, int nrows, int W, int c0, bool load) {
    for (int e = threadIdx.x; e < XP_LINES * XP_CH; e += 256) {
        const int r = e / XP_CH, k = e % XP_CH;
        if (r < nrows && c0 + k < W) {
            if (load) tile[r * XP_STRIDE + k] = rows[(int64_t)r * W + c0 + k];
            else rows[(int64_t)r * W + c0 + k] = tile[r * XP_STRIDE + k];
        }
    }
}

__global__ __launch_bounds__(256) void spline_x_kernel(double* __restrict__ ws, const int* __restrict__ flag,
                                                       const int* __restrict__ axes, int D, int H, int W, double zn1) {
#pragma clang fp contract(off)
    __shared__ double tile[XP_LINES * XP_STRIDE];
    const int n = blockIdx.y;
    if (flag[n] != 1 || !((axes[n] >> 2) & 1) || W < 2) return;      // (uniform over the block: no barrier is left behind)
    const int total = D * H;
    const int r0 = blockIdx.x * XP_LINES;
    const int nrows = total - r0 < XP_LINES ? total - r0 : XP_LINES;
    double* rows = ws + ((int64_t)n * total + r0) * W;
    const bool mine = (int)threadIdx.x < nrows;
    double* line = tile + threadIdx.x * XP_STRIDE;
    const double gain = spline_gain();
    const int nch = (W + XP_CH - 1) / XP_CH;

    CausalSum cs;
    cs.init();
    for (int c = 0; c < nch; ++c) {
        const int c0 = c * XP_CH, cnt = W - c0 < XP_CH ? W - c0 : XP_CH;
        xp_move(rows, tile, nrows, W, c0, true);
        __syncthreads();
        if (mine)
            for (int k = 0; k < cnt; ++k) cs.add(c0 + k, W, line[k] * gain);
        __syncthreads();
    }
    double prev = 0.0, prev2 = 0.0;
    for (int c = 0; c < nch; ++c) {
        const int c0 = c * XP_CH, cnt = W - c0 < XP_CH ? W - c0 : XP_CH;
        xp_move(rows, tile, nrows, W, c0, true);
        __syncthreads();
        if (mine)
            for (int k = 0; k < cnt; ++k) {
                const double v = c0 + k == 0 ? cs.start(zn1) : line[k] * gain + SPLINE_POLE * prev;
                line[k] = v;
                prev2 = prev;
                prev = v;
            }
        __syncthreads();
        xp_move(rows, tile, nrows, W, c0, false);
        __syncthreads();
    }
    double next = 0.0;
    for (int c = nch - 1; c >= 0; --c) {
        const int c0 = c * XP_CH, cnt = W - c0 < XP_CH ? W - c0 : XP_CH;
        xp_move(rows, tile, nrows, W, c0, true);
        __syncthreads();
        if (mine)
            for (int k = cnt - 1; k >= 0; --k) {
                const double v = c0 + k == W - 1 ? anticausal_start(prev2, prev) : SPLINE_POLE * (next - line[k]);
                line[k] = v;
                next = v;
            }
        __syncthreads();
        xp_move(rows, tile, nrows, W, c0, false);
        __syncthreads();
    }
}

// ---------------------------------------------------------------- gather
// Index i of a coefficient line of n elements under scipy's mirror (d c b | a b c d | c b a): period 2n - 2; n == 1 gives 0.
// Valid for every int i; the result is always in [0, n).
__device__ __forceinline__ int mirror_index(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * n - 2;
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - m;
}

struct SplineAxis {                     // one axis of one output voxel
    int cnt;                            // taps: 4, or 1 on the axis a plane transform leaves alone
    int idx[4];                         // element offsets of the taps along the axis (index times the axis stride)
    double w[4];
};

// The taps of source coordinate c on an axis of n elements `stride` apart (order 3: the weights as scipy forms them).
__device__ __forceinline__ void cubic_axis(double c, int n, int stride, bool fixed, SplineAxis& a) {
#pragma clang fp contract(off)
    const double fl = floor(c);
    if (fixed) {
        a.cnt = 1;
        a.idx[0] = mirror_index((int)fl, n) * stride;
        a.w[0] = 1.0;
        return;
    }
    const int start = (int)fl - 1;
    const double t = c - fl, u = 1.0 - t;
    a.cnt = 4;
    a.w[1] = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0;
    a.w[2] = (u * u * (u - 2.0) * 3.0 + 4.0) / 6.0;
    a.w[0] = u * u * u / 6.0;
    a.w[3] = 1.0 - a.w[0] - a.w[1] - a.w[2];
#pragma unroll
    for (int k = 0; k < 4; ++k) a.idx[k] = mirror_index(start + k, n) * stride;
}

// Grid (cdiv(D * H * W, 256), N): one output voxel per lane, x fastest, so that neighbouring lanes read overlapping taps.
// ORDER 3 reads the coefficients `ws` (T = float); ORDER 0 reads x.  The fill value is the sample's minimum, minmax[n][0].
template <typename T, int ORDER>
__global__ __launch_bounds__(256) void spline_resample_kernel(const T* __restrict__ x, T* __restrict__ y,
                                                              const double* __restrict__ ws, const SplineRec* __restrict__ table,
                                                              const float* __restrict__ minmax, const int* __restrict__ flag,
                                                              int D, int H, int W) {
#pragma clang fp contract(off)
    const int n = blockIdx.y;
    const int f = flag[n];
    if (f < 0) return;
    const int64_t S = (int64_t)D * H * W;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= S) return;
    const T* xs = x + (int64_t)n * S;
    T* ys = y + (int64_t)n * S;
    if (f == 0) {
        ys[i] = xs[i];
        return;
    }
    const SplineRec& r = table[n];
    const unsigned row = (unsigned)i / (unsigned)W;          // i < 2^31: 32-bit divisions
    const int xx = (int)((unsigned)i - row * (unsigned)W), yy = (int)(row % (unsigned)H), zz = (int)(row / (unsigned)H);
    const int dim[3] = {D, H, W};
    double c[3];
    bool in = true;
#pragma unroll
    for (int h = 0; h < 3; ++h) {
        c[h] = ((r.off[h] + r.m[3 * h] * (double)zz) + r.m[3 * h + 1] * (double)yy) + r.m[3 * h + 2] * (double)xx;
        in = in && c[h] >= 0.0 && c[h] <= (double)(dim[h] - 1);      // (false for NaN)
    }
    const T cval = (T)minmax[2 * n];
    if (!in) {
        ys[i] = cval;
        return;
    }
    if (ORDER == 0) {
        int q[3];
#pragma unroll
        for (int h = 0; h < 3; ++h) {
            const int v = (int)floor(c[h] + 0.5);
            q[h] = v < 0 ? 0 : (v > dim[h] - 1 ? dim[h] - 1 : v);
        }
        ys[i] = xs[((int64_t)q[0] * H + q[1]) * W + q[2]];
        return;
    }
    const double* cf = ws + (int64_t)n * S;
    SplineAxis az, ay, ax;
    cubic_axis(c[0], D, H * W, r.fixed == 0, az);
    cubic_axis(c[1], H, W, r.fixed == 1, ay);
    cubic_axis(c[2], W, 1, r.fixed == 2, ax);
    double acc = 0.0;
    for (int a = 0; a < az.cnt; ++a)
        for (int b = 0; b < ay.cnt; ++b) {
            const double* p = cf + az.idx[a] + ay.idx[b];
            for (int k = 0; k < ax.cnt; ++k) acc = acc + ((p[ax.idx[k]] * az.w[a]) * ay.w[b]) * ax.w[k];
        }
    ys[i] = (T)acc;
}

bool spline_sizes_ok(int N, int D, int H, int W) {
    return N > 0 && N <= 65535 && D > 0 && H > 0 && W > 0 && (int64_t)D * H * W <= 0x1fffffffLL;
}

}  // namespace
}  // namespace dram

using namespace dram;

extern "C" size_t dram_aug_spline_ws_bytes(int N, int D, int H, int W) {
    if (!spline_sizes_ok(N, D, H, W)) return 0;
    return (size_t)N * D * H * W * sizeof(double);
}

extern "C" int dram_aug_spline_prefilter(const float* x, const int* axes, const int* flag, int n_table, int N, int D, int H,
                                         int W, void* ws, size_t ws_bytes, void* stream) {
    DRAM_REQUIRE(x && axes && flag && ws, "aug_spline_prefilter: null pointer");
    DRAM_REQUIRE(spline_sizes_ok(N, D, H, W), "aug_spline_prefilter: bad sizes (N 1..65535, D*H*W 1..2^29-1)");
    DRAM_REQUIRE(n_table == N, "aug_spline_prefilter: table length %d does not match the batch of %d samples", n_table, N);
    DRAM_REQUIRE(((uintptr_t)ws & 7) == 0 && ((uintptr_t)x & 3) == 0, "aug_spline_prefilter: misaligned pointer");
    if (ws_bytes < dram_aug_spline_ws_bytes(N, D, H, W)) {
        set_error("aug_spline_prefilter: workspace too small");
        return DRAM_EWS;
    }
    hipStream_t st = (hipStream_t)stream;
    double* c = (double*)ws;
    const int64_t HW = (int64_t)H * W;
    hipLaunchKernelGGL(spline_lines_kernel<0>, dim3((unsigned)cdiv64(HW, 256), N), dim3(256), 0, st, x, c, flag, axes, D, H, W,
                       pow(SPLINE_POLE, D - 1));
    if (H > 1)
        hipLaunchKernelGGL(spline_lines_kernel<1>, dim3((unsigned)cdiv64((int64_t)D * W, 256), N), dim3(256), 0, st, x, c, flag,
                           axes, D, H, W, pow(SPLINE_POLE, H - 1));
    if (W > 1)
        hipLaunchKernelGGL(spline_x_kernel, dim3((unsigned)cdiv64((int64_t)D * H, XP_LINES), N), dim3(256), 0, st, c, flag, axes,
                           D, H, W, pow(SPLINE_POLE, W - 1));
    return check_launch("aug_spline_prefilter");
}

extern "C" int dram_aug_spline_resample(const void* x, void* y, int elem_size, int order, const void* table, const float* minmax,
                                        const void* ws, size_t ws_bytes, const int* flag, int n_table, int N, int D, int H,
                                        int W, void* stream) {
    DRAM_REQUIRE(x && y && table && minmax && flag, "aug_spline_resample: null pointer");
    DRAM_REQUIRE(elem_size == 1 || elem_size == 4, "aug_spline_resample: element size %d (supported: 4 = float32, 1 = uint8)",
                 elem_size);
    DRAM_REQUIRE(order == 0 || order == 3, "aug_spline_resample: order %d (supported: 0 and 3)", order);
    DRAM_REQUIRE(order == 0 || elem_size == 4, "aug_spline_resample: order 3 is built for float32 only");
    DRAM_REQUIRE(spline_sizes_ok(N, D, H, W), "aug_spline_resample: bad sizes (N 1..65535, D*H*W 1..2^29-1)");
    DRAM_REQUIRE(n_table == N, "aug_spline_resample: table length %d does not match the batch of %d samples", n_table, N);
    DRAM_REQUIRE(x != y, "aug_spline_resample: cannot run in place");
    DRAM_REQUIRE(((uintptr_t)table & 7) == 0 && ((uintptr_t)x & (elem_size - 1)) == 0 && ((uintptr_t)y & (elem_size - 1)) == 0 &&
                     ((uintptr_t)minmax & 3) == 0,
                 "aug_spline_resample: misaligned pointer");
    if (order == 3) {
        DRAM_REQUIRE(ws, "aug_spline_resample: order 3 needs the coefficients of dram_aug_spline_prefilter");
        DRAM_REQUIRE(((uintptr_t)ws & 7) == 0, "aug_spline_resample: workspace must be 8-byte aligned");
        if (ws_bytes < dram_aug_spline_ws_bytes(N, D, H, W)) {
            set_error("aug_spline_resample: workspace too small");
            return DRAM_EWS;
        }
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)cdiv64((int64_t)D * H * W, 256), N);
    const SplineRec* t = (const SplineRec*)table;
    const double* c = (const double*)ws;
    if (order == 3)
        hipLaunchKernelGGL((spline_resample_kernel<float, 3>), grid, dim3(256), 0, st, (const float*)x, (float*)y, c, t, minmax,
                           flag, D, H, W);
    else if (elem_size == 4)
        hipLaunchKernelGGL((spline_resample_kernel<float, 0>), grid, dim3(256), 0, st, (const float*)x, (float*)y, c, t, minmax,
                           flag, D, H, W);
    else
        hipLaunchKernelGGL((spline_resample_kernel<unsigned char, 0>), grid, dim3(256), 0, st, (const unsigned char*)x,
                           (unsigned char*)y, c, t, minmax, flag, D, H, W);
    return check_launch("aug_spline_resample");
}
