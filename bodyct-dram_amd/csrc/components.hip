// Lesion-wise report at inference (gfx950): 3-D connected-component labelling of a binary mask on the device, per-component
// statistics, the look-up-table relabelling that filters and renumbers components, and the per-lobe lesion burden.
//
// Labelling is union-find on the linear voxel index, in a FIXED sequence of six launches (no host loop, no flag read back, no
// device loop that waits for another thread):
//   cc_init      P[i] = i on set voxels, -1 on the background                       (P is the `labels` output itself)
//   cc_merge     every set voxel unites itself with those of its 3 / 9 / 13 neighbours of SMALLER linear index that are set
//   cc_flatten   P[i] = root of i; a root is its component's minimum index; roots are counted per block of CC_TILE voxels
//   cc_scan      exclusive prefix of the block counts (one block, integers: exact), the total is the component count
//   cc_rank      a root's rank = roots before it in raster order; stored in place as -(rank + 2)
//   cc_final     every voxel takes rank(root) + 1, the background 0
// The invariant behind every loop: P[x] <= x for every set voxel, at every moment.  cc_init establishes it, and P[x] is only
// ever lowered (atomicMin in cc_merge, the root in cc_flatten).  A `find` therefore follows strictly decreasing indices and ends
// at a fixed point; nothing depends on the order in which the atomics land, since the root of a component is its minimum index
// whatever the shape of the tree was.  Numbering roots in raster order is scipy.ndimage.label's numbering.
#include "label_stream.h"

namespace dram {

constexpr int CC_TILE = 1024;       // voxels per block of cc_flatten / cc_rank: 4 chunks of 256, a wave owns 64 consecutive ones
constexpr int CC_CHUNKS = CC_TILE / 256;

// The neighbours of smaller linear index (dz, dy, dx lexicographically below 0), ordered by |dz| + |dy| + |dx|: the first 3
// share a face (connectivity 1), the first 9 a face or an edge (2), all 13 at least a corner (3).
__constant__ signed char CC_NB[13][3] = {
    {0, 0, -1}, {0, -1, 0}, {-1, 0, 0},
    {0, -1, -1}, {0, -1, 1}, {-1, 0, -1}, {-1, 0, 1}, {-1, -1, 0}, {-1, 1, 0},
    {-1, -1, -1}, {-1, -1, 1}, {-1, 1, -1}, {-1, 1, 1}};

__global__ __launch_bounds__(256) void cc_init_kernel(const uint8_t* __restrict__ mask, int* __restrict__ P, long long nvox) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < nvox) P[i] = mask[i] ? (int)i : -1;
}

// A relaxed device-scope load: the value may be older than the latest atomicMin, never invalid -- an older parent is still an
// ancestor-or-equal in the same component and still <= x (see the invariant above).
__device__ __forceinline__ int cc_load(const int* P, int x) {
    return __hip_atomic_load(P + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int cc_find(const int* P, int x) {
    // Ends by construction: P[x] <= x, so every step that does not stop strictly decreases x, and x >= 0.
    int p = cc_load(P, x);
    while (p != x) {
        x = p;
        p = cc_load(P, x);
    }
    return x;
}

__device__ __forceinline__ void cc_union(int* P, int a, int b) {
    // Ends by construction: a round either returns or replaces the pair (a, b), a > b, by (old, b) with old < a -- the pair's
    // maximum strictly decreases (cc_find only lowers its argument) and is bounded by 0.  No round waits for another thread:
    // a lost race hands this thread the value that won (old) and the duty to unite it with b, which keeps every requested
    // union in the closure of the parent links.
    for (;;) {
        a = cc_find(P, a);
        b = cc_find(P, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&P[a], b);
        if (old == a) return;          // a was a root and hangs under b now
        a = old;                       // a had got a parent meanwhile (old < a): P[a] = min(old, b), and old still needs b
    }
}

// One thread per voxel.  Neighbours are addressed by (z, y, x) with a bounds check per axis, never by a linear offset alone: the
// voxel at x = W - 1 does not see x = 0 of the next row.
__global__ __launch_bounds__(256) void cc_merge_kernel(const uint8_t* __restrict__ mask, int* P, int nn, int D, int H, int W) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long nvox = (long long)D * H * W;
    if (i >= nvox || !mask[i]) return;
    const int x = (int)(i % W), row = (int)(i / W);
    const int y = row % H, z = row / H;
    for (int k = 0; k < nn; ++k) {
        const int zz = z + CC_NB[k][0], yy = y + CC_NB[k][1], xx = x + CC_NB[k][2];
        if (zz < 0 || yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
        const long long j = ((long long)zz * H + yy) * W + xx;
        if (mask[j]) cc_union(P, (int)i, (int)j);
    }
}

// Block b owns voxels [b * CC_TILE, (b + 1) * CC_TILE): chunk k of it is 256 consecutive voxels, one per thread, so that a wave's
// lanes hold 64 consecutive voxels and a ballot is their raster order.
__global__ __launch_bounds__(256) void cc_flatten_kernel(int* P, int* __restrict__ block_count, long long nvox) {
    __shared__ int wave_roots[4];
    int roots = 0;
    for (int k = 0; k < CC_CHUNKS; ++k) {
        const long long i = (long long)blockIdx.x * CC_TILE + k * 256 + threadIdx.x;
        bool is_root = false;
        if (i < nvox) {
            const int p = P[i];
            if (p >= 0) {
                // Ends by construction: P[r] <= r (this kernel only replaces a parent by the root, which is smaller still), so
                // the walk strictly decreases r until the fixed point.
                int r = p, q = P[r];
                while (q != r) { r = q; q = P[r]; }
                if (r != p) P[i] = r;
                is_root = r == (int)i;
            }
        }
        roots += __popcll(__ballot(is_root));
    }
    if ((threadIdx.x & 63) == 0) wave_roots[threadIdx.x >> 6] = roots;
    __syncthreads();
    if (threadIdx.x == 0) block_count[blockIdx.x] = wave_roots[0] + wave_roots[1] + wave_roots[2] + wave_roots[3];
}

// Exclusive prefix sum of cnt[0 .. nb) in place, one block of 1024 threads walking chunks of 1024 with a carry; *total = the sum.
__global__ __launch_bounds__(1024) void cc_scan_kernel(int* __restrict__ cnt, int nb, int* __restrict__ total) {
    __shared__ int wsum[16];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int carry = 0;
    for (int base = 0; base < nb; base += 1024) {          // the trip count is uniform over the block
        const int i = base + threadIdx.x;
        const int v = i < nb ? cnt[i] : 0;
        int s = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(s, o, 64);
            if (lane >= o) s += t;
        }
        if (lane == 63) wsum[w] = s;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int c = wsum[k];
            if (k < w) before += c;
            all += c;
        }
        if (i < nb) cnt[i] = carry + before + s - v;
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

// A root (P[i] == i) gets its rank among the roots in raster order: block offset + the (chunk, wave) segments before its own +
// the roots on lower lanes.  The rank is stored in place as -(rank + 2): below -1, the background's value, and told from a
// parent index (>= 0) by its sign.  Every thread reads and writes its own voxels only.
__global__ __launch_bounds__(256) void cc_rank_kernel(int* P, const int* __restrict__ block_off, long long nvox) {
    __shared__ int seg[CC_CHUNKS][4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    bool is_root[CC_CHUNKS];
    int below[CC_CHUNKS];
#pragma unroll
    for (int k = 0; k < CC_CHUNKS; ++k) {
        const long long i = (long long)blockIdx.x * CC_TILE + k * 256 + threadIdx.x;
        is_root[k] = i < nvox && P[i] == (int)i;
        const unsigned long long m = __ballot(is_root[k]);
        below[k] = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) seg[k][w] = __popcll(m);
    }
    __syncthreads();
    int off = block_off[blockIdx.x];
#pragma unroll
    for (int k = 0; k < CC_CHUNKS; ++k) {
#pragma unroll
        for (int ww = 0; ww < 4; ++ww) {
            if (ww == w && is_root[k]) {
                const long long i = (long long)blockIdx.x * CC_TILE + k * 256 + threadIdx.x;
                P[i] = -(off + below[k]) - 2;
            }
            off += seg[k][ww];
        }
    }
}

// labels[i] = rank(root of i) + 1.  A non-root holds its root's index r >= 0 and reads P[r], which is either the code of
// cc_rank (negative) or, if the root's own thread came first, the final label (positive): both decode to the same number.  A
// voxel is written by its own thread only.
__global__ __launch_bounds__(256) void cc_final_kernel(int* P, long long nvox) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nvox) return;
    const int v = P[i];
    if (v == -1) { P[i] = 0; return; }
    int u = v;
    if (v >= 0) u = cc_load(P, v);
    P[i] = u < 0 ? -u - 1 : u;
}

// ---- per-component statistics
__global__ __launch_bounds__(256) void cc_stats_init_kernel(unsigned long long* __restrict__ voxels, int* __restrict__ bbox,
                                                            unsigned long long* __restrict__ hits, int n, int D, int H, int W) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    voxels[k] = 0;
    if (hits) hits[k] = 0;
    int* b = bbox + (size_t)k * 6;
    b[0] = D; b[1] = 0; b[2] = H; b[3] = 0; b[4] = W; b[5] = 0;
}

// One thread per voxel; a wave's lanes hold 64 consecutive voxels.  The lanes of a wave that carry the same label are served
// together: one 64-bit add of their number (and of their hits), and -- when the group's first and last voxel lie in one row, the
// usual case -- one set of box atomics from the two ends of the run.  A group that spans rows sends its box atomics lane by
// lane.  Integer sums and min / max: the result does not depend on the order.  A label outside 1..n touches nothing.
__global__ __launch_bounds__(256) void cc_stats_kernel(const int* __restrict__ labels, const uint8_t* __restrict__ other, int n,
                                                       unsigned long long* voxels, int* bbox, unsigned long long* hits,
                                                       int H, int W, long long nvox) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int l = i < nvox ? labels[i] : 0;
    const bool valid = l >= 1 && l <= n;
    const bool hit = valid && other && other[i];
    unsigned long long todo = __ballot(valid);
    while (todo) {                                         // wave-uniform; the rounds of wave_reduce_by_key (label_stream.h)
        const int lead = __shfl(l, __ffsll((long long)todo) - 1, 64);
        const bool mine = valid && l == lead;
        const unsigned long long m = __ballot(mine), mh = __ballot(mine && hit);
        const int first = __ffsll((long long)m) - 1, last = 63 - __clzll((long long)m);
        const long long i_first = i - lane + first, i_last = i - lane + last;
        const long long row_first = i_first / W, row_last = i_last / W;
        int* b = bbox + (size_t)(lead - 1) * 6;
        if (lane == first) {
            atomicAdd(&voxels[lead - 1], (unsigned long long)__popcll(m));
            if (hits && mh) atomicAdd(&hits[lead - 1], (unsigned long long)__popcll(mh));
        }
        if (row_first == row_last) {
            if (lane == first) {
                const int z = (int)(row_first / H), y = (int)(row_first % H);
                const int x0 = (int)(i_first - row_first * W), x1 = (int)(i_last - row_first * W);
                atomicMin(&b[0], z); atomicMax(&b[1], z + 1);
                atomicMin(&b[2], y); atomicMax(&b[3], y + 1);
                atomicMin(&b[4], x0); atomicMax(&b[5], x1 + 1);
            }
        } else if (mine) {
            const long long row = i / W;
            const int z = (int)(row / H), y = (int)(row % H), x = (int)(i - row * W);
            atomicMin(&b[0], z); atomicMax(&b[1], z + 1);
            atomicMin(&b[2], y); atomicMax(&b[3], y + 1);
            atomicMin(&b[4], x); atomicMax(&b[5], x + 1);
        }
        todo &= ~m;
    }
}

// out_labels[i] = lut[labels[i]] (0 for a label outside 0..n), out_mask[i] = out_labels[i] != 0.  Element-wise, so out_labels
// may be labels itself.
__global__ __launch_bounds__(256) void cc_relabel_kernel(const int* labels, const int* __restrict__ lut, int n, int* out_labels,
                                                         uint8_t* __restrict__ out_mask, long long nvox) {
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nvox; i += stride) {
        const int l = labels[i];
        const int v = (l >= 0 && l <= n) ? lut[l] : 0;
        if (out_labels) out_labels[i] = v;
        if (out_mask) out_mask[i] = v != 0;
    }
}

// ---- per-lobe burden: counts[v] = {voxels with lobe == v, of which mask != 0}
// The pattern of chunk_hist_kernel (prep.hip): one LDS table per wave, then one 64-bit atomic per occupied entry and block.  A
// lobe map is long runs of one value, so a thread keeps the pair of its current value in registers and goes to LDS only when
// the value changes.  16-byte groups where both buffers are 16-byte aligned, the rest element by element.  The 32-bit LDS counts
// cannot wrap for the reason given in label_stream.h.
struct BurdenRun {
    unsigned* table;        // this wave's [256][2]
    int value;              // -1: nothing pending
    unsigned vox, set;
    __device__ __forceinline__ void flush() {
        if (value >= 0) {
            atomicAdd(&table[value * 2], vox);
            if (set) atomicAdd(&table[value * 2 + 1], set);
        }
    }
    __device__ __forceinline__ void add(unsigned lobe, unsigned mask) {
        if ((int)lobe != value) { flush(); value = (int)lobe; vox = 0; set = 0; }
        ++vox;
        set += mask != 0;
    }
};

__global__ __launch_bounds__(256) void lobe_burden_kernel(const uint8_t* __restrict__ mask, const uint8_t* __restrict__ lobe,
                                                          unsigned long long* __restrict__ counts, long long nvox, long long groups) {
    __shared__ unsigned table[4][512];
    for (int k = 0; k < 8; ++k) (&table[0][0])[k * 256 + threadIdx.x] = 0;
    __syncthreads();
    BurdenRun run{table[threadIdx.x >> 6], -1, 0, 0};
    const long long stride = (long long)gridDim.x * 256, t0 = (long long)blockIdx.x * 256 + threadIdx.x;
    for (long long g = t0; g < groups; g += stride) {
        const uint4 lv = reinterpret_cast<const uint4*>(lobe)[g], mv = reinterpret_cast<const uint4*>(mask)[g];
#pragma unroll
        for (int k = 0; k < 16; ++k) run.add(byte_of(lv, k), byte_of(mv, k));
    }
    for (long long e = groups * 16 + t0; e < nvox; e += stride) run.add(lobe[e], mask[e]);
    run.flush();
    __syncthreads();
    for (int k = 0; k < 2; ++k) {
        const int e = k * 256 + threadIdx.x;
        const unsigned long long c = (unsigned long long)table[0][e] + table[1][e] + table[2][e] + table[3][e];
        if (c) atomicAdd(&counts[e], c);
    }
}

static inline bool cc_sizes_ok(int D, int H, int W) {
    return D > 0 && H > 0 && W > 0 && (long long)D * H * W < (1LL << 31);
}

}  // namespace dram

using namespace dram;

extern "C" size_t dram_cc_ws_bytes(int D, int H, int W) {
    if (!cc_sizes_ok(D, H, W)) {
        set_error("cc_ws_bytes: sizes must be positive with D*H*W < 2^31");
        return 0;
    }
    return (size_t)cdiv64((int64_t)D * H * W, CC_TILE) * sizeof(int);
}

extern "C" int dram_cc_label(const uint8_t* mask, int32_t* labels, int32_t* count, int connectivity, int D, int H, int W,
                             void* ws, size_t ws_bytes, void* stream) {
    DRAM_REQUIRE(mask && labels && count && ws, "cc_label: null pointer");
    DRAM_REQUIRE(cc_sizes_ok(D, H, W), "cc_label: sizes must be positive with D*H*W < 2^31");
    DRAM_REQUIRE(connectivity >= 1 && connectivity <= 3, "cc_label: connectivity must be 1, 2 or 3 (6, 18 or 26 neighbours)");
    DRAM_REQUIRE(((uintptr_t)ws & 3) == 0 && ((uintptr_t)labels & 3) == 0, "cc_label: labels and workspace must be 4-byte aligned");
    if (ws_bytes < dram_cc_ws_bytes(D, H, W)) {
        set_error("cc_label: workspace too small");
        return DRAM_EWS;
    }
    const long long nvox = (long long)D * H * W;
    const unsigned per_voxel = (unsigned)cdiv64(nvox, 256), tiles = (unsigned)cdiv64(nvox, CC_TILE);
    const int nn = connectivity == 1 ? 3 : (connectivity == 2 ? 9 : 13);
    int* block = (int*)ws;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cc_init_kernel, dim3(per_voxel), dim3(256), 0, st, mask, labels, nvox);
    hipLaunchKernelGGL(cc_merge_kernel, dim3(per_voxel), dim3(256), 0, st, mask, labels, nn, D, H, W);
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(tiles), dim3(256), 0, st, labels, block, nvox);
    hipLaunchKernelGGL(cc_scan_kernel, dim3(1), dim3(1024), 0, st, block, (int)tiles, count);
    hipLaunchKernelGGL(cc_rank_kernel, dim3(tiles), dim3(256), 0, st, labels, (const int*)block, nvox);
    hipLaunchKernelGGL(cc_final_kernel, dim3(per_voxel), dim3(256), 0, st, labels, nvox);
    return check_launch("cc_label");
}

extern "C" int dram_cc_stats(const int32_t* labels, const uint8_t* other, int n, int64_t* voxels, int32_t* bbox, int64_t* hits,
                             int D, int H, int W, void* stream) {
    DRAM_REQUIRE(labels && voxels && bbox, "cc_stats: null pointer");
    DRAM_REQUIRE((other == nullptr) == (hits == nullptr), "cc_stats: other and hits go together");
    DRAM_REQUIRE(cc_sizes_ok(D, H, W), "cc_stats: sizes must be positive with D*H*W < 2^31");
    DRAM_REQUIRE(n > 0, "cc_stats: n must be positive");
    const long long nvox = (long long)D * H * W;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cc_stats_init_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, (unsigned long long*)voxels, bbox,
                       (unsigned long long*)hits, n, D, H, W);
    hipLaunchKernelGGL(cc_stats_kernel, dim3((unsigned)cdiv64(nvox, 256)), dim3(256), 0, st, labels, other, n,
                       (unsigned long long*)voxels, bbox, (unsigned long long*)hits, H, W, nvox);
    return check_launch("cc_stats");
}

extern "C" int dram_cc_relabel(const int32_t* labels, const int32_t* lut, int n, int32_t* out_labels, uint8_t* out_mask,
                               int64_t nvox, void* stream) {
    DRAM_REQUIRE(labels && lut, "cc_relabel: null pointer");
    DRAM_REQUIRE(out_labels || out_mask, "cc_relabel: no output");
    DRAM_REQUIRE(n >= 0, "cc_relabel: negative n");
    DRAM_REQUIRE(nvox > 0 && nvox < (1LL << 31), "cc_relabel: nvox must be in 1 .. 2^31 - 1");
    const int64_t blocks = cdiv64(nvox, 256);
    hipLaunchKernelGGL(cc_relabel_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, (hipStream_t)stream,
                       labels, lut, n, out_labels, out_mask, (long long)nvox);
    return check_launch("cc_relabel");
}

extern "C" int dram_lobe_burden(const uint8_t* mask, const uint8_t* lobe, int64_t* counts, int64_t nvox, void* stream) {
    DRAM_REQUIRE(mask && lobe && counts, "lobe_burden: null pointer");
    DRAM_REQUIRE(nvox > 0 && nvox < (1LL << 31), "lobe_burden: nvox must be in 1 .. 2^31 - 1");
    hipStream_t st = (hipStream_t)stream;
    (void)hipMemsetAsync(counts, 0, 512 * sizeof(int64_t), st);
    const long long groups = aligned16(mask) && aligned16(lobe) ? nvox / 16 : 0;
    const int64_t want = cdiv64(groups > 0 ? groups : nvox, 256 * 8);          // ~8 groups (or elements) per thread
    hipLaunchKernelGGL(lobe_burden_kernel, dim3((unsigned)(want < 1 ? 1 : (want > 4096 ? 4096 : want))), dim3(256), 0, st, mask, lobe,
                       (unsigned long long*)counts, (long long)nvox, groups);
    return check_launch("lobe_burden");
}
