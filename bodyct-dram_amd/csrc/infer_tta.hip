// Test-time augmentation around the model call of the per-lobe inference (include/dram_hip.h, "test-time augmentation"), gfx950.
//   tta_expand       every signed-permutation view of every R^3 chunk in one launch (data movement only)
//   tta_combine      mean and population standard deviation over the views of sigmoid(dense), at the chunk's resolution, one pass
//   lobe_paste_prob  the paste of infer.hip without the sigmoid, for one or two fields in one walk over the crop
//
// A view reads a chunk along another axis than it writes, so one side of a plain gather (dram_spatial_permute_flip,
// resample.hip: contiguous stores, loads with a lane stride of the moved axis) runs at a lane stride of R or R^2 floats.  That
// is harmless for one cache-resident chunk; the ensemble reads V * L chunks, so here a block owns one TZ x TY x TX box of the
// CANONICAL grid, walks it in each view's own order -- the view's contiguous axis fastest, so global accesses are runs of TX
// (x) or TZ / TY (z, y) consecutive floats, ascending or descending -- and turns it through a padded LDS image of the box.
// A view that keeps x in place needs no turn: the canonical walk already runs along its rows.
#include "lobe_chunk.h"

namespace dram {

constexpr int TTA_TZ = 8, TTA_TY = 8, TTA_TX = 16;          // the box a block owns, canonical (z, y, x)
constexpr int TTA_BOX = TTA_TZ * TTA_TY * TTA_TX;           // 1024 points
constexpr int TTA_THREADS = 512;
constexpr int TTA_PER = TTA_BOX / TTA_THREADS;              // points per thread
constexpr int TTA_SY = TTA_TX + 1;                          // LDS image strides: a walk along y (17) or z (137) touches
constexpr int TTA_SZ = TTA_TY * TTA_SY + 1;                 // eight different banks, a walk along x sixteen
constexpr int TTA_IMG = TTA_TZ * TTA_SZ;
constexpr int TTA_GROUP = 4;                                // views staged per pair of barriers

struct TtaView {
    int p0, p1, p2;     // view axis k reads canonical axis p_k
    int f0, f1, f2;
};
// per view: perm[k] in bits 2k, 2k+1; flip[k] in bit 6 + k
struct TtaViews {
    unsigned short code[DRAM_TTA_MAX_VIEWS];
};
__device__ __forceinline__ TtaView tta_decode(unsigned c) {
    return TtaView{(int)(c & 3u), (int)((c >> 2) & 3u), (int)((c >> 4) & 3u), (int)((c >> 6) & 1u), (int)((c >> 7) & 1u), (int)((c >> 8) & 1u)};
}
__device__ __forceinline__ int tta_pick(int a, int v0, int v1, int v2) { return a == 0 ? v0 : a == 1 ? v1 : v2; }

// Element j of the box in the order of a view whose axes read canonical axes (p0, p1, p2), the last fastest -> its canonical
// offsets inside the box.  With (0, 1, 2) this is the canonical order itself.
__device__ __forceinline__ void tta_box_point(int j, int p0, int p1, int p2, int& cz, int& cy, int& cx) {
    const int s2 = p2 == 2 ? 4 : 3, s1 = p1 == 2 ? 4 : 3;                 // log2 of the box extent along that canonical axis
    const int t2 = j & ((1 << s2) - 1), t1 = (j >> s2) & ((1 << s1) - 1), t0 = j >> (s2 + s1);
    cz = p0 == 0 ? t0 : p1 == 0 ? t1 : t2;
    cy = p0 == 1 ? t0 : p1 == 1 ? t1 : t2;
    cx = p0 == 2 ? t0 : p1 == 2 ? t1 : t2;
}
// Where view w shows canonical point (z, y, x): o[k] = flip[k] ? R-1-i[perm[k]] : i[perm[k]]
__device__ __forceinline__ int tta_view_offset(const TtaView& w, int z, int y, int x, int R) {
    const int i0 = tta_pick(w.p0, z, y, x), i1 = tta_pick(w.p1, z, y, x), i2 = tta_pick(w.p2, z, y, x);
    const int o0 = w.f0 ? R - 1 - i0 : i0, o1 = w.f1 ? R - 1 - i1 : i1, o2 = w.f2 ? R - 1 - i2 : i2;
    return (o0 * R + o1) * R + o2;
}
__device__ __forceinline__ int tta_img(int cz, int cy, int cx) { return cz * TTA_SZ + cy * TTA_SY + cx; }

struct TtaBox {
    int bz, by, bx;
};
__device__ __forceinline__ TtaBox tta_box_of_block(int R) {
    const int nx = (R + TTA_TX - 1) / TTA_TX, ny = (R + TTA_TY - 1) / TTA_TY;
    const int b = blockIdx.x;
    return TtaBox{(b / (nx * ny)) * TTA_TZ, ((b / nx) % ny) * TTA_TY, (b % nx) * TTA_TX};
}

// xv[v][l][o] = x[l][i]; grid (boxes, V * L)
__global__ __launch_bounds__(TTA_THREADS) void tta_expand_kernel(const float* __restrict__ x, float* __restrict__ xv, TtaViews tv,
                                                                 int L, int R) {
    __shared__ float img[TTA_IMG];
    const int v = blockIdx.y / L, l = blockIdx.y % L;
    const TtaView w = tta_decode(tv.code[v]);
    const TtaBox b = tta_box_of_block(R);
    const size_t S = (size_t)R * R * R;
    const float* src = x + (size_t)l * S;
    float* dst = xv + (size_t)blockIdx.y * S;
    const bool turn = w.p2 != 2;                                           // block-uniform
#pragma unroll
    for (int r = 0; r < TTA_PER; ++r) {
        int cz, cy, cx;
        tta_box_point((int)threadIdx.x + r * TTA_THREADS, 0, 1, 2, cz, cy, cx);
        const int z = b.bz + cz, y = b.by + cy, xx = b.bx + cx;
        if (z < R && y < R && xx < R) {
            const float val = src[(z * R + y) * R + xx];
            if (turn) img[tta_img(cz, cy, cx)] = val;
            else dst[tta_view_offset(w, z, y, xx, R)] = val;
        }
    }
    if (!turn) return;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < TTA_PER; ++r) {
        int cz, cy, cx;
        tta_box_point((int)threadIdx.x + r * TTA_THREADS, w.p0, w.p1, w.p2, cz, cy, cx);
        const int z = b.bz + cz, y = b.by + cy, xx = b.bx + cx;
        if (z < R && y < R && xx < R) dst[tta_view_offset(w, z, y, xx, R)] = img[tta_img(cz, cy, cx)];
    }
}

// term(0) + ... + term(V-1) over the binary tree of the view index (include/dram_hip.h): views 2j and 2j+1 first, then pairs of
// pairs, earlier views on the left; the complete blocks that V's binary digits leave over are joined from the last one upwards.
// A binary counter of partial sums, one per level; v is a constant once the loop is unrolled, so every branch on it folds.
constexpr int TTA_LEVELS = 6;                               // 2^6 > DRAM_TTA_MAX_VIEWS
template <int VCAP, typename Term>
__device__ __forceinline__ float tta_tree_sum(int V, Term term) {
    float part[TTA_LEVELS];
#pragma unroll
    for (int v = 0; v < VCAP; ++v) {
        if (v < V) {
            float c = term(v);
            bool placed = false;
#pragma unroll
            for (int b = 0; b < TTA_LEVELS; ++b) {
                if (placed) continue;
                if ((v >> b) & 1) c = __fadd_rn(part[b], c);
                else { part[b] = c; placed = true; }
            }
        }
    }
    float acc = 0.f;
    bool have = false;
#pragma unroll
    for (int b = 0; b < TTA_LEVELS; ++b)
        if ((V >> b) & 1) {
            acc = have ? __fadd_rn(part[b], acc) : part[b];
            have = true;
        }
    return acc;
}

// mean[l][i] = (p_0 + ... + p_{V-1}) / V, spread[l][i] = sqrt(((p_0 - m)^2 + ...) / V), p_v = sigmoid(dense[v][l][o_v(i)]): both
// sums by tta_tree_sum, no fused multiply-add.  grid (boxes, L).  The V probabilities of a point stay in registers (VCAP of
// them: the loops over views are unrolled so that every index is a constant).
template <int VCAP>
__global__ __launch_bounds__(TTA_THREADS) void tta_combine_kernel(const float* __restrict__ dense, float* __restrict__ mean,
                                                                  float* __restrict__ spread, TtaViews tv, int V, int L, int R) {
    __shared__ float img[TTA_GROUP][TTA_IMG];
    const int l = blockIdx.y;
    const TtaBox b = tta_box_of_block(R);
    const size_t S = (size_t)R * R * R;
    int z[TTA_PER], y[TTA_PER], xx[TTA_PER], at[TTA_PER];
    bool ok[TTA_PER];
#pragma unroll
    for (int r = 0; r < TTA_PER; ++r) {
        int cz, cy, cx;
        tta_box_point((int)threadIdx.x + r * TTA_THREADS, 0, 1, 2, cz, cy, cx);
        z[r] = b.bz + cz; y[r] = b.by + cy; xx[r] = b.bx + cx;
        at[r] = tta_img(cz, cy, cx);
        ok[r] = z[r] < R && y[r] < R && xx[r] < R;
    }
    float p[TTA_PER][VCAP];
#pragma unroll
    for (int g = 0; g < VCAP; g += TTA_GROUP) {
        if (g >= V) continue;                                              // block-uniform
        float ld[TTA_GROUP][TTA_PER];
        int to[TTA_GROUP][TTA_PER];
#pragma unroll
        for (int u = 0; u < TTA_GROUP; ++u) {
            if (g + u >= V) continue;
            const TtaView w = tta_decode(tv.code[g + u]);
            const float* src = dense + ((size_t)(g + u) * L + l) * S;
#pragma unroll
            for (int r = 0; r < TTA_PER; ++r) {
                ld[u][r] = 0.f;
                to[u][r] = -1;
                if (w.p2 == 2) {                                           // x stays x: this thread's own points, along the row
                    if (ok[r]) ld[u][r] = src[tta_view_offset(w, z[r], y[r], xx[r], R)];
                } else {                                                   // the box in the view's order, into the LDS image
                    int cz, cy, cx;
                    tta_box_point((int)threadIdx.x + r * TTA_THREADS, w.p0, w.p1, w.p2, cz, cy, cx);
                    const int zz = b.bz + cz, yy = b.by + cy, xc = b.bx + cx;
                    if (zz < R && yy < R && xc < R) {
                        ld[u][r] = src[tta_view_offset(w, zz, yy, xc, R)];
                        to[u][r] = tta_img(cz, cy, cx);
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < TTA_GROUP; ++u)
#pragma unroll
            for (int r = 0; r < TTA_PER; ++r)
                if (g + u < V && to[u][r] >= 0) img[u][to[u][r]] = ld[u][r];
        __syncthreads();
#pragma unroll
        for (int u = 0; u < TTA_GROUP; ++u) {
            if (g + u >= V) continue;
            const bool turn = ((tv.code[g + u] >> 4) & 3u) != 2u;
#pragma unroll
            for (int r = 0; r < TTA_PER; ++r) {
                const float d = turn ? (ok[r] ? img[u][at[r]] : 0.f) : ld[u][r];
                p[r][g + u] = paste_sigmoid(d);
            }
        }
        __syncthreads();
    }
    const float fv = (float)V;
#pragma unroll
    for (int r = 0; r < TTA_PER; ++r) {
        if (!ok[r]) continue;
        const float m = __fdiv_rn(tta_tree_sum<VCAP>(V, [&](int v) { return p[r][v]; }), fv);
        const size_t o = (size_t)l * S + (size_t)((z[r] * R + y[r]) * R + xx[r]);
        mean[o] = m;
        if (spread) {
            const float q = tta_tree_sum<VCAP>(V, [&](int v) {
                const float e = __fsub_rn(p[r][v], m);
                return __fmul_rn(e, e);
            });
            spread[o] = sqrtf(__fdiv_rn(q, fv));
        }
    }
}

// crop_voxel's walk pasting fields that are probabilities already; prob2 / htp2 (both or neither) ride along on the same taps.
__global__ __launch_bounds__(256) void lobe_paste_prob_kernel(const float* __restrict__ prob, const float* __restrict__ prob2,
                                                              const uint8_t* __restrict__ lobe, float* __restrict__ htp,
                                                              float* __restrict__ htp2, ChunkList cl, int H, int W, int R) {
    const CropVoxel v = crop_voxel(cl, lobe, H, W);
    if (!v.mine) return;
    const Trilinear t(R, v.c, v.z, v.y, v.x);
    htp[v.o] = t.combine(ChunkField{prob + (size_t)v.l * R * R * R, R});
    if (prob2) htp2[v.o] = t.combine(ChunkField{prob2 + (size_t)v.l * R * R * R, R});
}

// views: host array of V x {perm[3], flip[3]}
static int fill_views(const char* who, TtaViews& tv, const int* views, int V) {
    DRAM_REQUIRE(views, "%s: null view table", who);
    DRAM_REQUIRE(V >= 1 && V <= DRAM_TTA_MAX_VIEWS, "%s: between 1 and %d views", who, DRAM_TTA_MAX_VIEWS);
    for (int v = 0; v < V; ++v) {
        const int* q = views + 6 * v;
        int seen = 0;
        unsigned code = 0;
        for (int k = 0; k < 3; ++k) {
            DRAM_REQUIRE(q[k] >= 0 && q[k] < 3, "%s: view %d: perm must be a permutation of 0,1,2", who, v);
            DRAM_REQUIRE(q[3 + k] == 0 || q[3 + k] == 1, "%s: view %d: flip must be 0 or 1", who, v);
            seen |= 1 << q[k];
            code |= (unsigned)q[k] << (2 * k) | (unsigned)q[3 + k] << (6 + k);
        }
        DRAM_REQUIRE(seen == 7, "%s: view %d: perm must be a permutation of 0,1,2", who, v);
        tv.code[v] = (unsigned short)code;
    }
    for (int v = V; v < DRAM_TTA_MAX_VIEWS; ++v) tv.code[v] = (unsigned short)(0u | 1u << 2 | 2u << 4);
    return DRAM_OK;
}

static int check_chunk_grid(const char* who, int L, int R) {
    DRAM_REQUIRE(L >= 1 && L <= MAX_CHUNKS, "%s: between 1 and %d chunks", who, MAX_CHUNKS);
    DRAM_REQUIRE(R >= 2 && R <= 1024, "%s: R must be in 2..1024", who);       // R^3 < 2^31: offsets inside a chunk are ints
    return DRAM_OK;
}
static unsigned tta_boxes(int R) { return (unsigned)(cdiv(R, TTA_TZ) * cdiv(R, TTA_TY) * cdiv(R, TTA_TX)); }

}  // namespace dram

using namespace dram;

extern "C" int dram_tta_expand(const float* x, float* xv, int L, int R, const int* views, int V, void* stream) {
    DRAM_REQUIRE(x && xv, "tta_expand: null pointer");
    int rc = check_chunk_grid("tta_expand", L, R);
    if (rc) return rc;
    TtaViews tv;
    rc = fill_views("tta_expand", tv, views, V);
    if (rc) return rc;
    hipLaunchKernelGGL(tta_expand_kernel, dim3(tta_boxes(R), V * L), dim3(TTA_THREADS), 0, (hipStream_t)stream, x, xv, tv, L, R);
    return check_launch("tta_expand");
}

extern "C" int dram_tta_combine(const float* dense, float* mean, float* spread, int L, int R, const int* views, int V,
                                void* stream) {
    DRAM_REQUIRE(dense && mean, "tta_combine: null pointer");
    int rc = check_chunk_grid("tta_combine", L, R);
    if (rc) return rc;
    TtaViews tv;
    rc = fill_views("tta_combine", tv, views, V);
    if (rc) return rc;
    const dim3 grid(tta_boxes(R), L), block(TTA_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (V <= 8) hipLaunchKernelGGL(tta_combine_kernel<8>, grid, block, 0, st, dense, mean, spread, tv, V, L, R);
    else hipLaunchKernelGGL(tta_combine_kernel<DRAM_TTA_MAX_VIEWS>, grid, block, 0, st, dense, mean, spread, tv, V, L, R);
    return check_launch("tta_combine");
}

extern "C" int dram_lobe_paste_prob(const float* prob, const float* prob2, const uint8_t* lobe, float* htp, float* htp2,
                                    const int* chunks, int L, int D, int H, int W, int R, void* stream) {
    DRAM_REQUIRE(prob && lobe && htp, "lobe_paste_prob: null pointer");
    DRAM_REQUIRE((prob2 == nullptr) == (htp2 == nullptr), "lobe_paste_prob: prob2 and htp2 go together");
    DRAM_REQUIRE(R >= 2, "lobe_paste_prob: bad resample size");
    ChunkList cl;
    dim3 grid;
    const int rc = crop_grid("lobe_paste_prob", cl, grid, chunks, L, D, H, W);
    if (rc) return rc;
    hipLaunchKernelGGL(lobe_paste_prob_kernel, grid, dim3(256), 0, (hipStream_t)stream, prob, prob2, lobe, htp, htp2, cl, H, W, R);
    return check_launch("lobe_paste_prob");
}
