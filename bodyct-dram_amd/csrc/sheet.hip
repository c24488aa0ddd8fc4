// Result contact sheet (gfx950): which planes the zoomed coordinate mask occupies, and the finished sheet in one launch.  The
// definition -- flip, zoom, pad, layout, the 8-bit sources and the two drawing styles -- is in include/dram_hip.h ("result contact
// sheet"); this file is the kernels.
//
// The reference zooms six whole volumes to keep five planes of each.  Along the coordinate axis its zoom is the identity, so a
// plane of the result depends on that plane of the source alone: here nothing is zoomed or materialised.
//   sheet_occupancy_kernel  the one volume-sized pass.  Works in the SOURCE grid: a row (z, y) is read when the order-0 zoom
//                           samples its z and its y, as whole words along x, and the bytes of a word that the zoom skips are
//                           masked by a per-block table in LDS (they share the row's cache lines anyway).  A block owns one
//                           index of the flag axis -- or, for coord_axis 2, where a lane's bytes are the flags, one z -- and 32
//                           indices of the other row axis; a wave reads 256 consecutive bytes of a row per step in all three
//                           cases.
//   sheet_render_kernel     one thread per sheet pixel: it decodes column, row of tiles and tile pixel, undoes pad, zoom and flip
//                           and reads its taps -- four windowed-on-load sources for the fp64 lerp of the image, one nearest voxel
//                           per layer (five for an outline).  The colour table is rebuilt per block in LDS from its closed form.
#include <math.h>
#include "volume_math.h"

#pragma clang fp contract(off)

namespace dram {

// One axis of the volume: extent n, zoomed extent zn (n without a zoom), the zoom's step (1 without, 0 for zn == 1), whether the
// flip runs along it, and the zeros in front of the zoomed extent inside a tile.
struct SheetAxis {
    int n, zn, flip, pad;
    double step;
};

// Order 0: the index in the source volume (flip undone) that output index o reads, -1 when it reads nothing.
__device__ __forceinline__ int axis_nearest(const SheetAxis& a, int o) {
    const double c = (double)o * a.step;
    if (c > (double)(a.n - 1)) return -1;
    int i = (int)floor(c + 0.5);
    i = i > a.n - 1 ? a.n - 1 : i;
    return a.flip ? a.n - 1 - i : i;
}

// Does the order-0 zoom read index i (counted in the flipped volume)?  The output index nearest to i / step and its two neighbours
// are put through the forward map: for step >= 1 the one reader lies within 0.5 / step of i / step, for step < 1 the readers are
// consecutive and the nearest is one of them.
__device__ __forceinline__ bool axis_samples(const SheetAxis& a, int i) {
    const int oc = a.step > 0.0 ? (int)floor((double)i / a.step + 0.5) : 0;
    for (int o = oc - 1; o <= oc + 1; ++o) {
        if (o < 0 || o >= a.zn) continue;
        const double c = (double)o * a.step;
        if (c > (double)(a.n - 1)) continue;
        int j = (int)floor(c + 0.5);
        j = j > a.n - 1 ? a.n - 1 : j;
        if (j == i) return true;
    }
    return false;
}

// ---------------------------------------------------------------------------------------------------------------- occupancy
constexpr int OC_ROWS = 32;                  // rows per block, 8 per wave

struct OccArgs {
    const uint8_t* m[DRAM_SHEET_MAX_MASKS];
    int nm, ca;
    SheetAxis ax[3];
    int* flags;
    int chunks;                              // blocks per index of the block's fixed axis
};

// Block (64, 4).  blockIdx.x = f * chunks + chunk: f an index of the fixed axis (axis 1 for ca == 1, else axis 0), chunk 32
// consecutive indices of the other row axis; all counted in the flipped volume.  T: uint32_t (W % 4 == 0, 4-byte aligned masks) or
// uint8_t.  sel: T-sized pieces of the row, 0xFF in every byte whose x the zoom samples.
template <typename T>
__global__ __launch_bounds__(256) void sheet_occupancy_kernel(OccArgs a) {
    extern __shared__ uint32_t sel32[];
    uint8_t* sel8 = reinterpret_cast<uint8_t*>(sel32);
    const int W = a.ax[2].n, H = a.ax[1].n;
    const int tid = threadIdx.y * 64 + threadIdx.x;
    const int f = blockIdx.x / a.chunks, r0 = (int)(blockIdx.x % a.chunks) * OC_ROWS;
    const int fixed = a.ca == 1 ? 1 : 0, moving = 1 - fixed;
    if (a.ca == 2 && !axis_samples(a.ax[0], f)) return;       // block-uniform: a z that the zoom skips
    for (int c = tid; c < (W + 3) / 4; c += 256) sel32[c] = 0;
    __syncthreads();
    for (int o = tid; o < a.ax[2].zn; o += 256) {
        const int x = axis_nearest(a.ax[2], o);
        if (x >= 0) sel8[x] = 0xFF;
    }
    __syncthreads();
    const SheetAxis& fa = a.ax[fixed];
    const SheetAxis& ma = a.ax[moving];
    const int fsrc = fa.flip ? fa.n - 1 - f : f;
    long long base[OC_ROWS / 4];                              // the rows of this wave; -1: outside, or skipped by the zoom
#pragma unroll
    for (int k = 0; k < OC_ROWS / 4; ++k) {
        const int e = r0 + 4 * k + threadIdx.y;
        base[k] = -1;
        if (e < ma.n && axis_samples(ma, e)) {
            const int msrc = ma.flip ? ma.n - 1 - e : e;
            const int z = fixed == 0 ? fsrc : msrc, y = fixed == 0 ? msrc : fsrc;
            base[k] = ((long long)z * H + y) * W;
        }
    }
    constexpr int PER = (int)sizeof(T);
    const T* sel = reinterpret_cast<const T*>(sel32);
    const int pieces = W / PER;
    unsigned any = 0;
    for (int c = threadIdx.x; c < pieces; c += 64) {
        const T keep = sel[c];
        if (!keep) continue;
        unsigned acc = 0;
#pragma unroll
        for (int k = 0; k < OC_ROWS / 4; ++k) {
            if (base[k] < 0) continue;
            for (int q = 0; q < a.nm; ++q) acc |= reinterpret_cast<const T*>(a.m[q] + base[k])[c];
        }
        acc &= keep;
        if (a.ca == 2) {                                      // this lane's bytes are flags of their own
            for (int j = 0; j < PER; ++j)
                if ((acc >> (8 * j)) & 0xFFu) {
                    const int x = c * PER + j;
                    a.flags[a.ax[2].flip ? W - 1 - x : x] = 1;
                }
        } else {
            any |= acc;
        }
    }
    if (a.ca != 2 && __any(any != 0) && threadIdx.x == 0) a.flags[f] = 1;
}

// ---------------------------------------------------------------------------------------------------------------- render
struct SheetLayer {
    const void* data;
    int kind, thickness;
    unsigned char color[4];
};
static_assert(sizeof(SheetLayer) == sizeof(dram_sheet_layer), "the launch copies dram_sheet_layer field by field into this");

struct SheetArgs {
    const void* image;
    int image_kind, wmin, wmax;
    SheetAxis ax[3];
    int ca, aa, ab;                          // tile rows run along aa, tile columns along ab
    long long stride[3];
    int th, tw, n_rows, num_slices, left, Hs, Ws, style, cmap;
    float alpha, beta;
    int plane[DRAM_SHEET_MAX_SLICES];        // the SOURCE plane of every column (flip undone)
    int row_first[DRAM_SHEET_MAX_ROWS + 1];
    SheetLayer layer[DRAM_SHEET_MAX_LAYERS];
    uint8_t* sheet;
};

__device__ __forceinline__ double image_source(const SheetArgs& a, long long at) {
    if (a.image_kind == DRAM_SHEET_U8) return (double)((const uint8_t*)a.image)[at];
    return (double)(uint8_t)scan_bin(windowed_scan(((const int16_t*)a.image)[at], a.wmin, a.wmax));
}

__device__ __forceinline__ int layer_source(const SheetLayer& l, long long at) {
    if (l.kind == DRAM_SHEET_MASK) return ((const uint8_t*)l.data)[at] ? 255 : 0;
    if (l.kind == DRAM_SHEET_U8) return ((const uint8_t*)l.data)[at];
    const float h = ((const float*)l.data)[at];
    if (h != h) return 0;
    float w = h < 0.f ? 0.f : (h > 1.f ? 1.f : h);
    w = (w - 0.f) / 1.f * 255.f + 0.f;
    return (int)w;
}

// The grey value at tile pixel (ty, tx) of the column whose source plane is `plane`.
__device__ __forceinline__ int image_pixel(const SheetArgs& a, int ty, int tx, int plane) {
    const SheetAxis& A = a.ax[a.aa];
    const SheetAxis& B = a.ax[a.ab];
    const int i = ty - A.pad, j = tx - B.pad;
    if (i < 0 || i >= A.zn || j < 0 || j >= B.zn) return 0;
    const double ca = (double)i * A.step, cb = (double)j * B.step;
    if (ca > (double)(A.n - 1) || cb > (double)(B.n - 1)) return 0;
    int a0 = (int)floor(ca), b0 = (int)floor(cb);
    a0 = a0 > A.n - 1 ? A.n - 1 : a0;
    b0 = b0 > B.n - 1 ? B.n - 1 : b0;
    const int a1 = a0 + 1 > A.n - 1 ? A.n - 1 : a0 + 1, b1 = b0 + 1 > B.n - 1 ? B.n - 1 : b0 + 1;
    const double ta = ca - (double)a0, tb = cb - (double)b0;
    const long long p = (long long)plane * a.stride[a.ca];
    const long long ra0 = (A.flip ? A.n - 1 - a0 : a0) * a.stride[a.aa], ra1 = (A.flip ? A.n - 1 - a1 : a1) * a.stride[a.aa];
    const long long rb0 = (B.flip ? B.n - 1 - b0 : b0) * a.stride[a.ab], rb1 = (B.flip ? B.n - 1 - b1 : b1) * a.stride[a.ab];
    const double v00 = image_source(a, p + ra0 + rb0), v10 = image_source(a, p + ra1 + rb0);
    const double v01 = image_source(a, p + ra0 + rb1), v11 = image_source(a, p + ra1 + rb1);
    const double u0 = v00 * (1.0 - ta) + v10 * ta;            // along aa first (the lower axis), unrounded
    const double u1 = v01 * (1.0 - ta) + v11 * ta;
    const double v = u0 * (1.0 - tb) + u1 * tb;
    return (int)floor(v + 0.5);
}

// The 8-bit value of a layer at tile pixel (ty, tx); 0 in the pad, outside the tile and where the zoom reads nothing.
__device__ __forceinline__ int layer_pixel(const SheetArgs& a, const SheetLayer& l, int ty, int tx, int plane) {
    const SheetAxis& A = a.ax[a.aa];
    const SheetAxis& B = a.ax[a.ab];
    const int i = ty - A.pad, j = tx - B.pad;
    if (i < 0 || i >= A.zn || j < 0 || j >= B.zn) return 0;
    const int ia = axis_nearest(A, i), ib = axis_nearest(B, j);
    if (ia < 0 || ib < 0) return 0;
    return layer_source(l, (long long)plane * a.stride[a.ca] + ia * a.stride[a.aa] + ib * a.stride[a.ab]);
}

__device__ __forceinline__ int blend(int x, int y, float alpha, float beta) {
    const float p = (float)x * alpha, q = (float)y * beta;
    float s = rintf(p + q);
    s = s < 0.f ? 0.f : (s > 255.f ? 255.f : s);
    return (int)s;
}

__device__ __forceinline__ int rne255(double c) { return (int)rint(255.0 * c); }

// Grid (cdiv(Ws, 256), Hs), block 256: one sheet pixel per thread.
__global__ __launch_bounds__(256) void sheet_render_kernel(SheetArgs a) {
    __shared__ unsigned char lut[256][4];
    if (a.style == DRAM_SHEET_HEATMAP) {
        const double t = (double)threadIdx.x / 255.0;
        for (int ch = 0; ch < 3; ++ch) {
            double c;
            if (a.cmap == DRAM_SHEET_JET) {
                c = 1.5 - fabs(4.0 * t - (double)(3 - ch));
                c = c < 0.0 ? 0.0 : (c > 1.0 ? 1.0 : c);
            } else {
                c = ch == 0 ? t : (ch == 1 ? 0.5 + 0.5 * t : 0.4);
            }
            lut[threadIdx.x][ch] = (unsigned char)rne255(c);
        }
        __syncthreads();
    }
    const int X = blockIdx.x * 256 + threadIdx.x, Y = blockIdx.y;
    if (X >= a.Ws) return;
    int v[3] = {0, 0, 0};
    const int xin = X - a.left;
    if (xin >= 0 && xin < a.num_slices * a.tw) {
        const int col = xin / a.tw, tx = xin % a.tw, trow = Y / a.th, ty = Y % a.th;
        const int plane = a.plane[col];
        const int grey = image_pixel(a, ty, tx, plane);
        v[0] = v[1] = v[2] = grey;
        if (trow > 0) {
            const int first = a.row_first[trow - 1], last = a.row_first[trow];
            if (a.style == DRAM_SHEET_HEATMAP) {
                for (int k = first; k < last; ++k) {
                    const int lv = layer_pixel(a, a.layer[k], ty, tx, plane);
                    for (int ch = 0; ch < 3; ++ch) v[ch] = blend(lut[lv][ch], v[ch], a.alpha, a.beta);
                }
            } else {
                int painted[3] = {grey, grey, grey};
                for (int k = first; k < last; ++k) {
                    const SheetLayer& l = a.layer[k];
                    bool paint = layer_pixel(a, l, ty, tx, plane) != 0;
                    if (paint && l.thickness == 1) {          // an outline pixel: a 4-neighbour that is zero or outside the tile
                        const bool inner = ty > 0 && ty < a.th - 1 && tx > 0 && tx < a.tw - 1 &&
                                           layer_pixel(a, l, ty - 1, tx, plane) != 0 && layer_pixel(a, l, ty + 1, tx, plane) != 0 &&
                                           layer_pixel(a, l, ty, tx - 1, plane) != 0 && layer_pixel(a, l, ty, tx + 1, plane) != 0;
                        paint = !inner;
                    }
                    if (paint)
                        for (int ch = 0; ch < 3; ++ch) painted[ch] = l.color[ch];
                }
                for (int ch = 0; ch < 3; ++ch) v[ch] = blend(painted[ch], grey, a.alpha, a.beta);
            }
        }
    }
    uint8_t* out = a.sheet + ((long long)Y * a.Ws + X) * 3;
    out[0] = (uint8_t)v[0];
    out[1] = (uint8_t)v[1];
    out[2] = (uint8_t)v[2];
}

// The axes of a call; 0, or DRAM_EINVAL with the error set.
static int sheet_axes(const char* who, int D, int H, int W, int coord_axis, int flip_axis, int zoom_size, SheetAxis* ax) {
    DRAM_REQUIRE(D > 0 && H > 0 && W > 0 && (long long)D * H * W < (1LL << 31), "%s: sizes must be positive with D*H*W < 2^31", who);
    DRAM_REQUIRE(coord_axis >= 0 && coord_axis <= 2, "%s: coord_axis must be 0, 1 or 2", who);
    DRAM_REQUIRE(flip_axis >= -1 && flip_axis <= 2, "%s: flip_axis must be 0, 1, 2 or -1 for none", who);
    DRAM_REQUIRE(zoom_size >= 0, "%s: zoom_size must be positive, or 0 for none", who);
    const int n[3] = {D, H, W};
    int longest = 0;
    for (int d = 0; d < 3; ++d)
        if (d != coord_axis && n[d] > longest) longest = n[d];
    const double ratio = zoom_size > 0 ? (double)zoom_size / (double)longest : 1.0;
    for (int d = 0; d < 3; ++d) {
        SheetAxis& a = ax[d];
        a.n = n[d];
        a.flip = flip_axis == d;
        a.zn = n[d];
        a.step = 1.0;
        a.pad = 0;
        if (d == coord_axis || zoom_size == 0) continue;
        const double scaled = (double)n[d] * ratio;
        a.zn = (int)nearbyint(scaled);                         // round half to even, like Python's round
        DRAM_REQUIRE(a.zn >= 1 && a.zn <= zoom_size, "%s: axis %d of %d voxels zooms to an extent of %d", who, d, n[d], a.zn);
        a.step = a.zn > 1 ? (double)(n[d] - 1) / (double)(a.zn - 1) : 0.0;
        a.pad = (zoom_size - a.zn) / 2;
    }
    return DRAM_OK;
}

}  // namespace dram

using namespace dram;

extern "C" int dram_sheet_occupancy(const void* const* masks, int n_masks, int D, int H, int W, int coord_axis, int flip_axis,
                                    int zoom_size, int* flags, void* stream) {
    DRAM_REQUIRE(masks && flags, "sheet_occupancy: null pointer");
    DRAM_REQUIRE(n_masks >= 1 && n_masks <= DRAM_SHEET_MAX_MASKS, "sheet_occupancy: 1 .. %d masks", DRAM_SHEET_MAX_MASKS);
    OccArgs a;
    if (int rc = sheet_axes("sheet_occupancy", D, H, W, coord_axis, flip_axis, zoom_size, a.ax)) return rc;
    DRAM_REQUIRE(W <= DRAM_SHEET_MAX_W, "sheet_occupancy: W must not exceed %d", DRAM_SHEET_MAX_W);
    bool vec = W % 4 == 0;
    for (int q = 0; q < DRAM_SHEET_MAX_MASKS; ++q) {
        a.m[q] = q < n_masks ? (const uint8_t*)masks[q] : nullptr;
        DRAM_REQUIRE(q >= n_masks || a.m[q], "sheet_occupancy: null mask");
        if (q < n_masks && ((uintptr_t)a.m[q] & 3)) vec = false;
    }
    a.nm = n_masks;
    a.ca = coord_axis;
    a.flags = flags;
    const int n[3] = {D, H, W};
    const int fixed = coord_axis == 1 ? 1 : 0;
    a.chunks = cdiv(n[1 - fixed], OC_ROWS);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(flags, 0, sizeof(int) * (size_t)n[coord_axis], st) != hipSuccess) return check_launch("sheet_occupancy");
    const unsigned blocks = (unsigned)((long long)n[fixed] * a.chunks);          // <= D * H < 2^31
    const size_t lds = (size_t)cdiv(W, 4) * 4;
    if (vec)
        hipLaunchKernelGGL(sheet_occupancy_kernel<uint32_t>, dim3(blocks), dim3(64, 4), lds, st, a);
    else
        hipLaunchKernelGGL(sheet_occupancy_kernel<uint8_t>, dim3(blocks), dim3(64, 4), lds, st, a);
    return check_launch("sheet_occupancy");
}

extern "C" int dram_sheet_render(const void* image, int image_kind, int wmin, int wmax, const dram_sheet_layer* layers,
                                 const int* row_layers, int n_rows, const int* slice_ids, int num_slices, int D, int H, int W,
                                 int coord_axis, int flip_axis, int zoom_size, int sheet_width, int style, int colormap, double alpha,
                                 uint8_t* sheet, void* stream) {
    DRAM_REQUIRE(image && layers && row_layers && slice_ids && sheet, "sheet_render: null pointer");
    SheetArgs a;
    if (int rc = sheet_axes("sheet_render", D, H, W, coord_axis, flip_axis, zoom_size, a.ax)) return rc;
    DRAM_REQUIRE(image_kind == DRAM_SHEET_INT16 || image_kind == DRAM_SHEET_U8, "sheet_render: the image is DRAM_SHEET_INT16 or DRAM_SHEET_U8");
    if (image_kind == DRAM_SHEET_INT16) {
        DRAM_REQUIRE(wmax > wmin, "sheet_render: an int16 image needs a window with wmax > wmin");
        DRAM_REQUIRE(((uintptr_t)image & 1) == 0, "sheet_render: an int16 image must be 2-byte aligned");
    }
    DRAM_REQUIRE(style == DRAM_SHEET_HEATMAP || style == DRAM_SHEET_CONTOUR, "sheet_render: unknown style");
    DRAM_REQUIRE(style != DRAM_SHEET_HEATMAP || colormap == DRAM_SHEET_JET || colormap == DRAM_SHEET_SUMMER, "sheet_render: unknown colour map");
    DRAM_REQUIRE(alpha >= 0.0 && alpha <= 1.0, "sheet_render: alpha must lie in [0, 1]");
    DRAM_REQUIRE(n_rows >= 1 && n_rows <= DRAM_SHEET_MAX_ROWS, "sheet_render: 1 .. %d rows", DRAM_SHEET_MAX_ROWS);
    DRAM_REQUIRE(num_slices >= 1 && num_slices <= DRAM_SHEET_MAX_SLICES, "sheet_render: 1 .. %d slices", DRAM_SHEET_MAX_SLICES);
    const int n[3] = {D, H, W};
    int total = 0;
    a.row_first[0] = 0;
    for (int r = 0; r < n_rows; ++r) {
        DRAM_REQUIRE(row_layers[r] >= 1 && row_layers[r] <= DRAM_SHEET_MAX_LAYERS - total, "sheet_render: a row has 1 or more layers, all rows %d at most",
                     DRAM_SHEET_MAX_LAYERS);
        total += row_layers[r];
        a.row_first[r + 1] = total;
    }
    for (int r = n_rows + 1; r <= DRAM_SHEET_MAX_ROWS; ++r) a.row_first[r] = total;
    for (int k = 0; k < DRAM_SHEET_MAX_LAYERS; ++k) {
        SheetLayer& l = a.layer[k];
        l = SheetLayer{nullptr, DRAM_SHEET_MASK, -1, {0, 0, 0, 0}};
        if (k >= total) continue;
        const dram_sheet_layer& s = layers[k];
        DRAM_REQUIRE(s.data, "sheet_render: layer %d has no data", k);
        DRAM_REQUIRE(s.kind == DRAM_SHEET_MASK || s.kind == DRAM_SHEET_U8 || s.kind == DRAM_SHEET_UNIT, "sheet_render: layer %d has an unknown kind", k);
        DRAM_REQUIRE(s.kind != DRAM_SHEET_UNIT || ((uintptr_t)s.data & 3) == 0, "sheet_render: a float32 layer must be 4-byte aligned");
        DRAM_REQUIRE(style != DRAM_SHEET_CONTOUR || s.thickness == -1 || s.thickness == 1, "sheet_render: thickness must be -1 or 1");
        l.data = s.data;
        l.kind = s.kind;
        l.thickness = s.thickness;
        for (int c = 0; c < 4; ++c) l.color[c] = s.color[c];
    }
    for (int j = 0; j < DRAM_SHEET_MAX_SLICES; ++j) {
        a.plane[j] = 0;
        if (j >= num_slices) continue;
        DRAM_REQUIRE(slice_ids[j] >= 0 && slice_ids[j] < n[coord_axis], "sheet_render: slice id %d is outside 0 .. %d", slice_ids[j], n[coord_axis] - 1);
        a.plane[j] = flip_axis == coord_axis ? n[coord_axis] - 1 - slice_ids[j] : slice_ids[j];
    }
    a.ca = coord_axis;
    a.aa = coord_axis == 0 ? 1 : 0;
    a.ab = coord_axis == 2 ? 1 : 2;
    a.stride[0] = (long long)H * W;
    a.stride[1] = W;
    a.stride[2] = 1;
    a.th = zoom_size > 0 ? zoom_size : n[a.aa];
    a.tw = zoom_size > 0 ? zoom_size : n[a.ab];
    const long long cur = (long long)num_slices * a.tw, rows = (long long)(1 + n_rows) * a.th;
    DRAM_REQUIRE(sheet_width >= 0 && (sheet_width == 0 || cur <= sheet_width), "sheet_render: %d tiles of width %d do not fit a sheet of width %d",
                 num_slices, a.tw, sheet_width);
    const long long ws = sheet_width > 0 ? sheet_width : cur;
    DRAM_REQUIRE(ws * rows * 3 < (1LL << 31) && rows <= 65535, "sheet_render: the sheet is too large");
    a.Ws = (int)ws;
    a.Hs = (int)rows;
    a.left = (int)((ws - cur) / 2);
    a.n_rows = n_rows;
    a.num_slices = num_slices;
    a.image = image;
    a.image_kind = image_kind;
    a.wmin = wmin;
    a.wmax = wmax;
    a.style = style;
    a.cmap = colormap;
    a.alpha = (float)alpha;
    a.beta = (float)(1.0 - alpha);
    a.sheet = sheet;
    hipLaunchKernelGGL(sheet_render_kernel, dim3((unsigned)cdiv(a.Ws, 256), (unsigned)a.Hs), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch("sheet_render");
}
