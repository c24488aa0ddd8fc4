// RandomCrop(keep_size=True) on a device batch (gfx950): pad, crop and resample back to the chunk's size in one launch per tensor.
//
// The reference (dram/data_transforms.py:582-636) pads every "#" array with np.pad(mode=padding_mode) where the drawn window
// leaves the chunk, slices the window out and hands it to Resample('fixed_size', 1, data_shape) (data_transforms.py:170-175 ->
// utils.resample, utils.py:414-434): linear for the image, nearest neighbour for every "reference" / "weight_map" key, on the
// grid of sitk.ResampleImageFilter (volume_math.h).  Here the crop is never materialised: an output voxel
// maps to a crop index, the crop index plus the window's start is a chunk coordinate, and a coordinate outside the chunk takes the
// value np.pad would have put there:
//   'constant'  0
//   'edge'      the chunk's voxel at the clamped coordinate
//   'minimum'   np.pad pads axis by axis with the minimum along that axis of the array as padded so far, so a padded position
//               holds the minimum of the chunk over exactly the axes in which it lies outside, the other coordinates held fixed.
//               Those seven projections (over z, y, x, zy, zx, yx, zyx) come from a pre-pass, pad_min, into a workspace.
// Two entry points, neither of which synchronises, allocates or reads per-sample data from the host.
#include "volume_math.h"
#include <limits.h>
#include <math.h>

namespace dram {
namespace {

constexpr int PAD_MAX_DIM = 2048;       // H and W of pad_min (row / column minima of a slice in LDS)
constexpr int CROP_MAX_ROWS = 64;       // output rows (z, y) per block
constexpr int CROP_MAX_W = 2048;        // x table: 16 bytes per output column in dynamic LDS
constexpr int CROP_OUT = INT_MIN;       // table entry of an output position beyond the crop (ITK's default value 0)

struct CropRec {                        // 56 bytes, mirrored by dram_amd/augment.py:CROP_DTYPE
    int z0, y0, x0;                     // the window's first voxel in chunk coordinates (negative: the window starts in the pad)
    int cd, ch, cw;                     // the crop's actual size (numpy truncates a slice that runs past the padded array)
    int mode, pad;                      // DRAM_AUG_PAD_*
    double sz, sy, sx;                  // output-to-crop index step per axis (required_spacing / spacing)
};
static_assert(sizeof(CropRec) == 56, "CropRec is part of the ABI");

// ---------------------------------------------------------------- pad_min: the seven min projections of a sample
// Workspace of one sample, in elements of T: Pz [H][W] (min over z), Py [D][W], Px [D][H], Pzy [W], Pzx [H], Pyx [D], Pzyx [1].
struct PadLayout { int py, px, pzy, pzx, pyx, pzyx; size_t stride; };
inline __host__ __device__ PadLayout pad_layout(int D, int H, int W) {
    PadLayout l;
    l.py = H * W;
    l.px = l.py + D * W;
    l.pzy = l.px + D * H;
    l.pzx = l.pzy + W;
    l.pyx = l.pzx + H;
    l.pzyx = l.pyx + D;
    l.stride = ((size_t)l.pzyx + 1 + 3) / 4 * 4;
    return l;
}

// grid (D, N): a block owns one z-slice and reads it once.  Lanes are laid out (ty, tx) with tx over TX = 1 << lx consecutive
// columns (TX <= 64, a power of two: a row's TX lanes sit in one wave); a lane keeps the running minimum of its column, the TX
// lanes of a row reduce theirs with xor shuffles below TX (which stay inside the row's lanes), and both land in LDS through
// integer atomics.  Every lane runs every shuffle: positions past H or W contribute the top key.
template <typename T>
__global__ __launch_bounds__(256) void pad_slice_kernel(const T* __restrict__ x, T* __restrict__ ws, const int* __restrict__ flag,
                                                        int D, int H, int W, int lx) {
    __shared__ unsigned rowk[PAD_MAX_DIM], colk[PAD_MAX_DIM];
    const int n = blockIdx.y, z = blockIdx.x;
    if (flag[n] != 1) return;
    for (int i = threadIdx.x; i < H; i += 256) rowk[i] = KEY_TOP;
    for (int i = threadIdx.x; i < W; i += 256) colk[i] = KEY_TOP;
    __syncthreads();
    const T* sl = x + ((size_t)n * D + z) * H * W;
    const int TX = 1 << lx, TY = 256 >> lx;
    const int tx = threadIdx.x & (TX - 1), ty = threadIdx.x >> lx;
    for (int xb = 0; xb < W; xb += TX) {
        const int xx = xb + tx;
        unsigned ck = KEY_TOP;
        for (int yb = 0; yb < H; yb += TY) {
            const int yy = yb + ty;
            const bool in = xx < W && yy < H;
            const unsigned k = in ? Key<T>::enc(sl[(size_t)yy * W + xx]) : KEY_TOP;
            ck = umin_(ck, k);
            unsigned r = k;
            for (int o = TX >> 1; o > 0; o >>= 1) r = umin_(r, (unsigned)__shfl_xor((int)r, o, 64));
            if (tx == 0 && yy < H) atomicMin(&rowk[yy], r);
        }
        if (xx < W) atomicMin(&colk[xx], ck);
    }
    __syncthreads();
    const PadLayout l = pad_layout(D, H, W);
    T* w = ws + (size_t)n * l.stride;
    for (int i = threadIdx.x; i < H; i += 256) w[l.px + z * H + i] = Key<T>::dec(rowk[i]);
    for (int i = threadIdx.x; i < W; i += 256) w[l.py + z * W + i] = Key<T>::dec(colk[i]);
}

// grid (cdiv(H * W, 256), N): Pz, one lane per (y, x) column walking z (a second, coalesced read of the sample).
template <typename T>
__global__ __launch_bounds__(256) void pad_z_kernel(const T* __restrict__ x, T* __restrict__ ws, const int* __restrict__ flag,
                                                    int D, int H, int W) {
    const int n = blockIdx.y;
    if (flag[n] != 1) return;
    const int HW = H * W;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= HW) return;
    const T* s = x + (size_t)n * D * HW + i;
    unsigned k = KEY_TOP;
    for (int z = 0; z < D; ++z) k = umin_(k, Key<T>::enc(s[(size_t)z * HW]));
    ws[(size_t)n * pad_layout(D, H, W).stride + i] = Key<T>::dec(k);
}

// grid (N): the four projections over two and three axes from Px and Py (D * (H + W) elements: nothing next to the passes above).
template <typename T>
__global__ __launch_bounds__(256) void pad_edges_kernel(T* __restrict__ ws, const int* __restrict__ flag, int D, int H, int W) {
    __shared__ unsigned red[256];
    const int n = blockIdx.x;
    if (flag[n] != 1) return;
    const PadLayout l = pad_layout(D, H, W);
    T* w = ws + (size_t)n * l.stride;
    for (int i = threadIdx.x; i < W; i += 256) {
        unsigned k = KEY_TOP;
        for (int z = 0; z < D; ++z) k = umin_(k, Key<T>::enc(w[l.py + z * W + i]));
        w[l.pzy + i] = Key<T>::dec(k);
    }
    for (int i = threadIdx.x; i < H; i += 256) {
        unsigned k = KEY_TOP;
        for (int z = 0; z < D; ++z) k = umin_(k, Key<T>::enc(w[l.px + z * H + i]));
        w[l.pzx + i] = Key<T>::dec(k);
    }
    unsigned all = KEY_TOP;
    for (int z = threadIdx.x; z < D; z += 256) {
        unsigned k = KEY_TOP;
        for (int i = 0; i < H; ++i) k = umin_(k, Key<T>::enc(w[l.px + z * H + i]));
        w[l.pyx + z] = Key<T>::dec(k);
        all = umin_(all, k);
    }
    red[threadIdx.x] = all;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] = umin_(red[threadIdx.x], red[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) w[l.pzyx] = Key<T>::dec(red[0]);
}

// ---------------------------------------------------------------- crop_resample
struct CropX {                          // per output column
    int x0, x1;                         // chunk coordinates of the linear pair (nearest: both the nearest voxel); CROP_OUT: beyond the crop
    double tx;
};
struct CropRow {                        // per output row of the block
    int z0, z1, y0, y1;
    double tz, ty;
};
struct CropArgs {
    const void* x;
    void* y;
    const CropRec* table;
    const void* ws;                     // pad_min's workspace; may be null when no sample pads with 'minimum'
    const int* flag;
    int D, H, W, rows;
};

// One axis of the ITK grid (itk_axis, volume_math.h) in crop indices, c = o * step: the linear pair or, twice, the nearest voxel,
// shifted by the window's start to chunk coordinates.  'edge' clamps the chunk coordinate here, once per table entry, so that
// its fetches are plain reads.
template <bool LINEAR>
__device__ __forceinline__ void crop_axis(int o, double step, int size, int start, int dim, int mode, int& i0, int& i1, double& t) {
    const ItkAxis g = itk_axis(mul_rn((double)o, step), size);
    t = LINEAR ? g.t : 0.0;
    if (!g.inside) {                                           // (also NaN and an empty crop)
        i0 = i1 = CROP_OUT;
        return;
    }
    int a = (LINEAR ? g.lo : g.nearest) + start;
    int b = (LINEAR ? g.hi : g.nearest) + start;
    if (mode == DRAM_AUG_PAD_EDGE) {
        a = a < 0 ? 0 : (a > dim - 1 ? dim - 1 : a);
        b = b < 0 ? 0 : (b > dim - 1 ? dim - 1 : b);
    }
    i0 = a;
    i1 = b;
}

// grid (row tiles, N), 256 threads.  A block owns `rows` consecutive output rows (z, y) of one sample: a contiguous span of the
// output.  It fills the sample's x table and the z / y entries of its rows into LDS -- per block, not per voxel --, then walks its
// span in groups of 16 bytes aligned in the OUTPUT'S ADDRESS (the base's misalignment in elements is added to the element index
// before it is cut into groups): a group inside the span is one 16-byte store, the ragged ends go element by element, so any W
// and any base address take this one path.  Per output voxel: 8 source fetches (linear) or 1 (nearest), gathered through the
// caches; a fetch outside the chunk reads the pad value instead (file comment).  fp64 lerps along x, then y, then z (lerp_rn,
// volume_math.h), cast to the element type: the bits of oracle.resample_itk.
template <typename T, bool LINEAR>
__global__ __launch_bounds__(256) void crop_resample_kernel(CropArgs a) {
#pragma clang fp contract(off)
    constexpr int VEC = 16 / (int)sizeof(T);
    extern __shared__ __align__(16) unsigned char crop_lds[];
    CropX* xt = reinterpret_cast<CropX*>(crop_lds);
    __shared__ CropRow rt[CROP_MAX_ROWS];
    __shared__ int cs[8][4];            // pad value of a fetch outside in axes m (bit 2 = z, 1 = y, 0 = x): ws[base + z*sz + y*sy + x*sx]
    const int n = blockIdx.y;
    const int f = a.flag[n];
    if (f < 0) return;
    const int D = a.D, H = a.H, W = a.W;
    const int nrows_all = D * H;
    const int row0 = blockIdx.x * a.rows;
    const int nrows = nrows_all - row0 < a.rows ? nrows_all - row0 : a.rows;
    const T* src = static_cast<const T*>(a.x) + (size_t)n * nrows_all * W;
    T* out = static_cast<T*>(a.y);
    const size_t span0 = ((size_t)n * nrows_all + row0) * W, span1 = span0 + (size_t)nrows * W;
    const size_t mis = ((size_t)(uintptr_t)out / sizeof(T)) & (VEC - 1);
    const CropRec r = a.table[n];
    const T* ws = nullptr;
    if (f == 1) {
        const PadLayout l = pad_layout(D, H, W);
        if (a.ws && r.mode == DRAM_AUG_PAD_MINIMUM) ws = static_cast<const T*>(a.ws) + (size_t)n * l.stride;
        for (int xo = threadIdx.x; xo < W; xo += 256) {
            CropX q;
            crop_axis<LINEAR>(xo, r.sx, r.cw, r.x0, W, r.mode, q.x0, q.x1, q.tx);
            xt[xo] = q;
        }
        if ((int)threadIdx.x < nrows) {
            const int row = row0 + threadIdx.x;
            CropRow& p = rt[threadIdx.x];
            crop_axis<LINEAR>(row / H, r.sz, r.cd, r.z0, D, r.mode, p.z0, p.z1, p.tz);
            crop_axis<LINEAR>(row % H, r.sy, r.ch, r.y0, H, r.mode, p.y0, p.y1, p.ty);
        }
        if (threadIdx.x >= 248) {
            const int m = threadIdx.x - 248;                   // 1: Px[z][y]  2: Py[z][x]  3: Pyx[z]  4: Pz[y][x]  5: Pzx[y]  6: Pzy[x]  7: Pzyx
            cs[m][0] = m == 1 ? l.px : m == 2 ? l.py : m == 3 ? l.pyx : m == 5 ? l.pzx : m == 6 ? l.pzy : m == 7 ? l.pzyx : 0;
            cs[m][1] = m == 1 ? H : m == 2 ? W : m == 3 ? 1 : 0;
            cs[m][2] = m == 1 || m == 5 ? 1 : m == 4 ? W : 0;
            cs[m][3] = m == 2 || m == 4 || m == 6 ? 1 : 0;
        }
        __syncthreads();
    }

    auto fetch = [&](int z, int y, int x) -> T {
        const int m = ((unsigned)z >= (unsigned)D ? 4 : 0) | ((unsigned)y >= (unsigned)H ? 2 : 0) | ((unsigned)x >= (unsigned)W ? 1 : 0);
        if (m == 0) return src[((size_t)z * H + y) * W + x];
        if (!ws) return (T)0;                                  // 'constant' ('edge' never gets here: its coordinates are clamped)
        return ws[cs[m][0] + z * cs[m][1] + y * cs[m][2] + x * cs[m][3]];    // (a coordinate outside has stride 0)
    };
    auto voxel = [&](int lr, int x) -> T {
#pragma clang fp contract(off)
        const CropRow& p = rt[lr];
        const CropX q = xt[x];
        if (p.z0 == CROP_OUT || p.y0 == CROP_OUT || q.x0 == CROP_OUT) return (T)0;
        if (!LINEAR) return fetch(p.z0, p.y0, q.x0);
        const double v00 = lerp_rn((double)fetch(p.z0, p.y0, q.x0), (double)fetch(p.z0, p.y0, q.x1), q.tx);
        const double v01 = lerp_rn((double)fetch(p.z0, p.y1, q.x0), (double)fetch(p.z0, p.y1, q.x1), q.tx);
        const double v10 = lerp_rn((double)fetch(p.z1, p.y0, q.x0), (double)fetch(p.z1, p.y0, q.x1), q.tx);
        const double v11 = lerp_rn((double)fetch(p.z1, p.y1, q.x0), (double)fetch(p.z1, p.y1, q.x1), q.tx);
        return (T)lerp_rn(lerp_rn(v00, v01, p.ty), lerp_rn(v10, v11, p.ty), p.tz);
    };

    const T* same = static_cast<const T*>(a.x);                // a PASS sample: the same elements of x
    for (size_t g = (span0 + mis) / VEC + threadIdx.x; g * VEC < span1 + mis; g += 256) {
        const size_t s0 = g * VEC;
        const size_t ea = (s0 > span0 + mis ? s0 : span0 + mis) - mis;
        const size_t eb = (s0 + VEC < span1 + mis ? s0 + VEC : span1 + mis) - mis;
        int lr = (int)((ea - span0) / W), x = (int)((ea - span0) % W);
        if (eb - ea == VEC) {
            // a whole group: the subscripts are compile-time constants after unrolling, so the words stay in registers
            unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const T v = f == 1 ? voxel(lr, x) : same[ea + k];
                if (sizeof(T) == 4) w[k] = __float_as_uint((float)v);
                else w[k >> 2] |= (unsigned)v << (8 * (k & 3));
                if (++x == W) { x = 0; ++lr; }
            }
            *reinterpret_cast<uint4*>(out + ea) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
            for (size_t e = ea; e < eb; ++e) {                 // the ragged ends of the span: element by element
                out[e] = f == 1 ? voxel(lr, x) : same[e];
                if (++x == W) { x = 0; ++lr; }
            }
        }
    }
}

template <typename T, bool LINEAR>
void launch_crop(const CropArgs& a, int N, hipStream_t st) {
    hipLaunchKernelGGL((crop_resample_kernel<T, LINEAR>), dim3(cdiv(a.D * a.H, a.rows), N), dim3(256), (size_t)a.W * sizeof(CropX), st, a);
}

template <typename T>
void launch_pad_min(const void* x, void* ws, const int* flag, int N, int D, int H, int W, hipStream_t st) {
    int lx = 0;
    while (lx < 6 && (1 << lx) < W) ++lx;
    hipLaunchKernelGGL(pad_slice_kernel<T>, dim3(D, N), dim3(256), 0, st, (const T*)x, (T*)ws, flag, D, H, W, lx);
    hipLaunchKernelGGL(pad_z_kernel<T>, dim3(cdiv(H * W, 256), N), dim3(256), 0, st, (const T*)x, (T*)ws, flag, D, H, W);
    hipLaunchKernelGGL(pad_edges_kernel<T>, dim3(N), dim3(256), 0, st, (T*)ws, flag, D, H, W);
}

bool crop_sizes_ok(int N, int D, int H, int W) {
    return N > 0 && N <= 65535 && D > 0 && H > 0 && W > 0 && D <= 65535 && (int64_t)D * H * W <= 0x1fffffffLL;
}

}  // namespace
}  // namespace dram

using namespace dram;

extern "C" size_t dram_aug_pad_min_ws_bytes(int N, int D, int H, int W, int elem_size) {
    if (!crop_sizes_ok(N, D, H, W) || (elem_size != 1 && elem_size != 4)) return 0;
    return (size_t)N * pad_layout(D, H, W).stride * elem_size;
}

extern "C" int dram_aug_pad_min(const void* x, int elem_size, const int* flag, int N, int D, int H, int W, void* ws,
                                size_t ws_bytes, void* stream) {
    DRAM_REQUIRE(x && flag && ws, "aug_pad_min: null pointer");
    DRAM_REQUIRE(elem_size == 1 || elem_size == 4, "aug_pad_min: element size %d (supported: 4 = float32, 1 = uint8)", elem_size);
    DRAM_REQUIRE(crop_sizes_ok(N, D, H, W) && H <= PAD_MAX_DIM && W <= PAD_MAX_DIM,
                 "aug_pad_min: bad sizes (N, D 1..65535, H, W 1..%d, D*H*W up to 2^29-1)", PAD_MAX_DIM);
    DRAM_REQUIRE(((uintptr_t)ws & 15) == 0, "aug_pad_min: workspace must be 16-byte aligned");
    if (ws_bytes < dram_aug_pad_min_ws_bytes(N, D, H, W, elem_size)) {
        set_error("aug_pad_min: workspace too small");
        return DRAM_EWS;
    }
    hipStream_t st = (hipStream_t)stream;
    if (elem_size == 4) launch_pad_min<float>(x, ws, flag, N, D, H, W, st);
    else launch_pad_min<unsigned char>(x, ws, flag, N, D, H, W, st);
    return check_launch("aug_pad_min");
}

extern "C" int dram_aug_crop_resample(const void* x, void* y, int elem_size, int linear, const void* table, const void* pad_ws,
                                      size_t pad_ws_bytes, const int* flag, int n_table, int N, int D, int H, int W,
                                      void* stream) {
    DRAM_REQUIRE(x && y && table && flag, "aug_crop_resample: null pointer");
    DRAM_REQUIRE(elem_size == 1 || elem_size == 4, "aug_crop_resample: element size %d (supported: 4 = float32, 1 = uint8)",
                 elem_size);
    DRAM_REQUIRE(elem_size == 4 || !linear, "aug_crop_resample: linear interpolation is built for float32 only");
    // (H is not bounded here: the row table is sized by `rows`, not by H; a workspace has passed pad_min's H <= PAD_MAX_DIM)
    DRAM_REQUIRE(crop_sizes_ok(N, D, H, W) && W <= CROP_MAX_W,
                 "aug_crop_resample: bad sizes (N, D 1..65535, W 1..%d, D*H*W up to 2^29-1)", CROP_MAX_W);
    DRAM_REQUIRE(n_table == N, "aug_crop_resample: table length %d does not match the batch of %d samples", n_table, N);
    DRAM_REQUIRE(x != y, "aug_crop_resample: cannot run in place");
    DRAM_REQUIRE(((uintptr_t)table & 7) == 0 && ((uintptr_t)x & (elem_size - 1)) == 0 && ((uintptr_t)y & (elem_size - 1)) == 0,
                 "aug_crop_resample: misaligned pointer");
    if (pad_ws) {
        DRAM_REQUIRE(((uintptr_t)pad_ws & 15) == 0, "aug_crop_resample: workspace must be 16-byte aligned");
        if (pad_ws_bytes < dram_aug_pad_min_ws_bytes(N, D, H, W, elem_size)) {
            set_error("aug_crop_resample: workspace too small");
            return DRAM_EWS;
        }
    }
    CropArgs a{x, y, (const CropRec*)table, pad_ws, flag, D, H, W, 0};
    int rows = cdiv(512 * (16 / elem_size), W);       // two 16-byte groups per lane
    a.rows = rows > CROP_MAX_ROWS ? CROP_MAX_ROWS : rows;
    hipStream_t st = (hipStream_t)stream;
    if (elem_size == 1) launch_crop<unsigned char, false>(a, N, st);
    else if (linear) launch_crop<float, true>(a, N, st);
    else launch_crop<float, false>(a, N, st);
    return check_launch("aug_crop_resample");
}
