// What the whole-scan inference kernels of infer.hip, infer_cam.hip and infer_tta.hip share: the chunk list that a launch
// carries and the host-side reading of the caller's chunk array, the two index rules between a crop and its R^3 chunk, the
// trilinear gather of the way back, the walk over the voxels of the crops, the sigmoid of the paste, and for the streaming
// kernels the capped grid and the 256-bin LDS histogram.  One definition each.
#pragma once
#include "volume_math.h"

namespace dram {

struct Chunk {   // crop window [z0,z0+dz) x [y0,y0+dy) x [x0,x0+dx) of lobe `label`
    int z0, y0, x0, dz, dy, dx, label, pad;
};
constexpr int MAX_CHUNKS = 8;
struct ChunkList {
    Chunk c[MAX_CHUNKS];
};

// R^3 -> crop, the way back: F.interpolate(..., align_corners=True) (job_runner.py:767, 993)
__device__ __forceinline__ void ac_index(int in, int out, int o, int& i0, int& i1, float& l0, float& l1) {
    const float scale = out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;   // ATen area_pixel_compute_scale
    const float src = scale * (float)o;
    i0 = (int)src;
    if (i0 > in - 1) i0 = in - 1;
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = src - (float)i0;
    l0 = 1.f - l1;
}

// One axis of the crop -> R^3 grid: Resample('fixed_size') (data_transforms.py:170-175 -> utils.resample, utils.py:371-381:
// sitkLinear, new_spacing = spacing * size_in / size_out), so c = o * size_in / size_out (itk_axis, volume_math.h); fp32 weights.
__device__ __forceinline__ ItkAxis fixed_size_axis(int in, int out, int o, float& l0, float& l1) {
    const ItkAxis a = itk_axis((double)o * (double)in / (double)out, in);
    l1 = (float)a.t;
    l0 = 1.f - l1;
    return a;
}

// The eight taps with which crop voxel (z, y, x) of chunk c samples the chunk's R^3 grid (ac_index per axis), and their fp32 weights
struct Trilinear {
    int z0, z1, y0, y1, x0, x1;
    float a0, a1, b0, b1, c0, c1;                                  // of z0, z1, y0, y1, x0, x1
    __device__ __forceinline__ Trilinear(int R, const Chunk& c, int z, int y, int x) {
        ac_index(R, c.dz, z, z0, z1, a0, a1);
        ac_index(R, c.dy, y, y0, y1, b0, b1);
        ac_index(R, c.dx, x, x0, x1, c0, c1);
    }
    // at(z, y, x): the value of a tap.  hipcc contracts `p * q + r` of this tree into fmas, and which ones depends on the code around
    // the call: a kernel whose use of it changes is compared bit for bit with its former self again.
    template <class At>
    __device__ __forceinline__ float combine(At&& at) const {
        return a0 * (b0 * (c0 * at(z0, y0, x0) + c1 * at(z0, y0, x1)) + b1 * (c0 * at(z0, y1, x0) + c1 * at(z0, y1, x1))) +
               a1 * (b0 * (c0 * at(z1, y0, x0) + c1 * at(z1, y0, x1)) + b1 * (c0 * at(z1, y1, x0) + c1 * at(z1, y1, x1)));
    }
};

// One R^3 field of a chunk as the `at` of Trilinear::combine
struct ChunkField {
    const float* p;
    int R;
    __device__ __forceinline__ float operator()(int z, int y, int x) const { return p[((size_t)z * R + y) * R + x]; }
};

// F.sigmoid before the resize (job_runner.py:765)
__device__ __forceinline__ float paste_sigmoid(float d) { return 1.f / (1.f + expf(-d)); }

// Crop voxel e of chunk c, x fastest
__device__ __forceinline__ void crop_decode(const Chunk& c, int e, int& z, int& y, int& x) {
    x = e % c.dx; y = (e / c.dx) % c.dy; z = e / (c.dx * c.dy);
}

// The walk of the paste kernels: blockIdx.y = chunk l, one thread per voxel of the largest crop (crop_grid).  `mine`: the thread
// has a voxel (z, y, x) of crop c, at offset o of the volume, and it carries the chunk's label (otherwise z, y, x, o are not set).
// A voxel carries one label, so it is written by the chunk of that label alone: chunks with different labels may overlap.
struct CropVoxel { int l; Chunk c; int z, y, x; size_t o; bool mine; };
__device__ __forceinline__ CropVoxel crop_voxel(const ChunkList& cl, const uint8_t* lobe, int H, int W) {
    CropVoxel v;
    v.l = blockIdx.y;
    v.c = cl.c[v.l];
    v.mine = false;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < v.c.dz * v.c.dy * v.c.dx) {
        crop_decode(v.c, e, v.z, v.y, v.x);
        v.o = ((size_t)(v.c.z0 + v.z) * H + (v.c.y0 + v.y)) * W + (v.c.x0 + v.x);
        v.mine = lobe[v.o] == v.c.label;
    }
    return v;
}

// 256-bin histogram of a stream, blocks of 256 threads: counts in LDS (lh[256]), then one 64-bit atomic per occupied bin.
// bin_of(i) is asked for the voxels with inside(i) only.  The barrier of the flush also serves what the caller left in LDS
// between the two calls.
template <class Inside, class Bin>
__device__ __forceinline__ void hist256_count(unsigned* lh, size_t n, Inside&& inside, Bin&& bin_of) {
    lh[threadIdx.x] = 0;
    __syncthreads();
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride)
        if (inside(i)) atomicAdd(&lh[bin_of(i)], 1u);
}
__device__ __forceinline__ void hist256_flush(const unsigned* lh, unsigned long long* hist) {
    __syncthreads();
    if (lh[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (unsigned long long)lh[threadIdx.x]);
}

// chunks: host array of L x {z0,y0,x0,dz,dy,dx,label}
inline int fill_chunks(const char* who, ChunkList& cl, const int* chunks, int L, int D, int H, int W) {
    DRAM_REQUIRE(chunks && L > 0 && L <= MAX_CHUNKS, "%s: between 1 and %d chunks", who, MAX_CHUNKS);
    for (int l = 0; l < L; ++l) {
        Chunk& c = cl.c[l];
        c.z0 = chunks[l * 7 + 0]; c.y0 = chunks[l * 7 + 1]; c.x0 = chunks[l * 7 + 2];
        c.dz = chunks[l * 7 + 3]; c.dy = chunks[l * 7 + 4]; c.dx = chunks[l * 7 + 5];
        c.label = chunks[l * 7 + 6]; c.pad = 0;
        DRAM_REQUIRE(c.z0 >= 0 && c.y0 >= 0 && c.x0 >= 0 && c.dz > 0 && c.dy > 0 && c.dx > 0 && c.z0 + c.dz <= D &&
                         c.y0 + c.dy <= H && c.x0 + c.dx <= W, "%s: chunk %d outside the volume", who, l);
    }
    return DRAM_OK;
}

// Blocks of 256 threads for a stream of n > 0 elements at per_thread elements a thread, at most cap of them
inline unsigned stream_grid(int64_t n, int per_thread, int64_t cap) {
    const int64_t want = cdiv64(n, 256 * per_thread);
    return (unsigned)(want < cap ? (want > 0 ? want : 1) : cap);
}

// The launch of a kernel that walks the crops: reads the chunk array, refuses a crop whose voxels an int cannot index, and
// gives the grid: x over the largest crop (one voxel per thread and no cap, unless told otherwise), y the chunk.
inline int crop_grid(const char* who, ChunkList& cl, dim3& grid, const int* chunks, int L, int D, int H, int W,
                     int per_thread = 1, int64_t cap = 0x7fffffff) {
    const int rc = fill_chunks(who, cl, chunks, L, D, H, W);
    if (rc) return rc;
    int64_t mx = 0;
    for (int l = 0; l < L; ++l) {
        const int64_t v = (int64_t)cl.c[l].dz * cl.c[l].dy * cl.c[l].dx;
        mx = v > mx ? v : mx;
    }
    DRAM_REQUIRE(mx < 0x7fffffffLL, "%s: chunk too large", who);
    grid = dim3(stream_grid(mx, per_thread, cap), L);
    return DRAM_OK;
}

}  // namespace dram
