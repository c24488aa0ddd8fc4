// What the per-lobe kernels of infer.hip and infer_cam.hip share: the chunk list that a launch carries, the two index rules
// between a crop and its R^3 chunk, and the host-side reading of the caller's chunk array.  One definition each.
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

// the largest crop of the list, in voxels
inline int64_t max_chunk_voxels(const ChunkList& cl, int L) {
    int64_t mx = 0;
    for (int l = 0; l < L; ++l) {
        const int64_t v = (int64_t)cl.c[l].dz * cl.c[l].dy * cl.c[l].dx;
        mx = v > mx ? v : mx;
    }
    return mx;
}

}  // namespace dram
