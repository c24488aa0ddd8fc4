// The lobe-wise class head of the reference's inference entry point, gfx950.
//
// process_pipeline.py -> LesionSegTest.run (dram/job_runner.py:985-1004) does, for every lobe: pool the dense output over the
// resampled lobe mask (pooling_dense_features, models.py:37-49: the masked-mean kernel of head.hip), take the arg-max as the
// lobe's severity class, resize all channels back to the crop, ReLU, pick the predicted class's channel, divide it by its
// maximum over the crop, zero it when the class is 0, and paste it where the lobe is.  Three kernels around the model call and
// the pooling, next to lobe_chunks / lobe_paste of infer.hip (the sigmoid head of evaluate_scan):
//   lobe_chunk_masks  t_lobe_chunk: (lobe == label) of the crop on the crop -> R^3 grid, nearest neighbour
//                     (Resample('fixed_size') takes 'nearest' for '#...reference' keys, data_transforms.py:182-187)
//   lobe_cam_max      cls = argmax_c pool[l, c] by torch.max's CPU rule; max over the WHOLE crop box of
//                     relu(trilinear_ac(dense[l, cls])) -- the reference's order: resize, ReLU, select, max
//   lobe_cam_paste    htp = cls == 0 ? 0 : relu(trilinear_ac(dense[l, cls])) / max, where lobe == label
// Only the selected channel of `dense` is read.  The class stays on the device between the pooling and the paste.
//
// NaN: `dense` is finite by contract.  ReLU and the maximum are fmaxf, which drops a NaN: a voxel that a NaN of the selected
// channel reaches is pasted as 0 and does not take part in the maximum (the reference's dense_out.max() would be NaN and with
// it the lobe's whole map).  A `pool` row is read by torch.max's rule: the first NaN wins, else the first of equal maxima.
#include "lobe_chunk.h"
#include "lane_reduce.h"

namespace dram {

// out[l][R][R][R] = 1 where the nearest voxel of output voxel o on the crop -> R^3 grid carries the chunk's label, else 0;
// 0 beyond the crop's buffer (a crop smaller than R).  The grid is lobe_chunks_kernel's (fixed_size_axis); the nearest voxel
// is resample_volume_kernel's (ItkAxis::nearest: round half up).
__global__ __launch_bounds__(256) void lobe_chunk_masks_kernel(const uint8_t* __restrict__ lobe, float* __restrict__ out,
                                                               ChunkList cl, int H, int W, int R) {
    const int l = blockIdx.y;
    const Chunk c = cl.c[l];
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= R * R * R) return;
    const int xo = e % R, yo = (e / R) % R, zo = e / (R * R);
    float w0, w1;
    const ItkAxis gz = fixed_size_axis(c.dz, R, zo, w0, w1), gy = fixed_size_axis(c.dy, R, yo, w0, w1), gx = fixed_size_axis(c.dx, R, xo, w0, w1);
    float v = 0.f;
    if (gz.inside && gy.inside && gx.inside) {
        const size_t o = ((size_t)(c.z0 + gz.nearest) * H + (c.y0 + gy.nearest)) * W + (c.x0 + gx.nearest);
        v = lobe[o] == c.label ? 1.f : 0.f;
    }
    out[(size_t)l * R * R * R + e] = v;
}

// torch.max(pool[l], dim=-1) on the CPU (ATen compare_base_kernel): a value replaces the running maximum when it is not <= it,
// and a NaN ends the scan -- the first occurrence of the maximum, or the first NaN.
__device__ __forceinline__ int pool_argmax(const float* __restrict__ row, int C) {
    float best = row[0];
    int idx = 0;
    for (int k = 0; k < C; ++k) {
        const float v = row[k];
        if (!(v <= best)) {
            best = v;
            idx = k;
            if (v != v) break;
        }
    }
    return idx;
}

// relu(trilinear_ac(p)(z, y, x)) of crop voxel (z, y, x); p: one R^3 channel.  F.relu AFTER the resize (job_runner.py:993-995)
__device__ __forceinline__ float cam_value(const float* __restrict__ p, const Chunk& c, int R, int z, int y, int x) {
    return fmaxf(Trilinear(R, c, z, y, x).combine(ChunkField{p, R}), 0.f);
}

// blockIdx.y = chunk; a capped grid strides over the dz * dy * dx voxels of the box, outside-lobe voxels included
// (dense_out.max(), job_runner.py:997, is over the crop).  Maximum per wave, per block, then one atomicMax per block on the
// unsigned view: the value is >= 0 after the ReLU, where the unsigned order is the float order -- exact and order-independent.
__global__ __launch_bounds__(256) void lobe_cam_max_kernel(const float* __restrict__ dense, const float* __restrict__ pool,
                                                           ChunkList cl, int C, int R, int* __restrict__ cls_out,
                                                           float* __restrict__ max_out) {
    __shared__ float red[4];
    const int l = blockIdx.y;
    const Chunk c = cl.c[l];
    const int cls = pool_argmax(pool + (size_t)l * C, C);
    if (blockIdx.x == 0 && threadIdx.x == 0) cls_out[l] = cls;
    const float* p = dense + ((size_t)l * C + cls) * R * R * R;
    const int64_t n = (int64_t)c.dz * c.dy * c.dx;
    const int64_t stride = (int64_t)gridDim.x * 256;
    float m = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        int z, y, x;
        crop_decode(c, (int)i, z, y, x);
        m = fmaxf(m, cam_value(p, c, R, z, y, x));
    }
    m = block_max_256(m, red);
    m = m > 0.f ? m : 0.f;                                        // (never the bit pattern of -0: it would be the largest key)
    if (threadIdx.x == 0) atomicMax(reinterpret_cast<unsigned*>(max_out + l), __float_as_uint(m));
}

// crop_voxel's walk.  v / m is the IEEE quotient: 0 / 0 = NaN when the whole channel is <= 0 over the box, as in the reference.
__global__ __launch_bounds__(256) void lobe_cam_paste_kernel(const float* __restrict__ dense, const uint8_t* __restrict__ lobe,
                                                             float* __restrict__ htp, ChunkList cl,
                                                             const int* __restrict__ cls_in, const float* __restrict__ max_in,
                                                             int C, int H, int W, int R) {
    const CropVoxel v = crop_voxel(cl, lobe, H, W);
    if (!v.mine) return;
    const int cls = cls_in[v.l];
    if (cls == 0) {                                               // `if cls_pred < 1e-7: dense_out.zero_()`, job_runner.py:999
        htp[v.o] = 0.f;
        return;
    }
    htp[v.o] = cam_value(dense + ((size_t)v.l * C + cls) * R * R * R, v.c, R, v.z, v.y, v.x) / max_in[v.l];
}

}  // namespace dram

using namespace dram;

extern "C" int dram_lobe_chunk_masks(const uint8_t* lobe, float* out, const int* chunks, int L, int D, int H, int W, int R,
                                     void* stream) {
    DRAM_REQUIRE(lobe && out, "lobe_chunk_masks: null pointer");
    DRAM_REQUIRE(R > 0 && R <= 1024, "lobe_chunk_masks: bad resample size");
    ChunkList cl;
    int rc = fill_chunks("lobe_chunk_masks", cl, chunks, L, D, H, W);
    if (rc) return rc;
    hipLaunchKernelGGL(lobe_chunk_masks_kernel, dim3(cdiv(R * R * R, 256), L), dim3(256), 0, (hipStream_t)stream, lobe, out,
                       cl, H, W, R);
    return check_launch("lobe_chunk_masks");
}

constexpr int CAM_MAX_VOXELS_PER_THREAD = 8;
constexpr int CAM_MAX_GRID_CAP = 1024;       // blocks per chunk

extern "C" int dram_lobe_cam_max(const float* dense, const float* pool, const int* chunks, int L, int C, int R, int* cls_out,
                                 float* max_out, void* stream) {
    DRAM_REQUIRE(dense && pool && cls_out && max_out, "lobe_cam_max: null pointer");
    DRAM_REQUIRE(R > 0 && R <= 1024 && C > 0, "lobe_cam_max: bad resample size or channel count");
    ChunkList cl;
    dim3 grid;
    const int rc = crop_grid("lobe_cam_max", cl, grid, chunks, L, 0x7fffffff, 0x7fffffff, 0x7fffffff,   // only the sizes are used
                             CAM_MAX_VOXELS_PER_THREAD, CAM_MAX_GRID_CAP);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    (void)hipMemsetAsync(max_out, 0, (size_t)L * sizeof(float), st);
    hipLaunchKernelGGL(lobe_cam_max_kernel, grid, dim3(256), 0, st, dense, pool, cl, C, R, cls_out, max_out);
    return check_launch("lobe_cam_max");
}

extern "C" int dram_lobe_cam_paste(const float* dense, const uint8_t* lobe, float* htp, const int* chunks, const int* cls,
                                   const float* max, int L, int C, int D, int H, int W, int R, void* stream) {
    DRAM_REQUIRE(dense && lobe && htp && cls && max, "lobe_cam_paste: null pointer");
    DRAM_REQUIRE(R > 0 && R <= 1024 && C > 0, "lobe_cam_paste: bad resample size or channel count");
    ChunkList cl;
    dim3 grid;
    const int rc = crop_grid("lobe_cam_paste", cl, grid, chunks, L, D, H, W);
    if (rc) return rc;
    hipLaunchKernelGGL(lobe_cam_paste_kernel, grid, dim3(256), 0, (hipStream_t)stream, dense, lobe, htp, cl, cls, max, C, H, W, R);
    return check_launch("lobe_cam_paste");
}
