// Training-time augmentation pool on a whole device batch (reference: LesionSegChunkTrain.ensemble_scan_augmentation,
// dram/job_runner.py:548-581, over dram/data_transforms.py GaussianBlur / RandomMaskOut / RandomFlip / RandomRotate90 /
// GaussianAddictive).  One launch transforms every sample of [N, D, H, W] with that sample's own parameters, read from
// small device tables; nothing synchronises with the host.  Beside the pool's five: IntensityInverse, GammaTransform,
// ContrastStretchingTransform and ContrastJitter of the same file, point-wise over rows (a sample, or one z-slice of it); the
// three slab projections (a causal sliding min / max along one axis); DiskMaskOut and RandomCubeMask (keep a region, zero the rest).
//
// Every table carries a per-sample flag:  1 = transform,  0 = pass through (copied when y != x),  < 0 = skip the sample
// (y is not written: the ensemble driver keeps samples in different buffers and moves only the ones a launch is for).
#include "philox.h"
#include "volume_math.h"
#include <math.h>

namespace dram {
namespace {

constexpr int AUG_MAX_RADIUS = DRAM_AUG_MAX_RADIUS;
constexpr int AUG_MAX_BOXES = DRAM_AUG_MAX_BOXES;

// ---------------------------------------------------------------- per-sample min / max
// Through the order keys of volume_math.h, so that the result does not depend on which block arrives first.
__global__ void minmax_init_kernel(unsigned* mm, const int* flag, int N) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N || (flag && flag[n] != 1)) return;
    mm[2 * n] = 0xffffffffu;
    mm[2 * n + 1] = 0u;
}

template <bool VEC>
__global__ __launch_bounds__(256) void minmax_kernel(const float* __restrict__ x, unsigned* mm, const int* flag, int64_t S) {
    const int n = blockIdx.y;
    if (flag && flag[n] != 1) return;
    const float* row = x + (int64_t)n * S;
    float lo = INFINITY, hi = -INFINITY;
    const int64_t stride = (int64_t)gridDim.x * 256;
    if (VEC) {
        const float4* r4 = reinterpret_cast<const float4*>(row);
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (S >> 2); i += stride) {
            const float4 v = r4[i];
            lo = fminf(fminf(lo, v.x), fminf(v.y, fminf(v.z, v.w)));
            hi = fmaxf(fmaxf(hi, v.x), fmaxf(v.y, fmaxf(v.z, v.w)));
        }
    } else {
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < S; i += stride) {
            const float v = row[i];
            lo = fminf(lo, v);
            hi = fmaxf(hi, v);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    __shared__ float red[8];
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[w] = lo; red[4 + w] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        lo = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
        hi = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
        atomicMin(&mm[2 * n], Key<float>::enc(lo));
        atomicMax(&mm[2 * n + 1], Key<float>::enc(hi));
    }
}

__global__ void minmax_decode_kernel(unsigned* mm, const int* flag, int N) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N || (flag && flag[n] != 1)) return;
    float* out = reinterpret_cast<float*>(mm);
    const float lo = Key<float>::dec(mm[2 * n]), hi = Key<float>::dec(mm[2 * n + 1]);
    out[2 * n] = lo;
    out[2 * n + 1] = hi;
}

// The same {min, max} table (fp32: every uint8 value is exact in it) for a uint8 sample, between the same two small kernels.
__global__ __launch_bounds__(256) void minmax_u8_kernel(const unsigned char* __restrict__ x, unsigned* mm, const int* flag,
                                                        int64_t S) {
    const int n = blockIdx.y;
    if (flag && flag[n] != 1) return;
    const unsigned char* row = x + (int64_t)n * S;
    unsigned lo = 255u, hi = 0u;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < S; i += (int64_t)gridDim.x * 256) {
        const unsigned v = row[i];
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned a = (unsigned)__shfl_xor((int)lo, o, 64), b = (unsigned)__shfl_xor((int)hi, o, 64);
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMin(&mm[2 * n], Key<float>::enc((float)lo));
        atomicMax(&mm[2 * n + 1], Key<float>::enc((float)hi));
    }
}

// ---------------------------------------------------------------- Gaussian blur (scipy.ndimage.gaussian_filter, mode='reflect')
// 'reflect' (d c b a | a b c d): index into the 2n-periodic mirrored sequence; valid for any i and n >= 1.
__device__ __forceinline__ int reflect_index(int i, int n) {
    if (i >= 0 && i < n) return i;
    const int p = 2 * n;
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - 1 - m;
}

// One block: a TZ x TY x TX output tile.  The tile and its halo of R (mirrored at the volume's faces, which commutes with the
// separable passes) are read once into LDS; the z and y passes run in place there, one thread per line with the line in
// registers; the x pass forms the outputs.  Intermediates are rounded to fp32 after each pass, as scipy's are.
template <int R, int TZ, int TY, int TX>
__global__ __launch_bounds__(256) void blur_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                   const float* __restrict__ wtab, const int* __restrict__ flag, int D, int H,
                                                   int W, int nTx, int nTy) {
    constexpr int LZ = TZ + 2 * R, LY = TY + 2 * R, LX = TX + 2 * R;
    __shared__ float s[LZ * LY * LX];
    __shared__ int rz[LZ], ry[LY], rx[LX];
    const int n = blockIdx.y;
    const int f = flag[n];
    if (f < 0) return;
    const int t = blockIdx.x;
    const int x0 = (t % nTx) * TX, y0 = ((t / nTx) % nTy) * TY, z0 = (t / (nTx * nTy)) * TZ;
    const int64_t S = (int64_t)D * H * W;
    const float* xs = x + (int64_t)n * S;
    float* ys = y + (int64_t)n * S;
    const int tid = threadIdx.x;

    if (f == 0) {   // pass through
        if (xs == ys) return;
        for (int i = tid; i < TZ * TY * TX; i += 256) {
            const int gx = x0 + i % TX, gy = y0 + (i / TX) % TY, gz = z0 + i / (TX * TY);
            if (gx < W && gy < H && gz < D) {
                const int64_t o = ((int64_t)gz * H + gy) * W + gx;
                ys[o] = xs[o];
            }
        }
        return;
    }

    if (tid < LZ) rz[tid] = reflect_index(z0 - R + tid, D);
    else if (tid >= 64 && tid < 64 + LY) ry[tid - 64] = reflect_index(y0 - R + tid - 64, H);
    else if (tid >= 128 && tid < 128 + LX) rx[tid - 128] = reflect_index(x0 - R + tid - 128, W);
    float w[R + 1];
#pragma unroll
    for (int j = 0; j <= R; ++j) w[j] = wtab[n * (AUG_MAX_RADIUS + 1) + j];
    __syncthreads();

    for (int i = tid; i < LZ * LY * LX; i += 256) {
        const int lx = i % LX, ly = (i / LX) % LY, lz = i / (LX * LY);
        s[i] = xs[((int64_t)rz[lz] * H + ry[ly]) * W + rx[lx]];
    }
    __syncthreads();

    // z pass: one thread per (y, x) column
    for (int c = tid; c < LY * LX; c += 256) {
        float v[LZ];
#pragma unroll
        for (int k = 0; k < LZ; ++k) v[k] = s[k * (LY * LX) + c];
#pragma unroll
        for (int k = 0; k < TZ; ++k) {
            float acc = v[k + R] * w[0];
#pragma unroll
            for (int j = 1; j <= R; ++j) acc += (v[k + R - j] + v[k + R + j]) * w[j];
            s[k * (LY * LX) + c] = acc;
        }
    }
    __syncthreads();

    // y pass: one thread per (z, x) line
    for (int c = tid; c < TZ * LX; c += 256) {
        const int base = (c / LX) * (LY * LX) + c % LX;
        float v[LY];
#pragma unroll
        for (int k = 0; k < LY; ++k) v[k] = s[base + k * LX];
#pragma unroll
        for (int k = 0; k < TY; ++k) {
            float acc = v[k + R] * w[0];
#pragma unroll
            for (int j = 1; j <= R; ++j) acc += (v[k + R - j] + v[k + R + j]) * w[j];
            s[base + k * LX] = acc;
        }
    }
    __syncthreads();

    // x pass and the only write
    for (int i = tid; i < TZ * TY * TX; i += 256) {
        const int lx = i % TX, ly = (i / TX) % TY, lz = i / (TX * TY);
        const int gx = x0 + lx, gy = y0 + ly, gz = z0 + lz;
        const float* p = s + (lz * LY + ly) * LX + lx + R;
        float acc = p[0] * w[0];
#pragma unroll
        for (int j = 1; j <= R; ++j) acc += (p[-j] + p[j]) * w[j];
        if (gx < W && gy < H && gz < D) ys[((int64_t)gz * H + gy) * W + gx] = acc;
    }
}

template <int R, int TZ, int TY, int TX>
void launch_blur(const float* x, float* y, const float* w, const int* flag, int N, int D, int H, int W, hipStream_t st) {
    const int nTx = cdiv(W, TX), nTy = cdiv(H, TY), nTz = cdiv(D, TZ);
    hipLaunchKernelGGL((blur_kernel<R, TZ, TY, TX>), dim3(nTx * nTy * nTz, N), dim3(256), 0, st, x, y, w, flag, D, H, W, nTx, nTy);
}

// ---------------------------------------------------------------- mask-out
template <int VEC>
__global__ __launch_bounds__(256) void maskout_kernel(const float* x, float* y, const float* __restrict__ mm,
                                                      const int* __restrict__ boxes, const double* __restrict__ u,
                                                      const int* __restrict__ flag, int times, int D, int H, int W) {
    __shared__ int sb[AUG_MAX_BOXES * 6];
    __shared__ float sf[AUG_MAX_BOXES];
    const int n = blockIdx.y;
    const int f = flag[n];
    if (f < 0 || (f == 0 && x == y)) return;
    const int tid = threadIdx.x;
    if (f == 1) {
        if (tid < times * 6) sb[tid] = boxes[n * times * 6 + tid];
        if (tid < times) {   // numpy's uniform(low, high): low + (high - low) * u in fp64, rounded when stored into the fp32 array
            const double lo = (double)mm[2 * n], hi = (double)mm[2 * n + 1];
            sf[tid] = (float)(lo + (hi - lo) * u[n * times + tid]);
        }
        __syncthreads();
    }
    const int64_t S = (int64_t)D * H * W;
    const int64_t i = ((int64_t)blockIdx.x * 256 + tid) * VEC;
    if (i >= S) return;
    const float* xs = x + (int64_t)n * S;
    float* ys = y + (int64_t)n * S;
    float v[VEC];
    if constexpr (VEC == 4) {
        const float4 q = *reinterpret_cast<const float4*>(xs + i);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        v[0] = xs[i];
    }
    if (f == 1) {
        const int xx = (int)(i % W), yy = (int)((i / W) % H), zz = (int)(i / ((int64_t)W * H));
        for (int k = 0; k < times; ++k) {   // later boxes overwrite earlier ones
            const int* b = sb + k * 6;
            if (zz >= b[0] && zz < b[1] && yy >= b[2] && yy < b[3]) {
#pragma unroll
                for (int e = 0; e < VEC; ++e)
                    if (xx + e >= b[4] && xx + e < b[5]) v[e] = sf[k];
            }
        }
    }
    if constexpr (VEC == 4) *reinterpret_cast<float4*>(ys + i) = make_float4(v[0], v[1], v[2], v[3]);
    else ys[i] = v[0];
}

// ---------------------------------------------------------------- additive Gaussian noise
// Philox4x32-10 (philox.h): key = the sample's seed, counter = index of the group of four elements.

// Box-Muller on 24-bit uniforms strictly inside (0, 1): two independent N(0, 1) values.
__device__ __forceinline__ void box_muller(unsigned a, unsigned b, float& z0, float& z1) {
    const float u1 = ((float)(a >> 8) + 0.5f) * 5.9604644775390625e-8f;
    const float u2 = ((float)(b >> 8) + 0.5f) * 5.9604644775390625e-8f;
    const float r = sqrtf(-2.0f * __logf(u1));
    z0 = r * __cosf(6.283185307179586f * u2);
    z1 = r * __sinf(6.283185307179586f * u2);
}

// The reference's arithmetic (data_transforms.py:372-388) with its roundings: every step in fp32, except that an explicit
// fp64 noise array is added in fp64 and the sum rounded (numpy's in-place float32 += float64).
template <bool VEC>
__global__ __launch_bounds__(256) void noise_kernel(const float* x, float* y, const float* __restrict__ mm,
                                                    const float* __restrict__ sigma, const unsigned long long* __restrict__ seeds,
                                                    const int* __restrict__ flag, const double* __restrict__ noise, int64_t S) {
    const int n = blockIdx.y;
    const int f = flag[n];
    if (f < 0 || (f == 0 && x == y)) return;
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i = g * 4;
    if (i >= S) return;
    const float* xs = x + (int64_t)n * S;
    float* ys = y + (int64_t)n * S;
    const int cnt = (S - i) < 4 ? (int)(S - i) : 4;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (VEC) {
        const float4 q = *reinterpret_cast<const float4*>(xs + i);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        for (int e = 0; e < cnt; ++e) v[e] = xs[i + e];
    }
    if (f == 1) {
        const float lo = mm[2 * n], hi = mm[2 * n + 1];
        const float range = __fsub_rn(hi, lo);
        const float denom = __fadd_rn(range, 1e-7f);
        float z[4];
        if (!noise) {
            const unsigned long long seed = seeds[n];
            unsigned r[4];
            philox4x32_10((unsigned)seed, (unsigned)(seed >> 32), (unsigned)g, (unsigned)((unsigned long long)g >> 32), r);
            box_muller(r[0], r[1], z[0], z[1]);
            box_muller(r[2], r[3], z[2], z[3]);
        }
        const float sg = noise ? 0.f : sigma[n];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float t = __fdiv_rn(__fsub_rn(v[e], lo), denom);
            if (noise) t = (e < cnt) ? (float)((double)t + noise[(int64_t)n * S + i + e]) : t;
            else t = __fadd_rn(t, __fmul_rn(z[e], sg));
            t = t < 0.f ? 0.f : t;
            t = t > 1.f ? 1.f : t;
            v[e] = __fadd_rn(__fmul_rn(t, range), lo);
        }
    }
    if (VEC) {
        *reinterpret_cast<float4*>(ys + i) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int e = 0; e < cnt; ++e) ys[i + e] = v[e];
    }
}

// ---------------------------------------------------------------- per-sample flip / quarter turn
// out[o] = in[i], i[perm[k]] = flip[k] ? n_k - 1 - o[k] : o[k], with a shape-preserving perm.  A block moves a TILE x TILE
// patch of the plane (A, x) for one index of the third axis.  When the input's x axis stays the output's x axis the patch is
// copied row by row; otherwise it runs along output axis A, and the patch is transposed through LDS so that both the reads and
// the writes are contiguous.
template <typename T, int TILE>
__global__ __launch_bounds__(256) void permflip_kernel(const T* __restrict__ x, T* __restrict__ y, const int* __restrict__ perm,
                                                       const int* __restrict__ flip, const int* __restrict__ flag, int C, int D,
                                                       int H, int W) {
    __shared__ T tile[TILE][TILE + 1];
    const int n = blockIdx.z;
    const int f = flag[n];
    if (f < 0) return;
    const int id[3] = {D, H, W};
    int p[3] = {0, 1, 2}, fl[3] = {0, 0, 0};
    if (f == 1) {
        const int a = perm[3 * n], b = perm[3 * n + 1], c = perm[3 * n + 2];
        // a table entry that is no shape-preserving permutation moves nothing (the host side refuses it earlier)
        const bool ok = a >= 0 && a < 3 && b >= 0 && b < 3 && c >= 0 && c < 3 && ((1 << a) | (1 << b) | (1 << c)) == 7 &&
                        id[a] == D && id[b] == H && id[c] == W;
        if (ok) {
            p[0] = a; p[1] = b; p[2] = c;
            fl[0] = flip[3 * n] != 0; fl[1] = flip[3 * n + 1] != 0; fl[2] = flip[3 * n + 2] != 0;
        }
    }
    const bool ident = p[0] == 0 && p[1] == 1 && p[2] == 2 && !fl[0] && !fl[1] && !fl[2];
    if (ident && x == y) return;
    const int q = p[0] == 2 ? 0 : (p[1] == 2 ? 1 : 2);   // the output axis that the input's x axis becomes
    const int A = q == 2 ? 1 : q, O = 1 - A;
    const int nTx = (W + TILE - 1) / TILE, nTa = (id[A] + TILE - 1) / TILE;
    const int t = blockIdx.x;
    if (t >= nTx * nTa * id[O]) return;
    const int x0 = (t % nTx) * TILE, a0 = ((t / nTx) % nTa) * TILE, co = t / (nTx * nTa);
    const int64_t S = (int64_t)D * H * W;
    const T* xs = x + ((int64_t)n * C + blockIdx.y) * S;
    T* ys = y + ((int64_t)n * C + blockIdx.y) * S;
    const int lane = threadIdx.x % TILE, row0 = threadIdx.x / TILE;
    constexpr int ROWS = 256 / TILE;

    auto src = [&](int oa, int ox) -> int64_t {
        int o[3], i[3];
        o[A] = oa; o[O] = co; o[2] = ox;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int v = fl[k] ? id[k] - 1 - o[k] : o[k];
            if (p[k] == 0) i[0] = v; else if (p[k] == 1) i[1] = v; else i[2] = v;
        }
        return ((int64_t)i[0] * H + i[1]) * W + i[2];
    };
    auto dst = [&](int oa, int ox) -> int64_t {
        int o[3];
        o[A] = oa; o[O] = co; o[2] = ox;
        return ((int64_t)o[0] * H + o[1]) * W + o[2];
    };

    if (q == 2) {
        for (int r = row0; r < TILE; r += ROWS) {
            const int oa = a0 + r, ox = x0 + lane;
            if (oa < id[A] && ox < W) ys[dst(oa, ox)] = xs[src(oa, ox)];
        }
        return;
    }
    for (int r = row0; r < TILE; r += ROWS) {   // lanes along output axis A = the input's x axis
        const int oa = a0 + lane, ox = x0 + r;
        if (oa < id[A] && ox < W) tile[r][lane] = xs[src(oa, ox)];
    }
    __syncthreads();
    for (int r = row0; r < TILE; r += ROWS) {
        const int oa = a0 + r, ox = x0 + lane;
        if (oa < id[A] && ox < W) ys[dst(oa, ox)] = tile[lane][r];
    }
}

template <typename T, int TILE>
void launch_permflip(const void* x, void* y, const int* perm, const int* flip, const int* flag, int N, int C, int D, int H,
                     int W, hipStream_t st) {
    const int nTx = cdiv(W, TILE);
    const int tiles = nTx * (cdiv(D, TILE) * H > cdiv(H, TILE) * D ? cdiv(D, TILE) * H : cdiv(H, TILE) * D);
    hipLaunchKernelGGL((permflip_kernel<T, TILE>), dim3(tiles, C, N), dim3(256), 0, st, (const T*)x, (T*)y, perm, flip, flag, C,
                       D, H, W);
}

// ---------------------------------------------------------------- per-row mean
// Rows of L floats (a sample, or one z-slice of it).  A block walks its row with a grid stride, every lane with four loads in
// flight and an fp64 sum per load slot; the block's fp64 partial goes to the workspace and one thread per row adds the row's
// partials in index order.  Which element goes to which lane depends on L alone (not on the row's alignment or on how many rows
// the launch has), so a row gives the same bits wherever it stands.  No atomics.
constexpr int MEAN_BLOCK_ELEMS = 4096;   // elements of a row per block and step: 16 per lane
constexpr int MEAN_MAX_BLOCKS = 128;     // blocks per row

inline int mean_blocks(int64_t L) {
    const int64_t b = cdiv64(L, MEAN_BLOCK_ELEMS);
    return (int)(b < 1 ? 1 : (b > MEAN_MAX_BLOCKS ? MEAN_MAX_BLOCKS : b));
}

__global__ __launch_bounds__(256) void row_sum_kernel(const float* __restrict__ x, double* __restrict__ part,
                                                      const int* __restrict__ flag, int64_t L, int nblk) {
    __shared__ double red[4];
    const int r = blockIdx.y;
    if (flag && flag[r] != 1) return;
    const float* row = x + (int64_t)r * L;
    const int64_t stride = (int64_t)nblk * 256;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < L; i += 4 * stride) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t j = i + u * stride;
            if (j < L) a[u] += (double)row[j];
        }
    }
    const double s = wave_sum_d((a[0] + a[1]) + (a[2] + a[3]));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[(size_t)r * nblk + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// numpy's mean of a float32 array is a float32: the fp64 quotient is rounded once.
__global__ void row_mean_kernel(const double* __restrict__ part, float* __restrict__ mean, const int* __restrict__ flag, int R,
                                int64_t L, int nblk) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R || (flag && flag[r] != 1)) return;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += part[(size_t)r * nblk + b];
    mean[r] = (float)(s / (double)L);
}

// StandarizeChannel (data_transforms.py:873-899): a = x - x.mean(); a /= a.std(), float32 arrays.  Three launches: the row sums
// above; then every block forms the row's mean from the partials (the order row_mean_kernel adds them in, so the same fp32 mean
// in every block) and adds d = fp32(x - mean) and d * d in fp64, element to lane as in row_sum_kernel; then one thread per row
// adds those partials in index order: std = sqrt(sum d^2 / L - (sum d / L)^2), numpy's population form of the centred values.
__global__ __launch_bounds__(256) void row_sqdev_kernel(const float* __restrict__ x, const double* __restrict__ part,
                                                        double* __restrict__ part2, const int* __restrict__ flag, int64_t L,
                                                        int nblk) {
    __shared__ double red[8];
    __shared__ float mean_s;
    const int r = blockIdx.y;
    if (flag && flag[r] != 1) return;
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int b = 0; b < nblk; ++b) s += part[(size_t)r * nblk + b];
        mean_s = (float)(s / (double)L);
    }
    __syncthreads();
    const float mean = mean_s;
    const float* row = x + (int64_t)r * L;
    const int64_t stride = (int64_t)nblk * 256;
    double a[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < L; i += 4 * stride) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t j = i + u * stride;
            if (j < L) {
                const double d = (double)__fsub_rn(row[j], mean);
                a[u] += d;
                q[u] += d * d;
            }
        }
    }
    const double sa = wave_sum_d((a[0] + a[1]) + (a[2] + a[3])), sq = wave_sum_d((q[0] + q[1]) + (q[2] + q[3]));
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = sa; red[4 + (threadIdx.x >> 6)] = sq; }
    __syncthreads();
    if (threadIdx.x == 0) {
        part2[((size_t)r * nblk + blockIdx.x) * 2] = (red[0] + red[1]) + (red[2] + red[3]);
        part2[((size_t)r * nblk + blockIdx.x) * 2 + 1] = (red[4] + red[5]) + (red[6] + red[7]);
    }
}

__global__ void row_mean_std_kernel(const double* __restrict__ part, const double* __restrict__ part2, float* __restrict__ ms,
                                    const int* __restrict__ flag, int R, int64_t L, int nblk) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R || (flag && flag[r] != 1)) return;
    double s = 0.0, sa = 0.0, sq = 0.0;
    for (int b = 0; b < nblk; ++b) {
        s += part[(size_t)r * nblk + b];
        sa += part2[((size_t)r * nblk + b) * 2];
        sq += part2[((size_t)r * nblk + b) * 2 + 1];
    }
    const double md = sa / (double)L;
    const double var = sq / (double)L - md * md;
    ms[2 * r] = (float)(s / (double)L);
    ms[2 * r + 1] = (float)sqrt(var > 0.0 ? var : 0.0);
}

// ---------------------------------------------------------------- point-wise intensity maps
// IntensityInverse, GammaTransform, ContrastStretchingTransform and ContrastJitter (data_transforms.py:213-248, 279-362, 538-579)
// with the reference's roundings: numpy keeps a float32 array float32 against Python scalars, so every step is one fp32
// operation and the drawn factors enter rounded to fp32.  `**` is powf.
struct MapCoef {
    float lo, hi, range, denom, rmin, mean, a, b;
    int keep;
};

template <int MODE>
__device__ __forceinline__ MapCoef map_coef(const float* __restrict__ mm, const float* __restrict__ mean,
                                            const float* __restrict__ par, int keep, int r) {
    MapCoef c = {};
    c.keep = keep;
    if (mm) {
        c.lo = mm[2 * r];
        c.hi = mm[2 * r + 1];
    }
    c.range = __fsub_rn(c.hi, c.lo);
    c.denom = __fadd_rn(c.range, 1e-7f);
    if (MODE == DRAM_AUG_MAP_INVERSE)   // (1 - rescaled).min(): the map decreases, so it is the value at x = max
        c.rmin = __fsub_rn(1.f, __fdiv_rn(__fsub_rn(c.hi, c.lo), c.denom));
    if (MODE == DRAM_AUG_MAP_JITTER) c.mean = mean[r];
    if (MODE != DRAM_AUG_MAP_INVERSE) {
        c.a = par[2 * r];
        c.b = par[2 * r + 1];
    }
    return c;
}

template <int MODE>
__device__ __forceinline__ float map_one(float v, const MapCoef& c) {
    if (MODE == DRAM_AUG_MAP_STANDARDIZE) return __fdiv_rn(__fsub_rn(v, c.a), c.b);     // params = {mean, std} of the row
    if (MODE == DRAM_AUG_MAP_JITTER) {
        float t = __fadd_rn(__fmul_rn(__fsub_rn(v, c.mean), c.a), c.mean);
        if (c.keep) {
            t = t < c.lo ? c.lo : t;
            t = t > c.hi ? c.hi : t;
        }
        return t;
    }
    const float r = __fdiv_rn(__fsub_rn(v, c.lo), c.denom);
    float d;
    if (MODE == DRAM_AUG_MAP_INVERSE) d = __fsub_rn(__fsub_rn(1.f, r), c.rmin);
    else if (MODE == DRAM_AUG_MAP_GAMMA) d = powf(r, c.a);
    else d = __fdiv_rn(1.f, __fadd_rn(1.f, powf(__fdiv_rn(c.b, __fadd_rn(r, 1e-7f)), c.a)));
    return __fadd_rn(__fmul_rn(d, c.range), c.lo);
}

// Grid (blocks, row).  VEC: both bases are 16-byte aligned, so a row that starts `r * L` floats in is 16-byte aligned after
// `head` elements, at the same place in x and in y; lanes 0 .. nvec-1 move one float4 each and lane nvec moves the head and the
// tail (six elements at most).  !VEC: four scalar elements per lane.  Every element is read and written by one lane: y may be x.
template <int MODE, bool VEC>
__global__ __launch_bounds__(256) void intensity_map_kernel(const float* x, float* y, const float* __restrict__ mm,
                                                            const float* __restrict__ mean, const float* __restrict__ par,
                                                            const int* __restrict__ flag, int keep, int64_t L) {
    const int r = blockIdx.y;
    const int f = flag[r];
    if (f < 0 || (f == 0 && x == y)) return;
    const int64_t off = (int64_t)r * L;
    const float* xs = x + off;
    float* ys = y + off;
    int64_t head = VEC ? ((4 - (off & 3)) & 3) : 0;
    if (head > L) head = L;
    const int64_t nvec = VEC ? ((L - head) >> 2) : 0;
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (VEC ? g > nvec : g * 4 >= L) return;
    MapCoef c = {};
    if (f == 1) c = map_coef<MODE>(mm, mean, par, keep, r);
    if (g < nvec) {
        float4 q = *reinterpret_cast<const float4*>(xs + head + 4 * g);
        if (f == 1) {
            q.x = map_one<MODE>(q.x, c);
            q.y = map_one<MODE>(q.y, c);
            q.z = map_one<MODE>(q.z, c);
            q.w = map_one<MODE>(q.w, c);
        }
        *reinterpret_cast<float4*>(ys + head + 4 * g) = q;
        return;
    }
    if (VEC) {
        for (int64_t i = 0; i < head; ++i) ys[i] = f == 1 ? map_one<MODE>(xs[i], c) : xs[i];
        for (int64_t i = head + 4 * nvec; i < L; ++i) ys[i] = f == 1 ? map_one<MODE>(xs[i], c) : xs[i];
    } else {
        const int64_t end = g * 4 + 4 < L ? g * 4 + 4 : L;
        for (int64_t i = g * 4; i < end; ++i) ys[i] = f == 1 ? map_one<MODE>(xs[i], c) : xs[i];
    }
}

template <int MODE>
void launch_intensity_map(const float* x, float* y, const float* mm, const float* mean, const float* par, const int* flag,
                          int keep, int R, int64_t L, hipStream_t st) {
    const dim3 grid((unsigned)cdiv64(L / 4 + 1, 256), R);
    if (aligned16(x) && aligned16(y))
        hipLaunchKernelGGL((intensity_map_kernel<MODE, true>), grid, dim3(256), 0, st, x, y, mm, mean, par, flag, keep, L);
    else
        hipLaunchKernelGGL((intensity_map_kernel<MODE, false>), grid, dim3(256), 0, st, x, y, mm, mean, par, flag, keep, L);
}

// ---------------------------------------------------------------- slab projections (causal sliding min / max along one axis)
// MinimalIntensityProjection / MaximumIntensityProjection / MinimalIntensityAxialProjection (data_transforms.py:409-504):
// out[.., i, ..] = min or max of in[.., max(0, i - t) .. i, ..] along the sample's axis.  A row of W floats is cut where the
// OUTPUT address is 16-byte aligned: `head` scalars, `nvec` quads, a scalar tail; one lane per quad and one more lane per row for
// the head and the tail.  The input is read through a 4-byte aligned quad type: window rows of a z or y walk stand W or H*W floats
// apart, which need not be a multiple of four.
constexpr int SLAB_MAX = DRAM_AUG_MAX_SLAB;
constexpr int SLAB_HALO = SLAB_MAX + 4;     // LDS columns in front of a row segment: a full window left of a head element
constexpr int SLAB_SEG_QUADS = 64;          // quads of a row per LDS pass (x walk)
constexpr int SLAB_MAX_ROWS = 64;           // rows per block (x walk)

struct __attribute__((packed, aligned(4))) quad_u { float x, y, z, w; };

template <bool IS_MAX>
__device__ __forceinline__ float slab_op(float a, float b) { return IS_MAX ? fmaxf(a, b) : fminf(a, b); }

template <bool IS_MAX>
__device__ __forceinline__ float4 slab_op4(float4 a, const quad_u& b) {
    return make_float4(slab_op<IS_MAX>(a.x, b.x), slab_op<IS_MAX>(a.y, b.y), slab_op<IS_MAX>(a.z, b.z), slab_op<IS_MAX>(a.w, b.w));
}

__device__ __forceinline__ int slab_head(const float* yrow, int W) {
    const int head = (int)(((16 - (reinterpret_cast<uintptr_t>(yrow) & 15)) & 15) >> 2);
    return head < W ? head : W;
}

// x walk: quads per LDS pass, lanes per row (one per quad and one for head and tail), rows per block, LDS floats per row.
struct SlabXGeom { int sq, slots, rows, stride; };
__host__ __device__ constexpr SlabXGeom slab_x_geom(int W) {
    const int sq = W / 4 < SLAB_SEG_QUADS ? W / 4 : SLAB_SEG_QUADS;
    const int rows = 256 / (sq + 1) < SLAB_MAX_ROWS ? 256 / (sq + 1) : SLAB_MAX_ROWS;
    return {sq, sq + 1, rows, SLAB_HALO + 4 * sq + 4};
}
constexpr int slab_x_lds_floats() {
    int m = 0;
    for (int sq = 0; sq <= SLAB_SEG_QUADS; ++sq) {
        const SlabXGeom g = slab_x_geom(4 * sq);
        m = g.rows * g.stride > m ? g.rows * g.stride : m;
    }
    return m;
}
constexpr int SLAB_X_LDS = slab_x_lds_floats();

// z or y walk: a lane owns its quad and walks the window through rows `step` floats apart (coalesced across the lanes of a row;
// what a neighbouring output row read a moment ago comes from the cache).  i = the row's index along the axis.
template <bool IS_MAX>
__device__ __forceinline__ void slab_walk_rows(const float* __restrict__ xs, float* __restrict__ ys, int t, int axis, int rows,
                                               int H, int W) {
    const int slots = (W + 3) / 4 + 1;
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= (int64_t)rows * slots) return;      // rows * slots < 2^32, as D*H*W < 2^31: 32-bit divisions from here on
    const unsigned row = (unsigned)g / (unsigned)slots;
    const int q = (int)((unsigned)g - row * (unsigned)slots);
    const int i = axis == 0 ? (int)(row / (unsigned)H) : (int)(row % (unsigned)H);
    const int64_t step = axis == 0 ? (int64_t)H * W : W;
    const int m = t < i ? t : i;
    const int64_t off = (int64_t)row * W;
    const int head = slab_head(ys + off, W);
    const int nvec = (W - head) >> 2;
    if (q < nvec) {
        const int64_t o = off + head + 4 * q;
        const quad_u v = *reinterpret_cast<const quad_u*>(xs + o);
        float4 acc = make_float4(v.x, v.y, v.z, v.w);
#pragma unroll 4
        for (int k = 1; k <= m; ++k) acc = slab_op4<IS_MAX>(acc, *reinterpret_cast<const quad_u*>(xs + o - k * step));
        *reinterpret_cast<float4*>(ys + o) = acc;
    } else if (q == slots - 1) {
        for (int c = 0; c < W; ++c) {
            if (c == head) c += 4 * nvec;
            if (c >= W) break;
            float acc = xs[off + c];
            for (int k = 1; k <= m; ++k) acc = slab_op<IS_MAX>(acc, xs[off + c - k * step]);
            ys[off + c] = acc;
        }
    }
}

// x walk: a block stages `rows` rows in LDS, SLAB_SEG_QUADS quads of each at a time, behind SLAB_HALO columns that hold the
// elements to their left (the identity of the operation left of the row's start, so the window needs no clipping).  Column
// SLAB_HALO is the segment's first aligned quad, so quads are 16-byte aligned in LDS as well.
template <bool IS_MAX>
__device__ __forceinline__ void slab_walk_x(const float* __restrict__ xs, float* __restrict__ ys, int t, int rows, int W,
                                            float* smem) {
    const SlabXGeom gm = slab_x_geom(W);
    if ((int64_t)blockIdx.x * gm.rows >= rows) return;
    const float ident = IS_MAX ? -INFINITY : INFINITY;
    const int rr = threadIdx.x / gm.slots, q = threadIdx.x - rr * gm.slots;
    const int64_t row = (int64_t)blockIdx.x * gm.rows + rr;
    const bool active = rr < gm.rows && row < rows;
    const int64_t off = active ? row * W : 0;
    const int head = active ? slab_head(ys + off, W) : 0;
    const int nvec = (W - head) >> 2;
    float* srow = smem + (active ? rr : 0) * gm.stride;
    const int nseg = (W / 4 + SLAB_SEG_QUADS - 1) / SLAB_SEG_QUADS > 1 ? (W / 4 + SLAB_SEG_QUADS - 1) / SLAB_SEG_QUADS : 1;
    for (int s = 0; s < nseg; ++s) {
        const int qs = s * SLAB_SEG_QUADS;
        int nq = nvec - qs;
        nq = nq < 0 ? 0 : (nq > SLAB_SEG_QUADS ? SLAB_SEG_QUADS : nq);
        const int xlo = head + 4 * qs;                   // the row element in LDS column SLAB_HALO
        const int tail0 = head + 4 * nvec;               // the row's scalar tail [tail0, W): staged and formed in the last pass
        const bool last = s == nseg - 1;
        if (active) {
            if (q < nq) {
                const quad_u v = *reinterpret_cast<const quad_u*>(xs + off + xlo + 4 * q);
                *reinterpret_cast<float4*>(srow + SLAB_HALO + 4 * q) = make_float4(v.x, v.y, v.z, v.w);
            }
            for (int j = q; j < SLAB_HALO; j += gm.slots) {
                const int c = xlo - SLAB_HALO + j;
                srow[j] = c >= 0 ? xs[off + c] : ident;
            }
            if (last && q == gm.slots - 1)
                for (int c = tail0; c < W; ++c) srow[c - xlo + SLAB_HALO] = xs[off + c];
        }
        __syncthreads();
        if (active) {
            if (q < nq) {
                const float* p = srow + SLAB_HALO + 4 * q - t;
                float o[4] = {ident, ident, ident, ident};
                for (int i = 0; i < t + 4; ++i) {        // p[i] lies in the window of output e iff 0 <= i - e <= t
                    const float v = p[i];
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (i >= e && i - e <= t) o[e] = slab_op<IS_MAX>(o[e], v);
                }
                *reinterpret_cast<float4*>(ys + off + xlo + 4 * q) = make_float4(o[0], o[1], o[2], o[3]);
            } else if (q == gm.slots - 1) {
                for (int c = (s == 0 ? 0 : W); c < W; ++c) {     // the head, with the first pass
                    if (c == head) break;
                    const float* p = srow + c - xlo + SLAB_HALO;
                    float acc = p[0];
                    for (int k = 1; k <= t; ++k) acc = slab_op<IS_MAX>(acc, p[-k]);
                    ys[off + c] = acc;
                }
                for (int c = (last ? tail0 : W); c < W; ++c) {
                    const float* p = srow + c - xlo + SLAB_HALO;
                    float acc = p[0];
                    for (int k = 1; k <= t; ++k) acc = slab_op<IS_MAX>(acc, p[-k]);
                    ys[off + c] = acc;
                }
            }
        }
        __syncthreads();
    }
}

// Grid (blocks, sample).  Axis and thickness are the sample's, so a block takes one path.  A passed-through sample is a window of
// one element; so is a table entry outside 0..2 / 0..DRAM_AUG_MAX_SLAB (the host side refuses those earlier).
template <bool IS_MAX>
__global__ __launch_bounds__(256) void slab_project_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                           const int* __restrict__ thickness, const int* __restrict__ axis,
                                                           const int* __restrict__ flag, int D, int H, int W) {
    __shared__ __attribute__((aligned(16))) float smem[SLAB_X_LDS];
    const int n = blockIdx.y;
    const int f = flag[n];
    if (f < 0) return;
    int t = 0, a = 0;
    if (f == 1) {
        t = thickness[n];
        a = axis[n];
        if (t < 0 || t > SLAB_MAX || a < 0 || a > 2) t = a = 0;
    }
    const int64_t S = (int64_t)D * H * W;
    const float* xs = x + (int64_t)n * S;
    float* ys = y + (int64_t)n * S;
    if (a == 2 && t > 0) slab_walk_x<IS_MAX>(xs, ys, t, D * H, W, smem);
    else slab_walk_rows<IS_MAX>(xs, ys, t, a, D * H, H, W);
}

// ---------------------------------------------------------------- keep a region, zero the rest
// DiskMaskOut / RandomCubeMask._mask (data_transforms.py:840-870, 647-657).  Grid (blocks, channel, sample); a lane moves 16
// bytes (VEC elements) or, beside the aligned body and when a base is unaligned, single elements, as intensity_map_kernel does.
struct Region {
    int z0, z1, y0, y1, x0, x1, cy, cx, r2;
};

__device__ __forceinline__ bool region_keeps(const Region& g, int z, int yy, int xx) {
    if (z < g.z0 || z >= g.z1 || yy < g.y0 || yy >= g.y1 || xx < g.x0 || xx >= g.x1) return false;
    if (g.r2 < 0) return true;
    const long long dy = yy - g.cy, dx = xx - g.cx;
    return dy * dy + dx * dx <= (long long)g.r2;
}

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void keep_region_kernel(const T* x, T* y, const int* __restrict__ boxes,
                                                          const int* __restrict__ disk, const int* __restrict__ flag, int C,
                                                          int D, int H, int W) {
    constexpr int PER = 16 / (int)sizeof(T);
    const int n = blockIdx.z;
    const int f = flag[n];
    if (f < 0 || (f == 0 && x == y)) return;
    const int64_t L = (int64_t)D * H * W;
    const int64_t off = ((int64_t)n * C + blockIdx.y) * L;
    const T* xs = x + off;
    T* ys = y + off;
    int64_t head = VEC ? ((PER - (off & (PER - 1))) & (PER - 1)) : 0;
    if (head > L) head = L;
    const int64_t nvec = VEC ? (L - head) / PER : 0;
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (VEC ? g > nvec : g * PER >= L) return;
    Region rg = {};
    if (f == 1) {
        const int* b = boxes + 6 * n;
        const int* d = disk + 3 * n;
        rg = {b[0], b[1], b[2], b[3], b[4], b[5], d[0], d[1], d[2]};
    }
    auto range = [&](int64_t i0, int64_t i1) {      // single elements [i0, i1)
        if (i0 >= i1) return;
        const unsigned r0 = (unsigned)i0 / (unsigned)W;      // i0 < 2^31: 32-bit divisions
        int xx = (int)((unsigned)i0 - r0 * (unsigned)W), yy = (int)(r0 % (unsigned)H), z = (int)(r0 / (unsigned)H);
        for (int64_t i = i0; i < i1; ++i) {
            ys[i] = (f == 0 || region_keeps(rg, z, yy, xx)) ? xs[i] : T(0);
            if (++xx == W) { xx = 0; if (++yy == H) { yy = 0; ++z; } }
        }
    };
    if (g < nvec) {
        const int64_t i0 = head + g * PER;
        union { uint4 q; T e[PER]; } v;
        v.q = *reinterpret_cast<const uint4*>(xs + i0);
        if (f == 1) {
            const unsigned r0 = (unsigned)i0 / (unsigned)W;
            int xx = (int)((unsigned)i0 - r0 * (unsigned)W), yy = (int)(r0 % (unsigned)H), z = (int)(r0 / (unsigned)H);
#pragma unroll
            for (int e = 0; e < PER; ++e) {
                if (!region_keeps(rg, z, yy, xx)) v.e[e] = T(0);
                if (++xx == W) { xx = 0; if (++yy == H) { yy = 0; ++z; } }
            }
        }
        *reinterpret_cast<uint4*>(ys + i0) = v.q;
        return;
    }
    if (VEC) {
        range(0, head);
        range(head + nvec * PER, L);
    } else {
        range(g * PER, g * PER + PER < L ? g * PER + PER : L);
    }
}

template <typename T>
void launch_keep_region(const void* x, void* y, const int* boxes, const int* disk, const int* flag, int N, int C, int D, int H,
                        int W, hipStream_t st) {
    constexpr int PER = 16 / (int)sizeof(T);
    const int64_t L = (int64_t)D * H * W;
    const dim3 grid((unsigned)cdiv64(L / PER + 1, 256), C, N);
    if (aligned16(x) && aligned16(y))
        hipLaunchKernelGGL((keep_region_kernel<T, true>), grid, dim3(256), 0, st, (const T*)x, (T*)y, boxes, disk, flag, C, D, H, W);
    else
        hipLaunchKernelGGL((keep_region_kernel<T, false>), grid, dim3(256), 0, st, (const T*)x, (T*)y, boxes, disk, flag, C, D, H, W);
}

int check_batch(const char* who, int n_table, int N, int64_t S) {
    DRAM_REQUIRE(N > 0 && N <= 65535 && S > 0 && S <= 0x7fffffff, "%s: bad sizes (N 1..65535, D*H*W 1..2^31-1)", who);
    DRAM_REQUIRE(n_table == N, "%s: table length %d does not match the batch of %d samples", who, n_table, N);
    return DRAM_OK;
}

}  // namespace
}  // namespace dram

using namespace dram;

extern "C" int dram_aug_minmax(const float* x, float* minmax, const int* flag, int N, int64_t S, void* stream) {
    DRAM_REQUIRE(x && minmax, "aug_minmax: null pointer");
    DRAM_REQUIRE(N > 0 && N <= 65535 && S > 0, "aug_minmax: bad sizes");
    hipStream_t st = (hipStream_t)stream;
    unsigned* mm = reinterpret_cast<unsigned*>(minmax);
    const bool vec = (S & 3) == 0 && aligned16(x);
    const int64_t work = vec ? (S >> 2) : S;
    int64_t bps = cdiv64(work, 256 * 8);
    const int64_t cap = 8192 / N > 1 ? 8192 / N : 1;
    if (bps > cap) bps = cap;
    hipLaunchKernelGGL(minmax_init_kernel, dim3(cdiv(N, 256)), dim3(256), 0, st, mm, flag, N);
    if (vec) hipLaunchKernelGGL(minmax_kernel<true>, dim3((unsigned)bps, N), dim3(256), 0, st, x, mm, flag, S);
    else hipLaunchKernelGGL(minmax_kernel<false>, dim3((unsigned)bps, N), dim3(256), 0, st, x, mm, flag, S);
    hipLaunchKernelGGL(minmax_decode_kernel, dim3(cdiv(N, 256)), dim3(256), 0, st, mm, flag, N);
    return check_launch("aug_minmax");
}

extern "C" int dram_aug_minmax_u8(const unsigned char* x, float* minmax, const int* flag, int N, int64_t S, void* stream) {
    DRAM_REQUIRE(x && minmax, "aug_minmax_u8: null pointer");
    DRAM_REQUIRE(N > 0 && N <= 65535 && S > 0, "aug_minmax_u8: bad sizes");
    hipStream_t st = (hipStream_t)stream;
    unsigned* mm = reinterpret_cast<unsigned*>(minmax);
    int64_t bps = cdiv64(S, 256 * 32);
    const int64_t cap = 8192 / N > 1 ? 8192 / N : 1;
    if (bps > cap) bps = cap;
    hipLaunchKernelGGL(minmax_init_kernel, dim3(cdiv(N, 256)), dim3(256), 0, st, mm, flag, N);
    hipLaunchKernelGGL(minmax_u8_kernel, dim3((unsigned)bps, N), dim3(256), 0, st, x, mm, flag, S);
    hipLaunchKernelGGL(minmax_decode_kernel, dim3(cdiv(N, 256)), dim3(256), 0, st, mm, flag, N);
    return check_launch("aug_minmax_u8");
}

extern "C" int dram_aug_gaussian_blur(const float* x, float* y, const float* weights, const int* flag, int n_table, int radius,
                                      int N, int D, int H, int W, void* stream) {
    DRAM_REQUIRE(x && y && weights && flag, "aug_gaussian_blur: null pointer");
    DRAM_REQUIRE(radius >= 0 && radius <= AUG_MAX_RADIUS, "aug_gaussian_blur: radius %d outside the supported 0..%d", radius,
                 AUG_MAX_RADIUS);
    DRAM_REQUIRE(D > 0 && H > 0 && W > 0, "aug_gaussian_blur: bad sizes");
    int rc = check_batch("aug_gaussian_blur", n_table, N, (int64_t)D * H * W);
    if (rc) return rc;
    DRAM_REQUIRE(x != y, "aug_gaussian_blur: cannot run in place");
    hipStream_t st = (hipStream_t)stream;
    switch (radius) {
        case 0:
        case 1: launch_blur<1, 16, 16, 32>(x, y, weights, flag, N, D, H, W, st); break;
        case 2: launch_blur<2, 16, 16, 32>(x, y, weights, flag, N, D, H, W, st); break;
        case 3: launch_blur<3, 8, 8, 32>(x, y, weights, flag, N, D, H, W, st); break;
        default: launch_blur<4, 8, 8, 32>(x, y, weights, flag, N, D, H, W, st); break;
    }
    return check_launch("aug_gaussian_blur");
}

extern "C" int dram_aug_mask_out(const float* x, float* y, const float* minmax, const int* boxes, const double* u,
                                 const int* flag, int n_table, int times, int N, int D, int H, int W, void* stream) {
    DRAM_REQUIRE(x && y && minmax && boxes && u && flag, "aug_mask_out: null pointer");
    DRAM_REQUIRE(times >= 1 && times <= AUG_MAX_BOXES, "aug_mask_out: %d boxes per sample outside the supported 1..%d", times,
                 AUG_MAX_BOXES);
    DRAM_REQUIRE(D > 0 && H > 0 && W > 0, "aug_mask_out: bad sizes");
    const int64_t S = (int64_t)D * H * W;
    int rc = check_batch("aug_mask_out", n_table, N, S);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if ((W & 3) == 0 && aligned16(x) && aligned16(y))
        hipLaunchKernelGGL(maskout_kernel<4>, dim3((unsigned)cdiv64(S / 4, 256), N), dim3(256), 0, st, x, y, minmax, boxes, u, flag,
                           times, D, H, W);
    else
        hipLaunchKernelGGL(maskout_kernel<1>, dim3((unsigned)cdiv64(S, 256), N), dim3(256), 0, st, x, y, minmax, boxes, u, flag,
                           times, D, H, W);
    return check_launch("aug_mask_out");
}

extern "C" int dram_aug_gaussian_noise(const float* x, float* y, const float* minmax, const float* sigma,
                                       const unsigned long long* seeds, const int* flag, int n_table, const double* noise, int N,
                                       int64_t S, void* stream) {
    DRAM_REQUIRE(x && y && minmax && flag && (noise || (sigma && seeds)), "aug_gaussian_noise: null pointer");
    int rc = check_batch("aug_gaussian_noise", n_table, N, S);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)cdiv64(cdiv64(S, 4), 256), N);
    if ((S & 3) == 0 && aligned16(x) && aligned16(y))
        hipLaunchKernelGGL(noise_kernel<true>, grid, dim3(256), 0, st, x, y, minmax, sigma, seeds, flag, noise, S);
    else
        hipLaunchKernelGGL(noise_kernel<false>, grid, dim3(256), 0, st, x, y, minmax, sigma, seeds, flag, noise, S);
    return check_launch("aug_gaussian_noise");
}

extern "C" int dram_aug_permute_flip(const void* x, void* y, int elem_size, const int* perm, const int* flip, const int* flag,
                                     int n_table, int N, int C, int D, int H, int W, void* stream) {
    DRAM_REQUIRE(x && y && perm && flip && flag, "aug_permute_flip: null pointer");
    DRAM_REQUIRE(elem_size == 1 || elem_size == 4, "aug_permute_flip: element size %d (supported: 4 = float32, 1 = uint8)",
                 elem_size);
    DRAM_REQUIRE(D > 0 && H > 0 && W > 0 && C > 0 && C <= 65535, "aug_permute_flip: bad sizes");
    int rc = check_batch("aug_permute_flip", n_table, N, (int64_t)D * H * W);
    if (rc) return rc;
    DRAM_REQUIRE(x != y, "aug_permute_flip: cannot run in place");
    hipStream_t st = (hipStream_t)stream;
    if (elem_size == 4) launch_permflip<float, 32>(x, y, perm, flip, flag, N, C, D, H, W, st);
    else launch_permflip<unsigned char, 64>(x, y, perm, flip, flag, N, C, D, H, W, st);
    return check_launch("aug_permute_flip");
}

extern "C" int dram_aug_slab_project(const float* x, float* y, const int* thickness, const int* axis, int is_max,
                                     const int* flag, int n_table, int N, int D, int H, int W, void* stream) {
    DRAM_REQUIRE(x && y && thickness && axis && flag, "aug_slab_project: null pointer");
    DRAM_REQUIRE(D > 0 && H > 0 && W > 0, "aug_slab_project: bad sizes");
    int rc = check_batch("aug_slab_project", n_table, N, (int64_t)D * H * W);
    if (rc) return rc;
    DRAM_REQUIRE(x != y, "aug_slab_project: cannot run in place");
    hipStream_t st = (hipStream_t)stream;
    const int64_t rows = (int64_t)D * H;
    const int64_t by_rows = cdiv64(rows * (cdiv(W, 4) + 1), 256), by_x = cdiv64(rows, slab_x_geom(W).rows);
    const dim3 grid((unsigned)(by_rows > by_x ? by_rows : by_x), N);
    if (is_max) hipLaunchKernelGGL(slab_project_kernel<true>, grid, dim3(256), 0, st, x, y, thickness, axis, flag, D, H, W);
    else hipLaunchKernelGGL(slab_project_kernel<false>, grid, dim3(256), 0, st, x, y, thickness, axis, flag, D, H, W);
    return check_launch("aug_slab_project");
}

extern "C" int dram_aug_keep_region(const void* x, void* y, int elem_size, const int* boxes, const int* disk, const int* flag,
                                    int n_table, int N, int C, int D, int H, int W, void* stream) {
    DRAM_REQUIRE(x && y && boxes && disk && flag, "aug_keep_region: null pointer");
    DRAM_REQUIRE(elem_size == 1 || elem_size == 4, "aug_keep_region: element size %d (supported: 4 = float32, 1 = uint8)",
                 elem_size);
    DRAM_REQUIRE(D > 0 && H > 0 && W > 0 && C > 0 && C <= 65535, "aug_keep_region: bad sizes");
    int rc = check_batch("aug_keep_region", n_table, N, (int64_t)D * H * W);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (elem_size == 4) launch_keep_region<float>(x, y, boxes, disk, flag, N, C, D, H, W, st);
    else launch_keep_region<unsigned char>(x, y, boxes, disk, flag, N, C, D, H, W, st);
    return check_launch("aug_keep_region");
}

extern "C" size_t dram_aug_row_mean_ws_bytes(int R, int64_t L) {
    if (R <= 0 || L <= 0) return 0;
    return (size_t)R * mean_blocks(L) * sizeof(double);
}

extern "C" int dram_aug_row_mean(const float* x, float* mean, const int* flag, int R, int64_t L, void* ws, size_t ws_bytes,
                                 void* stream) {
    DRAM_REQUIRE(x && mean && ws, "aug_row_mean: null pointer");
    DRAM_REQUIRE(R > 0 && R <= 65535 && L > 0 && L <= 0x7fffffff, "aug_row_mean: bad sizes (rows 1..65535, row length 1..2^31-1)");
    DRAM_REQUIRE(((uintptr_t)ws & 7) == 0, "aug_row_mean: workspace must be 8-byte aligned");
    if (ws_bytes < dram_aug_row_mean_ws_bytes(R, L)) {
        set_error("aug_row_mean: workspace too small");
        return DRAM_EWS;
    }
    hipStream_t st = (hipStream_t)stream;
    const int nblk = mean_blocks(L);
    hipLaunchKernelGGL(row_sum_kernel, dim3(nblk, R), dim3(256), 0, st, x, (double*)ws, flag, L, nblk);
    hipLaunchKernelGGL(row_mean_kernel, dim3(cdiv(R, 256)), dim3(256), 0, st, (const double*)ws, mean, flag, R, L, nblk);
    return check_launch("aug_row_mean");
}

extern "C" size_t dram_aug_row_mean_std_ws_bytes(int R, int64_t L) { return 3 * dram_aug_row_mean_ws_bytes(R, L); }

extern "C" int dram_aug_row_mean_std(const float* x, float* mean_std, const int* flag, int R, int64_t L, void* ws,
                                     size_t ws_bytes, void* stream) {
    DRAM_REQUIRE(x && mean_std && ws, "aug_row_mean_std: null pointer");
    DRAM_REQUIRE(R > 0 && R <= 65535 && L > 0 && L <= 0x7fffffff,
                 "aug_row_mean_std: bad sizes (rows 1..65535, row length 1..2^31-1)");
    DRAM_REQUIRE(((uintptr_t)ws & 7) == 0, "aug_row_mean_std: workspace must be 8-byte aligned");
    if (ws_bytes < dram_aug_row_mean_std_ws_bytes(R, L)) {
        set_error("aug_row_mean_std: workspace too small");
        return DRAM_EWS;
    }
    hipStream_t st = (hipStream_t)stream;
    const int nblk = mean_blocks(L);
    double* part = (double*)ws;
    double* part2 = part + (size_t)R * nblk;
    hipLaunchKernelGGL(row_sum_kernel, dim3(nblk, R), dim3(256), 0, st, x, part, flag, L, nblk);
    hipLaunchKernelGGL(row_sqdev_kernel, dim3(nblk, R), dim3(256), 0, st, x, (const double*)part, part2, flag, L, nblk);
    hipLaunchKernelGGL(row_mean_std_kernel, dim3(cdiv(R, 256)), dim3(256), 0, st, (const double*)part, (const double*)part2,
                       mean_std, flag, R, L, nblk);
    return check_launch("aug_row_mean_std");
}

extern "C" int dram_aug_intensity_map(const float* x, float* y, int mode, const float* minmax, const float* mean,
                                      const float* params, int keep_range, const int* flag, int n_table, int R, int64_t L,
                                      void* stream) {
    DRAM_REQUIRE((mode >= DRAM_AUG_MAP_INVERSE && mode <= DRAM_AUG_MAP_JITTER) || mode == DRAM_AUG_MAP_STANDARDIZE,
                 "aug_intensity_map: unknown mode %d", mode);
    const bool jitter = mode == DRAM_AUG_MAP_JITTER, stand = mode == DRAM_AUG_MAP_STANDARDIZE;
    DRAM_REQUIRE(x && y && flag && (minmax || stand || (jitter && !keep_range)) && (mean || !jitter) &&
                     (params || mode == DRAM_AUG_MAP_INVERSE),
                 "aug_intensity_map: null pointer");
    int rc = check_batch("aug_intensity_map", n_table, R, L);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    switch (mode) {
        case DRAM_AUG_MAP_INVERSE:
            launch_intensity_map<DRAM_AUG_MAP_INVERSE>(x, y, minmax, mean, params, flag, 0, R, L, st);
            break;
        case DRAM_AUG_MAP_GAMMA:
            launch_intensity_map<DRAM_AUG_MAP_GAMMA>(x, y, minmax, mean, params, flag, 0, R, L, st);
            break;
        case DRAM_AUG_MAP_STRETCH:
            launch_intensity_map<DRAM_AUG_MAP_STRETCH>(x, y, minmax, mean, params, flag, 0, R, L, st);
            break;
        case DRAM_AUG_MAP_STANDARDIZE:
            launch_intensity_map<DRAM_AUG_MAP_STANDARDIZE>(x, y, nullptr, nullptr, params, flag, 0, R, L, st);
            break;
        default:
            launch_intensity_map<DRAM_AUG_MAP_JITTER>(x, y, minmax, mean, params, flag, keep_range != 0, R, L, st);
            break;
    }
    return check_launch("aug_intensity_map");
}
