// Training-time augmentation pool on a whole device batch (reference: LesionSegChunkTrain.ensemble_scan_augmentation,
// dram/job_runner.py:548-581, over dram/data_transforms.py GaussianBlur / RandomMaskOut / RandomFlip / RandomRotate90 /
// GaussianAddictive).  One launch transforms every sample of [N, D, H, W] with that sample's own parameters, read from
// small device tables; nothing synchronises with the host.  Beside the pool's five: IntensityInverse, GammaTransform,
// ContrastStretchingTransform and ContrastJitter of the same file, point-wise over rows (a sample, or one z-slice of it).
//
// Every table carries a per-sample flag:  1 = transform,  0 = pass through (copied when y != x),  < 0 = skip the sample
// (y is not written: the ensemble driver keeps samples in different buffers and moves only the ones a launch is for).
#include "common.h"
#include <math.h>

namespace dram {
namespace {

constexpr int AUG_MAX_RADIUS = DRAM_AUG_MAX_RADIUS;
constexpr int AUG_MAX_BOXES = DRAM_AUG_MAX_BOXES;

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---------------------------------------------------------------- per-sample min / max
// Floats mapped to unsigned ints of the same order: integer atomicMin / atomicMax are exact, associative and commutative,
// so the result does not depend on which block arrives first.
__device__ __forceinline__ unsigned order_enc(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float order_dec(unsigned e) {
    return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e);
}

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
        atomicMin(&mm[2 * n], order_enc(lo));
        atomicMax(&mm[2 * n + 1], order_enc(hi));
    }
}

__global__ void minmax_decode_kernel(unsigned* mm, const int* flag, int N) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N || (flag && flag[n] != 1)) return;
    float* out = reinterpret_cast<float*>(mm);
    const float lo = order_dec(mm[2 * n]), hi = order_dec(mm[2 * n + 1]);
    out[2 * n] = lo;
    out[2 * n + 1] = hi;
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
// Philox4x32-10 (Salmon et al., SC'11): key = the sample's seed, counter = index of the group of four elements.
__device__ __forceinline__ void philox4x32_10(unsigned k0, unsigned k1, unsigned c0, unsigned c1, unsigned out[4]) {
    unsigned c2 = 0u, c3 = 0u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

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

extern "C" int dram_aug_intensity_map(const float* x, float* y, int mode, const float* minmax, const float* mean,
                                      const float* params, int keep_range, const int* flag, int n_table, int R, int64_t L,
                                      void* stream) {
    DRAM_REQUIRE(mode >= DRAM_AUG_MAP_INVERSE && mode <= DRAM_AUG_MAP_JITTER, "aug_intensity_map: unknown mode %d", mode);
    const bool jitter = mode == DRAM_AUG_MAP_JITTER;
    DRAM_REQUIRE(x && y && flag && (minmax || (jitter && !keep_range)) && (mean || !jitter) &&
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
        default:
            launch_intensity_map<DRAM_AUG_MAP_JITTER>(x, y, minmax, mean, params, flag, keep_range != 0, R, L, st);
            break;
    }
    return check_launch("aug_intensity_map");
}
