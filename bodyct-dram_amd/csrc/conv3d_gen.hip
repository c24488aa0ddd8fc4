// General 3-D convolution for fp32 NCDHW tensors on gfx950: any kernel size 1..7 per axis, zero padding 0..max(k-1, 1),
// stride 1 or 2 per axis, any channel counts and spatial sizes.  Dilation 1, groups 1.
//
// Replaces the nn.Conv3d dispatches of the reference's blocks (dram/parts.py:66-196, models.py:54-112) for the
// geometries the 3x3x3 / pad 1 (conv3d_k3.hip) and 1x1x1 (head.hip) kernels do not cover: "valid" U-Nets
// (padding 0), 5x5x5 / anisotropic kernels, strided ConvBlock5d / ConvPoolBlock5d convs.  Those two kernels keep
// every shape they served; this file is only reached through HipConv3d's third kind.
//
// All three directions are implicit GEMMs on the exact-fp32 matrix cores (v_mfma_f32_32x32x2_f32), laid out like the
// direct 27-tap kernel conv3d_k3_fwd_kernel:
//
//   forward / backward-data   Y[m][voxel] += A[m][c][tap] * X[c][voxel * is + ib + tap]
//       block = 256 output voxels (BX x BY x 1) x 32 output channels, 4 waves of two 32x32 accumulator tiles; the
//       voxel index sits on the MFMA lane axis so that every accumulator register is a run along x of one channel.
//       K loop over (chunk of 4 input channels, z tap): each step stages the (BY-1)*is+Ty x (BX-1)*is+Tx input rows of
//       one z plane and the Ty*Tx taps of the filter in LDS (double-buffered, global loads of the next step in flight
//       during the MFMAs); out-of-volume halo elements and channel tails read as 0 through out-of-range buffer
//       offsets.  z taps whose plane lies outside the volume are skipped for the whole block.
//       The filter is read in the reference's own [Cout][Cin][kz][ky][kx] layout (no packing step): every thread
//       stages fixed (m, c) pairs and walks the taps.
//   backward-data             the same kernel.  Per axis, dX splits into s output phases r = (i + p) mod s; phase r
//       is a stride-1 correlation of dY with the taps k = r, r + s, ... in reverse order, written to every s-th
//       voxel (s = 1: one phase, the transposed filter with padding k - 1 - p).  A phase without taps (k < s) is
//       zero-filled.
//   backward-weights          dW[co][c][tap] += dY[co][voxel] * X[c][voxel * s - p + tap]
//       M = Cout (32 per block), N = (channel, tap) columns (<= 16 tiles of 32 per block, 4 per wave), K = voxels in
//       boxes of 32 x 4 x 2.  Each block sums a contiguous range of boxes into a partial slab; the slabs are added in
//       a fixed order (deterministic, no float atomics).
#include "conv_device.h"
#include <atomic>

namespace dram {
namespace gen {

constexpr int KC = 4;                   // input channels per K step (two MFMA k-pairs)
constexpr int NQ = 6;                   // input halo elements per thread and channel: (BY-1)*is+Ty x (BX-1)*is+Tx <= 1536
constexpr int TYX_MAX = 49;             // y x x taps per step
constexpr int WG_BOX_X = 32, WG_BOX_Y = 4, WG_BOX_Z = 2;   // backward-weights voxel box
constexpr int WG_PA = 257;              // LDS row stride of the dY tile (odd: conflict-free A reads)
constexpr int WG_NT = 4;                // 32-column tiles per wave (backward-weights)
constexpr int WG_HALO_MAX = 12288;      // floats of input halo per backward-weights block

// One launch of the forward-shaped kernel: output grid q in [0,Q) per axis, written at q*os + oo of the output tensor;
// tap t of the grid point q reads the input at q*is + ib + t and the filter at kb + ks*t (per axis).
struct GenArgs {
    const float* x;      // [N][C][ID][IH][IW]
    const float* w;      // filter; element (m, c, kz, ky, kx) at m*wsm + c*wsk + (kz*Ky + ky)*Kx + kx
    const float* bias;   // [M] or null
    float* y;            // [N][M][OD][OH][OW]
    int N, C, M;
    int ID, IH, IW;
    int OD, OH, OW;
    int QD, QH, QW;
    int osz, osy, osx, ooz, ooy, oox;
    int isz, isy, isx, ibz, iby, ibx;
    int Tz, Ty, Tx;
    int Ky, Kx;
    int kbz, kby, kbx, ksz, ksy, ksx;
    int wsm, wsk;
    unsigned wbytes;
    int HX, HY, PS;      // input rows staged per step
    int nbx, nby, co_tiles;
};

template <int BX, int WQ>
__global__ __launch_bounds__(256, 2) void conv3d_gen_fwd_kernel(GenArgs a) {
    constexpr int BY = 256 / BX;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, kh = lane >> 5;
    int b = blockIdx.x;                              // (n, qz, by, bx, co tile), co tile fastest
    const int co0 = (b % a.co_tiles) * 32; b /= a.co_tiles;
    const int bx = b % a.nbx; b /= a.nbx;
    const int by = b % a.nby; b /= a.nby;
    const int qz = b % a.QD;
    const int n = b / a.QD;
    const int qx0 = bx * BX, qy0 = by * BY;
    const int HX = a.HX, PS = a.PS;
    const int Tyx = a.Ty * a.Tx;
    const int STAGE = KC * PS + Tyx * KC * 32;

    // z taps whose input plane lies inside the volume (block-uniform)
    const int zb = qz * a.isz + a.ibz;
    const int tz_lo = zb < 0 ? -zb : 0;
    const int tz_hi = min(a.Tz, a.ID - zb);
    const int ntz = max(tz_hi - tz_lo, 0);
    const int nchunks = (a.C + KC - 1) / KC;
    const int niter = nchunks * ntz;

    // input halo: in-plane byte offsets of this thread's elements e = tid + 256 q (same for every channel / z tap)
    unsigned xoff[NQ];
    const int gy0 = qy0 * a.isy + a.iby, gx0 = qx0 * a.isx + a.ibx;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int e = tid + 256 * q;
        const int hy = e / HX, hx = e % HX;
        const int gy = gy0 + hy, gx = gx0 + hx;
        const bool ok = e < PS && gy >= 0 && gy < a.IH && gx >= 0 && gx < a.IW;
        xoff[q] = ok ? 4u * (unsigned)(gy * a.IW + gx) : OOB;
    }
    const unsigned plane_bytes = 4u * (unsigned)(a.IH * a.IW);
    const float* xs = a.x + (size_t)n * a.C * a.ID * a.IH * a.IW;

    // filter: slot f = tid + 256 q -> (m = f % 32, c = (f / 32) % KC, tap = f / 128); LDS index = f
    const int wm = tid & 31, wc = (tid >> 5) & 3;
    const bool wm_ok = co0 + wm < a.M;
    unsigned woff[WQ];
#pragma unroll
    for (int q = 0; q < WQ; ++q) {
        const int tap = (tid >> 7) + 2 * q;
        const int ty = tap / a.Tx, tx = tap % a.Tx;
        const int e = (co0 + wm) * a.wsm + wc * a.wsk + (a.kby + a.ksy * ty) * a.Kx + a.kbx + a.ksx * tx;
        woff[q] = (wm_ok && tap < Tyx) ? 4u * (unsigned)e : OOB;
    }
    const __amdgpu_buffer_rsrc_t wsrd = make_rsrc(a.w, a.wbytes);
    const int KyKx = a.Ky * a.Kx;

    f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    int bbase[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int v = 32 * (2 * wave + t) + j;
        const int vx = v % BX, vy = v / BX;
        bbase[t] = kh * PS + vy * a.isy * HX + vx * a.isx;
    }
    const int abase = kh * 32 + j;

    float rin[KC][NQ];
    float rw[WQ];
    auto load_step = [&](int it) {
        const int c0 = (it / ntz) * KC;
        const int tz = tz_lo + it % ntz;
        const int gz = zb + tz;
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) {
            const int c = c0 + kc;
            const float* plane = xs + ((size_t)min(c, a.C - 1) * a.ID + gz) * a.IH * a.IW;
            const __amdgpu_buffer_rsrc_t srd = make_rsrc(uniform_ptr(plane), c < a.C ? plane_bytes : 0u);
#pragma unroll
            for (int q = 0; q < NQ; ++q) rin[kc][q] = buf_load(srd, xoff[q], 0);
        }
        const bool wc_ok = c0 + wc < a.C;
        const unsigned wstep = 4u * (unsigned)(c0 * a.wsk + (a.kbz + a.ksz * tz) * KyKx);
#pragma unroll
        for (int q = 0; q < WQ; ++q) rw[q] = buf_load(wsrd, (wc_ok && woff[q] != OOB) ? woff[q] + wstep : OOB, 0);
    };
    auto store_step = [&](float* stage) {
        float* lin = stage;
        float* lw = stage + KC * PS;
#pragma unroll
        for (int kc = 0; kc < KC; ++kc)
#pragma unroll
            for (int q = 0; q < NQ; ++q)
                if (tid + 256 * q < PS) lin[kc * PS + tid + 256 * q] = rin[kc][q];
#pragma unroll
        for (int q = 0; q < WQ; ++q)
            if ((tid >> 7) + 2 * q < Tyx) lw[tid + 256 * q] = rw[q];
    };
    auto compute = [&](const float* stage) {
        const float* lin = stage;
        const float* lw = stage + KC * PS;
        // k-step s = (tap, kk): operands of step s+1 are read while the MFMAs of step s issue
        float av[2], bv[2][2];
        int ty = 0, tx = 0;
        av[0] = lw[abase];
        bv[0][0] = lin[bbase[0]];
        bv[0][1] = lin[bbase[1]];
        const int nsteps = 2 * Tyx;
        for (int s = 0; s < nsteps; ++s) {
            const int cur = s & 1;
            if (s + 1 < nsteps) {
                const int s1 = s + 1, tap1 = s1 >> 1, kk1 = s1 & 1;
                if (kk1 == 0 && ++tx == a.Tx) { tx = 0; ++ty; }
                const int toff = ty * HX + tx;
                av[cur ^ 1] = lw[abase + (tap1 * KC + 2 * kk1) * 32];
                bv[cur ^ 1][0] = lin[bbase[0] + 2 * kk1 * PS + toff];
                bv[cur ^ 1][1] = lin[bbase[1] + 2 * kk1 * PS + toff];
            }
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cur], bv[cur][0], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cur], bv[cur][1], acc[1], 0, 0, 0);
        }
    };

    if (niter > 0) {
        load_step(0);
        store_step(lds);
    }
    __syncthreads();
    int cur = 0;
    for (int it = 0; it < niter; ++it) {
        const bool has_next = it + 1 < niter;
        if (has_next) load_step(it + 1);
        __builtin_amdgcn_sched_barrier(0);
        compute(lds + cur * STAGE);
        __builtin_amdgcn_sched_barrier(0);
        if (has_next) store_step(lds + (cur ^ 1) * STAGE);
        __syncthreads();
        cur ^= 1;
    }

    // epilogue: accumulator register r of lane (j,kh) = channel (r&3)+8(r>>2)+4kh, voxel j of the tile
    const size_t OS = (size_t)a.OD * a.OH * a.OW;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int v = 32 * (2 * wave + t) + j;
        const int qx = qx0 + v % BX, qy = qy0 + v / BX;
        if (qx >= a.QW || qy >= a.QH) continue;
        const size_t sp = ((size_t)(qz * a.osz + a.ooz) * a.OH + (qy * a.osy + a.ooy)) * a.OW + (qx * a.osx + a.oox);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
            if (co < a.M) {
                float val = acc[t][r];
                if (a.bias) val += a.bias[co];
                a.y[((size_t)n * a.M + co) * OS + sp] = val;
            }
        }
    }
}

// backward-weights: one block = (box range `split`, 32 output channels, CIB input channels x all taps)
struct WgradArgs {
    const float* x;    // [N][Cin][D][H][W]
    const float* dy;   // [N][Cout][OD][OH][OW]
    float* slabs;      // [nsplit][Cout][Cin * T]
    int N, Cin, Cout, D, H, W, OD, OH, OW;
    int Kz, Ky, Kx, T;
    int sz, sy, sx, pz, py, px;
    int HX, HY, HZ, HV;
    int CIB, nci, co_tiles, nbx, nby, nbz, nboxes, boxes_per_split;
};

__global__ __launch_bounds__(256, 2) void conv3d_gen_wgrad_kernel(WgradArgs a) {
    constexpr int BX = WG_BOX_X, BY = WG_BOX_Y, BZ = WG_BOX_Z;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* ldy = lds;                    // [32][WG_PA]
    float* lx = lds + 32 * WG_PA;        // [CIB][HZ][HY][HX]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, kh = lane >> 5;
    int b = blockIdx.x;                  // (split, ci group, co tile), co tile fastest
    const int co0 = (b % a.co_tiles) * 32; b /= a.co_tiles;
    const int cg = b % a.nci;
    const int split = b / a.nci;
    const int ci0 = cg * a.CIB;
    const int ncols = a.CIB * a.T;
    const int HX = a.HX, HY = a.HY, HV = a.HV;

    int colbase[WG_NT];
    bool tile_on[WG_NT];
#pragma unroll
    for (int nt = 0; nt < WG_NT; ++nt) {
        const int tile = wave + 4 * nt;
        tile_on[nt] = tile * 32 < ncols;
        const int col = tile * 32 + j;
        const int cl = col / a.T, tap = col % a.T;
        const int kz = tap / (a.Ky * a.Kx), ky = (tap / a.Kx) % a.Ky, kx = tap % a.Kx;
        colbase[nt] = col < ncols ? cl * HV + (kz * HY + ky) * HX + kx : 0;
    }
    f32x16 acc[WG_NT];
#pragma unroll
    for (int nt = 0; nt < WG_NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;

    const unsigned oplane = 4u * (unsigned)(a.OD * a.OH * a.OW);
    const unsigned xplane = 4u * (unsigned)(a.D * a.H * a.W);
    const int b_lo = split * a.boxes_per_split;
    const int b_hi = min(b_lo + a.boxes_per_split, a.nboxes);
    const int cib = min(a.CIB, a.Cin - ci0);
    const int nx = cib * HV;
    for (int box = b_lo; box < b_hi; ++box) {
        int bb = box;
        const int bx = bb % a.nbx; bb /= a.nbx;
        const int by = bb % a.nby; bb /= a.nby;
        const int bz = bb % a.nbz;
        const int n = bb / a.nbz;
        const int ox0 = bx * BX, oy0 = by * BY, oz0 = bz * BZ;
        const int gx0 = ox0 * a.sx - a.px, gy0 = oy0 * a.sy - a.py, gz0 = oz0 * a.sz - a.pz;
        __syncthreads();   // the previous box's operands are consumed
        // dY tile: element e = co * 256 + v (v along x fastest)
        {
            const float* dyn = a.dy + ((size_t)n * a.Cout) * a.OD * a.OH * a.OW;
#pragma unroll 4
            for (int q0 = 0; q0 < 32; q0 += 8) {
                float r[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int e = tid + 256 * (q0 + u);
                    const int co = e >> 8, v = e & 255;
                    const int oz = oz0 + v / (BX * BY), oy = oy0 + (v / BX) % BY, ox = ox0 + v % BX;
                    const bool ok = co0 + co < a.Cout && oz < a.OD && oy < a.OH && ox < a.OW;
                    const __amdgpu_buffer_rsrc_t srd =
                        make_rsrc(uniform_ptr(dyn + (size_t)min(co0 + co, a.Cout - 1) * a.OD * a.OH * a.OW), oplane);
                    r[u] = buf_load(srd, ok ? 4u * (unsigned)((oz * a.OH + oy) * a.OW + ox) : OOB, 0);
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int e = tid + 256 * (q0 + u);
                    ldy[(e >> 8) * WG_PA + (e & 255)] = r[u];
                }
            }
        }
        // input halo of the box for channels ci0 .. ci0 + cib
        {
            const float* xn = a.x + ((size_t)n * a.Cin + ci0) * a.D * a.H * a.W;
            const __amdgpu_buffer_rsrc_t srd = make_rsrc(xn, (unsigned)min((size_t)cib * xplane, (size_t)0x7fffffff));
            for (int e0 = 0; e0 < nx; e0 += 256 * 8) {
                float r[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int e = e0 + tid + 256 * u;
                    const int cl = e / HV, h = e % HV;
                    const int hz = h / (HX * HY), hy = (h / HX) % HY, hx = h % HX;
                    const int gz = gz0 + hz, gy = gy0 + hy, gx = gx0 + hx;
                    const bool ok = e < nx && gz >= 0 && gz < a.D && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
                    r[u] = buf_load(srd, ok ? (unsigned)cl * xplane + 4u * (unsigned)((gz * a.H + gy) * a.W + gx) : OOB, 0);
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int e = e0 + tid + 256 * u;
                    if (e < nx) lx[e] = r[u];
                }
            }
        }
        __syncthreads();
        // K = the box's 256 voxels, two per MFMA (lane half kh takes voxel 2s + kh)
        const int vstep_y = a.sy * HX, vstep_z = a.sz * HY * HX;
        for (int s = 0; s < 128; ++s) {
            const int v = 2 * s + kh;
            const int vpos = (v / (BX * BY)) * vstep_z + ((v / BX) % BY) * vstep_y + (v % BX) * a.sx;
            const float av = ldy[j * WG_PA + v];
#pragma unroll
            for (int nt = 0; nt < WG_NT; ++nt)
                if (tile_on[nt]) acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, lx[colbase[nt] + vpos], acc[nt], 0, 0, 0);
        }
    }

    const size_t E = (size_t)a.Cout * a.Cin * a.T;
    float* slab = a.slabs + (size_t)split * E;
#pragma unroll
    for (int nt = 0; nt < WG_NT; ++nt) {
        const int col = (wave + 4 * nt) * 32 + j;
        const int cl = col / a.T, tap = col % a.T;
        if (col >= ncols || ci0 + cl >= a.Cin) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
            if (co < a.Cout) slab[((size_t)co * a.Cin + ci0 + cl) * a.T + tap] = acc[nt][r];
        }
    }
}

__global__ void gen_slab_reduce_kernel(const float* __restrict__ slabs, float* __restrict__ out, int64_t E, int nsplit) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    float s = 0.f;
    for (int p = 0; p < nsplit; ++p) s += slabs[(size_t)p * E + e];
    out[e] = s;
}

// ------------------------------------------------------------------------------------------------ host side
static std::atomic<unsigned long long> g_launches[DRAM_CONV_GEN_KINDS];

struct Geom {
    int N, Cin, Cout, D, H, W;
    int k[3], s[3], p[3];   // z, y, x
    int o[3];               // output size
};

static int check_geom(const char* who, Geom& g, int N, int Cin, int Cout, int D, int H, int W, int kz, int ky, int kx,
                      int sz, int sy, int sx, int pz, int py, int px) {
    DRAM_REQUIRE(N > 0 && Cin > 0 && Cout > 0 && D > 0 && H > 0 && W > 0, "%s: non-positive dimension", who);
    const int k[3] = {kz, ky, kx}, s[3] = {sz, sy, sx}, p[3] = {pz, py, px}, in[3] = {D, H, W};
    for (int i = 0; i < 3; ++i) {
        DRAM_REQUIRE(k[i] >= 1 && k[i] <= 7, "%s: kernel size %d outside the supported 1..7", who, k[i]);
        DRAM_REQUIRE(s[i] == 1 || s[i] == 2, "%s: stride %d is not supported (1 or 2)", who, s[i]);
        DRAM_REQUIRE(p[i] >= 0 && p[i] <= (k[i] > 2 ? k[i] - 1 : 1), "%s: padding %d outside the supported 0..max(k-1, 1) (k = %d)",
                     who, p[i], k[i]);
        const int o = (in[i] + 2 * p[i] - k[i]) / s[i] + 1;
        DRAM_REQUIRE(in[i] + 2 * p[i] >= k[i] && o >= 1, "%s: output size below 1 (input %d, kernel %d, padding %d)", who,
                     in[i], k[i], p[i]);
        g.k[i] = k[i];
        g.s[i] = s[i];
        g.p[i] = p[i];
        g.o[i] = o;
    }
    const int64_t cmax = Cin > Cout ? Cin : Cout;
    DRAM_REQUIRE((int64_t)D * H * W * cmax < 0x1fffffffLL && (int64_t)g.o[0] * g.o[1] * g.o[2] * cmax < 0x1fffffffLL,
                 "%s: one sample exceeds 2^29 elements (32-bit buffer offsets)", who);
    DRAM_REQUIRE((int64_t)Cin * Cout * kz * ky * kx < 0x1fffffffLL, "%s: filter exceeds 2^29 elements", who);
    g.N = N; g.Cin = Cin; g.Cout = Cout; g.D = D; g.H = H; g.W = W;
    return DRAM_OK;
}

static LdsAttrOnce g_lds_fwd[6], g_lds_wgrad;

template <int BX, int WQ>
static int launch_fwd_t(GenArgs& a, hipStream_t st, size_t lds, LdsAttrOnce& once) {
    constexpr int BY = 256 / BX;
    a.nbx = cdiv(a.QW, BX);
    a.nby = cdiv(a.QH, BY);
    const int64_t blocks = (int64_t)a.N * a.QD * a.nby * a.nbx * a.co_tiles;
    DRAM_REQUIRE(blocks < 0x7fffffffLL, "conv3d: grid too large");
    if (lds > 65536) {
        const int rc = ensure_dynamic_lds((const void*)conv3d_gen_fwd_kernel<BX, WQ>, lds, once, "conv3d");
        if (rc) return rc;
    }
    hipLaunchKernelGGL((conv3d_gen_fwd_kernel<BX, WQ>), dim3((unsigned)blocks), dim3(256), lds, st, a);
    return check_launch("conv3d_gen_fwd");
}

// One forward-shaped launch; a.Q*, a.T*, a.i*, a.o*, a.k* set by the caller.
static int launch_fwd(GenArgs& a, hipStream_t st) {
    if (a.QD <= 0 || a.QH <= 0 || a.QW <= 0) return DRAM_OK;
    const int BX = a.QW <= 16 ? 16 : 32, BY = 256 / BX;
    a.HX = (BX - 1) * a.isx + a.Tx;
    a.HY = (BY - 1) * a.isy + a.Ty;
    a.PS = a.HX * a.HY;
    DRAM_REQUIRE(a.PS <= 256 * NQ, "conv3d: input tile of %d elements exceeds %d", a.PS, 256 * NQ);
    const int Tyx = a.Ty * a.Tx;
    DRAM_REQUIRE(Tyx <= TYX_MAX, "conv3d: %d y x x taps exceed %d", Tyx, TYX_MAX);
    a.co_tiles = cdiv(a.M, 32);
    const size_t lds = 2 * (size_t)(KC * a.PS + Tyx * KC * 32) * sizeof(float);
    const int wq = (Tyx + 1) / 2;
    const int bi = BX == 16 ? 0 : 3;
    if (wq <= 5) return BX == 16 ? launch_fwd_t<16, 5>(a, st, lds, g_lds_fwd[bi]) : launch_fwd_t<32, 5>(a, st, lds, g_lds_fwd[bi]);
    if (wq <= 13)
        return BX == 16 ? launch_fwd_t<16, 13>(a, st, lds, g_lds_fwd[bi + 1]) : launch_fwd_t<32, 13>(a, st, lds, g_lds_fwd[bi + 1]);
    return BX == 16 ? launch_fwd_t<16, 25>(a, st, lds, g_lds_fwd[bi + 2]) : launch_fwd_t<32, 25>(a, st, lds, g_lds_fwd[bi + 2]);
}

struct WgradPlan {
    WgradArgs a;
    int nsplit;
    size_t lds, ws_bytes;
};

static void wgrad_plan(const Geom& g, WgradPlan& pl) {
    WgradArgs& a = pl.a;
    a.N = g.N; a.Cin = g.Cin; a.Cout = g.Cout; a.D = g.D; a.H = g.H; a.W = g.W;
    a.OD = g.o[0]; a.OH = g.o[1]; a.OW = g.o[2];
    a.Kz = g.k[0]; a.Ky = g.k[1]; a.Kx = g.k[2];
    a.T = a.Kz * a.Ky * a.Kx;
    a.sz = g.s[0]; a.sy = g.s[1]; a.sx = g.s[2];
    a.pz = g.p[0]; a.py = g.p[1]; a.px = g.p[2];
    a.HX = (WG_BOX_X - 1) * a.sx + a.Kx;
    a.HY = (WG_BOX_Y - 1) * a.sy + a.Ky;
    a.HZ = (WG_BOX_Z - 1) * a.sz + a.Kz;
    a.HV = a.HX * a.HY * a.HZ;
    int cib = (4 * WG_NT * 32) / a.T;
    cib = cib < WG_HALO_MAX / a.HV ? cib : WG_HALO_MAX / a.HV;
    cib = cib < g.Cin ? cib : g.Cin;
    a.CIB = cib < 1 ? 1 : cib;
    a.nci = cdiv(g.Cin, a.CIB);
    a.co_tiles = cdiv(g.Cout, 32);
    a.nbx = cdiv(a.OW, WG_BOX_X);
    a.nby = cdiv(a.OH, WG_BOX_Y);
    a.nbz = cdiv(a.OD, WG_BOX_Z);
    a.nboxes = g.N * a.nbx * a.nby * a.nbz;
    const int base = a.nci * a.co_tiles;
    int nsplit = cdiv(1024, base);
    nsplit = nsplit < a.nboxes ? nsplit : a.nboxes;
    a.boxes_per_split = cdiv(a.nboxes, nsplit);
    pl.nsplit = cdiv(a.nboxes, a.boxes_per_split);
    pl.lds = (size_t)(32 * WG_PA + a.CIB * a.HV) * sizeof(float);
    pl.ws_bytes = (size_t)pl.nsplit * g.Cout * g.Cin * a.T * sizeof(float);
}

// Output phases of backward-data along one axis (input size `in`, kernel k, stride s, padding p): phase r covers
// dx positions i = s*m + r - p, m in [m0, m0 + Q); it reads dy at m - (T-1) + u with the filter tap r + s*(T-1-u).
struct Phase {
    int Q, os, oo, ib, T, kb, ks;
};
static int floordiv(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
static Phase make_phase(int in, int k, int s, int p, int r) {
    Phase ph;
    ph.T = r < k ? (k - r + s - 1) / s : 0;
    const int m0 = -floordiv(r - p, s);                    // ceil((p - r) / s)
    const int m1 = floordiv(in - 1 - r + p, s);           // last m with i < in
    ph.Q = m1 >= m0 ? m1 - m0 + 1 : 0;
    ph.os = s;
    ph.oo = s * m0 + r - p;
    ph.ib = m0 - ph.T + 1;
    ph.kb = r + s * (ph.T - 1);
    ph.ks = -s;
    return ph;
}

}  // namespace gen
}  // namespace dram

using namespace dram;
using namespace dram::gen;

extern "C" int dram_conv3d_fwd(const float* x, const float* w, const float* bias, float* y, int N, int Cin, int Cout, int D,
                               int H, int W, int kz, int ky, int kx, int sz, int sy, int sx, int pz, int py, int px,
                               void* stream) {
    Geom g;
    int rc = check_geom("conv3d_fwd", g, N, Cin, Cout, D, H, W, kz, ky, kx, sz, sy, sx, pz, py, px);
    if (rc) return rc;
    DRAM_REQUIRE(x && w && y, "conv3d_fwd: null pointer");
    GenArgs a = {};
    a.x = x; a.w = w; a.bias = bias; a.y = y;
    a.N = N; a.C = Cin; a.M = Cout;
    a.ID = D; a.IH = H; a.IW = W;
    a.OD = a.QD = g.o[0]; a.OH = a.QH = g.o[1]; a.OW = a.QW = g.o[2];
    a.osz = a.osy = a.osx = 1;
    a.isz = sz; a.isy = sy; a.isx = sx;
    a.ibz = -pz; a.iby = -py; a.ibx = -px;
    a.Tz = kz; a.Ty = ky; a.Tx = kx;
    a.Ky = ky; a.Kx = kx;
    a.ksz = a.ksy = a.ksx = 1;
    a.wsm = Cin * kz * ky * kx;
    a.wsk = kz * ky * kx;
    a.wbytes = 4u * (unsigned)((int64_t)Cout * Cin * kz * ky * kx);
    rc = launch_fwd(a, (hipStream_t)stream);
    if (rc == DRAM_OK) g_launches[DRAM_CONV_GEN_FWD].fetch_add(1, std::memory_order_relaxed);
    return rc;
}

extern "C" int dram_conv3d_bwd_data(const float* dy, const float* w, float* dx, int N, int Cin, int Cout, int D, int H,
                                    int W, int kz, int ky, int kx, int sz, int sy, int sx, int pz, int py, int px,
                                    void* stream) {
    Geom g;
    int rc = check_geom("conv3d_bwd_data", g, N, Cin, Cout, D, H, W, kz, ky, kx, sz, sy, sx, pz, py, px);
    if (rc) return rc;
    DRAM_REQUIRE(dy && w && dx, "conv3d_bwd_data: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int in[3] = {D, H, W};
    bool empty_phase = false;
    for (int ax = 0; ax < 3; ++ax)
        for (int r = 0; r < g.s[ax]; ++r) {
            const Phase ph = make_phase(in[ax], g.k[ax], g.s[ax], g.p[ax], r);
            if (ph.Q > 0 && ph.T == 0) empty_phase = true;
        }
    if (empty_phase) {   // positions no tap reaches (kernel smaller than the stride): their gradient is 0
        const hipError_t e = hipMemsetAsync(dx, 0, (size_t)N * Cin * D * H * W * sizeof(float), st);
        DRAM_REQUIRE(e == hipSuccess, "conv3d_bwd_data: hipMemsetAsync failed: %s", hipGetErrorString(e));
    }
    for (int rz = 0; rz < g.s[0]; ++rz)
        for (int ry = 0; ry < g.s[1]; ++ry)
            for (int rx = 0; rx < g.s[2]; ++rx) {
                const Phase pz_ = make_phase(D, kz, sz, pz, rz), py_ = make_phase(H, ky, sy, py, ry),
                            px_ = make_phase(W, kx, sx, px, rx);
                if (pz_.T == 0 || py_.T == 0 || px_.T == 0) continue;
                GenArgs a = {};
                a.x = dy; a.w = w; a.bias = nullptr; a.y = dx;
                a.N = N; a.C = Cout; a.M = Cin;
                a.ID = g.o[0]; a.IH = g.o[1]; a.IW = g.o[2];
                a.OD = D; a.OH = H; a.OW = W;
                a.QD = pz_.Q; a.QH = py_.Q; a.QW = px_.Q;
                a.osz = pz_.os; a.osy = py_.os; a.osx = px_.os;
                a.ooz = pz_.oo; a.ooy = py_.oo; a.oox = px_.oo;
                a.isz = a.isy = a.isx = 1;
                a.ibz = pz_.ib; a.iby = py_.ib; a.ibx = px_.ib;
                a.Tz = pz_.T; a.Ty = py_.T; a.Tx = px_.T;
                a.Ky = ky; a.Kx = kx;
                a.kbz = pz_.kb; a.kby = py_.kb; a.kbx = px_.kb;
                a.ksz = pz_.ks; a.ksy = py_.ks; a.ksx = px_.ks;
                a.wsm = kz * ky * kx;          // A[m = input channel][c = output channel] = w[c][m]
                a.wsk = Cin * kz * ky * kx;
                a.wbytes = 4u * (unsigned)((int64_t)Cout * Cin * kz * ky * kx);
                rc = launch_fwd(a, st);
                if (rc) return rc;
                if (a.QD > 0 && a.QH > 0 && a.QW > 0) g_launches[DRAM_CONV_GEN_BWD_DATA].fetch_add(1, std::memory_order_relaxed);
            }
    return DRAM_OK;
}

extern "C" size_t dram_conv3d_wgrad_ws_bytes(int N, int Cin, int Cout, int D, int H, int W, int kz, int ky, int kx, int sz,
                                             int sy, int sx, int pz, int py, int px) {
    Geom g;
    if (check_geom("conv3d_wgrad_ws_bytes", g, N, Cin, Cout, D, H, W, kz, ky, kx, sz, sy, sx, pz, py, px)) return 0;
    WgradPlan pl;
    wgrad_plan(g, pl);
    return pl.ws_bytes;
}

extern "C" int dram_conv3d_wgrad(const float* x, const float* dy, float* dw, void* ws, size_t ws_bytes, int N, int Cin,
                                 int Cout, int D, int H, int W, int kz, int ky, int kx, int sz, int sy, int sx, int pz, int py,
                                 int px, void* stream) {
    Geom g;
    int rc = check_geom("conv3d_wgrad", g, N, Cin, Cout, D, H, W, kz, ky, kx, sz, sy, sx, pz, py, px);
    if (rc) return rc;
    DRAM_REQUIRE(x && dy && dw, "conv3d_wgrad: null pointer");
    WgradPlan pl;
    wgrad_plan(g, pl);
    if (ws_bytes < pl.ws_bytes || ws == nullptr) {
        set_error("conv3d_wgrad: workspace of %zu bytes, %zu needed", ws_bytes, pl.ws_bytes);
        return DRAM_EWS;
    }
    pl.a.x = x;
    pl.a.dy = dy;
    pl.a.slabs = (float*)ws;
    hipStream_t st = (hipStream_t)stream;
    if (pl.lds > 65536) {
        rc = ensure_dynamic_lds((const void*)conv3d_gen_wgrad_kernel, pl.lds, g_lds_wgrad, "conv3d_wgrad");
        if (rc) return rc;
    }
    const int64_t blocks = (int64_t)pl.nsplit * pl.a.nci * pl.a.co_tiles;
    hipLaunchKernelGGL(conv3d_gen_wgrad_kernel, dim3((unsigned)blocks), dim3(256), pl.lds, st, pl.a);
    rc = check_launch("conv3d_gen_wgrad");
    if (rc) return rc;
    const int64_t E = (int64_t)Cout * Cin * pl.a.T;
    hipLaunchKernelGGL(gen_slab_reduce_kernel, dim3((unsigned)cdiv64(E, 256)), dim3(256), 0, st, (const float*)ws, dw, E,
                       pl.nsplit);
    rc = check_launch("conv3d_gen_wgrad(reduce)");
    if (rc == DRAM_OK) g_launches[DRAM_CONV_GEN_WGRAD].fetch_add(1, std::memory_order_relaxed);
    return rc;
}

extern "C" int dram_conv3d_gen_launch_counts(unsigned long long* counts, int n) {
    DRAM_REQUIRE(counts && n > 0, "conv3d_gen_launch_counts: null pointer");
    for (int i = 0; i < n; ++i) counts[i] = i < DRAM_CONV_GEN_KINDS ? g_launches[i].load(std::memory_order_relaxed) : 0ull;
    return DRAM_OK;
}
