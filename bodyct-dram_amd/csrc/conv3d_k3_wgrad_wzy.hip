// 3x3x3 convolution, backward-weights with the transpose of Winograd F(2x2,3x3) over (z,y): the kernel and its table
// rows.  The other 3x3x3 kernels and the design common to all of them: conv3d_k3.hip.
#include "conv_args.h"
#include "conv_device.h"

namespace dram {

// ---------------------------------------------------------------------------------------------
// backward-weights with the transpose of Winograd F(2x2, 3x3) over (z, y) -- exact fp32 arithmetic, 4/9 of the direct
// MFMAs (2/3 of the z-only kernel's).
//
// For a 2x2 (z,y) tile e of output gradients and the 4x4 input patch d around it (per x, co, ci; the x taps stay direct)
//     E' = A e A^T,   V = B^T d B,   P[xi] += E'[xi] * V[xi](x + kx),   dg[:, :, kx] = G^T P G
// (the transpose of the forward algorithm of conv3d_k3_fwd_wzy_kernel: same B^T, G, A) -- 16 products per (co, ci, kx) and
// 4 voxels instead of 36; in GEMM terms 48 independent accumulators (16 xi x 3 kx) per (co, ci) pair with K = the positions
// (x, y pair, z pair) of the volume, on v_mfma_f32_16x16x4_f32.
//
// What made the z-only kernel lose 17-22 % to staging, and the (z,y) form look worse on paper (2.1x the staged floats per
// MFMA: DESIGN.md section 3), is avoided by construction:
//   * block = 512 threads, ONE per CU: wave = (row xi_z = q of the transformed tile, 32-channel half of the 64 co x 16 ci block
//     tile) -- 2 co tiles x 12 (kx, xi_y) accumulators = 96 registers -- two per SIMD, so that one wave's scalar / vector /
//     LDS instructions issue under its partner's MFMAs (a first version with ONE wave per SIMD and 192 accumulators each ran
//     at 0.55-0.6 of the matrix peak: every run of non-matrix instructions between two MFMAs of the only wave was matrix
//     time lost, and spreading them out by hand drowned in the register allocator's accumulator copies);
//   * nothing that comes from memory ever waits in a register: BOTH operands go global -> LDS by LDS-DMA (buffer_load ...
//     lds), two boxes ahead, and the only wait is the one in front of the box's barrier.  With a single wave per SIMD a
//     load that is waited for stops the matrix pipe: the first version staged X through registers one box ahead and ran at
//     190 TFLOP/s direct-equivalent with its loads and 263-290 without them;
//   * dY is NOT transformed on the way into LDS (that would be a 4x expansion: 2x2 -> 4x4): a wave forms its row of E' from
//     the four raw values after reading them (6 vector instructions per co tile and k-step, feeding 12 MFMAs each);
//   * X lands raw in a ring of plane slots [slot][ci][4 rows][20]; a block walks z columns (z pair fastest), so two of a
//     box's four planes are the previous box's last two and are not fetched again (2.25x instead of 4.5x halo traffic);
//     one LDS -> LDS pass per box (a 4x4 patch per lane: 16 reads, normalise + ReLU where the source is lazy, 32 adds, 16
//     stores) produces V one box ahead of its use, in pieces that ride between the wave's own MFMAs;
//   * one barrier per box.
// Box = 16 x positions x one y pair x one z pair (64 voxels, K = 16 per xi).  LDS reads are conflict-free by layout: dY chunks
// are permuted inside an LDS-DMA group (chunk = 16 row + 4 (co % 4) + x / 4, groups of 4 channels 65 chunks apart), V rows
// are 20 floats apart (4 x odd).  Deterministic like the other kernels: per-block partial slabs, fixed-order reduce.
// Serves W % 4 == 0 covered by 16-wide boxes with at most 1.3x padding (a ragged last box fetches zeros for its columns beyond
// W: the reference's 40^3 level), even H and D, channel tiles inside one source tensor (wgrad_plan); everything else: the z-only kernel.
struct WgradWzyGeom {
    static constexpr int CI_B = 16;
    static constexpr int CS = 20;                       // floats per (xi, ci) row: 18 halo columns + 2
    static constexpr int XIS = CI_B * CS;               // floats per transformed plane xi
    static constexpr int X_FLOATS = 16 * XIS;           // one V stage
    static constexpr int DY_GROUP = 65 * 4;             // floats per LDS-DMA group: 4 channels x 64 voxels + one 16-byte pad
    static constexpr int DY_FLOATS = 16 * DY_GROUP;     // 64 channels
    static constexpr int RCS = 24;                      // floats per raw row: x0 - 4 .. x0 + 19 (six aligned 16-byte chunks)
    static constexpr int RAWP = CI_B * 4 * RCS;         // one raw plane slot: [ci][row][24]
    static constexpr int NDY = 3;                       // dY stages: the box multiplied + two fetched ahead
    static constexpr int NSLOT = 8;                     // raw plane slots: 4 (box being transformed) + 2 (+ 2 where a column starts)
    static constexpr size_t LDS_BYTES = (size_t)(NDY * DY_FLOATS + 2 * X_FLOATS + NSLOT * RAWP) * sizeof(float);
};

template <bool LAZY>
__global__ __launch_bounds__(512, 1) void conv3d_k3_wgrad_wzy_kernel(WgradArgs a, int boxes_per_block) {
    using G = WgradWzyGeom;
    constexpr int CS = G::CS, XIS = G::XIS, DYG = G::DY_GROUP, DYF = G::DY_FLOATS, XF = G::X_FLOATS, RAWP = G::RAWP;
    constexpr int NSLOT = G::NSLOT, NDY = G::NDY, RCS = G::RCS;

    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* const ldv = lds + NDY * DYF;             // dY stages [NDY][DYF], V stages [2][XF], raw plane ring [NSLOT][RAWP]
    float* const ldr = ldv + 2 * XF;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q = wave & 3, cohalf = wave >> 2;         // wave = (xi_z, 32-channel half); waves w and w + 4 share a SIMD
    int b = xcd_remap(blockIdx.x, gridDim.x);       // logical item = (split, co tile, ci tile), ci tile fastest
    const int ci_t = b % a.ci_tiles; b /= a.ci_tiles;
    const int co_t = b % a.co_tiles;
    const int sp = b / a.co_tiles;
    const int ci0 = (ci_t + a.ci_tile0) * 16, co0 = co_t * 64;
    const int D = a.D, H = a.H, W = a.W;
    const int S = D * H * W;
    const bool use2 = a.src.p2 != nullptr && ci0 >= a.src.C1;
    const int Hs = use2 ? a.src.H2 : H, Ws = use2 ? a.src.W2 : W;
    const int Ss = use2 ? a.src.D2 * a.src.H2 * a.src.W2 : S;
    const int oz = use2 ? a.src.oz : 0, oy = use2 ? a.src.oy : 0, ox = use2 ? a.src.ox : 0;
    const int Cs = use2 ? a.src.C2 : a.src.C1;
    const int cs0 = use2 ? ci0 - a.src.C1 : ci0;
    const float* xs = use2 ? a.src.p2 : a.src.p1;
    const unsigned S4 = 4u * (unsigned)S, Ss4 = 4u * (unsigned)Ss;

    // ---- box range of this block (z pair fastest, then x, y, n)
    const int box_lo = sp * boxes_per_block;
    const int box_hi = (box_lo + boxes_per_block) < a.nboxes ? (box_lo + boxes_per_block) : a.nboxes;
    const int nbox = box_hi - box_lo;
    const int i = lane & 15, k = lane >> 4;
    // The sums as the epilogue takes them: waves 0 .. 3: co tile 0 (fin[0]); waves 4 .. 7: co tiles 1, 2, 3.  The accumulators
    // themselves live inside the per-role pipeline (run): with one array for all roles the 96 registers of tiles 1, 2 stayed
    // live -- holding zeros -- through the loop of waves 0 .. 3, whose fetch / transform state was then spilled to scratch and
    // reloaded every box (13 scratch loads per box on the critical waves; scratch traffic also counts in vmcnt).
    f32x4 fin[3][12];               // (every path assigns all of it AFTER its loop: zeros that are live through the loop cost registers too)

    if (nbox > 0) {
        // cursor of the next box to be fetched, and the ring of raw planes
        int s_bx, s_by, s_bz, s_n;
        {
            int bb = box_lo;
            s_bz = bb % a.nbz; bb /= a.nbz;
            s_bx = bb % a.nbx; bb /= a.nbx;
            s_by = bb % a.nby;
            s_n = bb / a.nby;
        }
        int ring = 0;               // planes fetched so far: the next one goes to slot ring % NSLOT
        bool first = true;

        // Division of labour inside a SIMD pair (waves w and w + 4): waves 0 .. 3 issue the FETCH (all LDS-DMA instructions), run the
        // TRANSFORM pass (with half of wave 4) and multiply ONE co tile; waves 4 .. 7 multiply the other THREE and do nothing
        // else -- a wave's scalar / vector instructions are issued instead of its own MFMAs, so the matrix pipe is only kept
        // busy through them by the partner's MFMAs (s_memtime stamps: with the work split evenly both partners ran the same
        // phases at the same time and a box took 8,700 cycles for 6,144 of matrix work).
        const int fw = wave & 3;
        // ---- dY by LDS-DMA: fetcher fw moves groups 4 fw .. 4 fw + 3 (4 channels each); lane = chunk 16 r + 4 c + s (r = 2 z + y
        // row, c = channel inside the group, s = x / 4).  Channels >= Cout and -- in the last box of a row whose width is not a
        // multiple of 16 -- pieces at x >= W: offset beyond the descriptor -> zeros (a zero dY column contributes nothing,
        // whatever X holds there).  Set where a z column starts (fetch_piece 0).
        unsigned dvoff[4] = {0xC0000000u, 0xC0000000u, 0xC0000000u, 0xC0000000u};
        // ---- raw X planes by LDS-DMA, 16 bytes per lane: a plane slot is [16 ci][4 rows][24]: a row = the six aligned chunks
        // x0 - 4 .. x0 + 19 around the 18 columns a box needs (an LDS-DMA instruction costs the issuing wave ~150 cycles wherever
        // it is placed -- s_memtime -- so there must be few of them: 6 per plane instead of the 20 a dword fetch of exactly the 18
        // columns took; both forms touch the same two 128-byte lines per row).  Instruction m (0 .. 5) of a plane is issued by wave
        // m % 4; lane l of it = chunk q = 64 m + l = (ci = q / 24, row = (q % 24) / 6, chunk = q % 6).  W % 4 == 0: a chunk is inside or
        // outside the volume as a whole.  The descriptor's base is moved back by one plane + one row + four elements, so that
        // every offset component (lane part, box part, plane part) is non-negative; what lies before the tensor is never read:
        // rows and chunks outside the volume get an out-of-range lane offset, planes outside a zero-size descriptor.
        const unsigned xmargin = 4u * (unsigned)(Hs * Ws + Ws + 4);
        constexpr int NXI = 2;
        const int nxi = fw < 2 ? 2 : 1;             // this wave's instructions per plane: m = fw (and fw + 4)
        unsigned xvoff[NXI];
        unsigned xflags = 0;           // per instruction 8 bits: chunk 0 / - / row 0 / row 3 (what a box at the border drops), chunk number << 4
#pragma unroll
        for (int m = 0; m < NXI; ++m) {
            const int qc = 64 * (fw + 4 * m) + lane;
            const int pci = qc / 24, row = (qc % 24) / 6, chk = qc % 6;
            const int ch = cs0 + pci;
            xvoff[m] = (qc < 384 && ch < Cs) ? (unsigned)ch * Ss4 + 4u * (unsigned)(4 * chk + ox + (row + oy + oz * Hs) * Ws) : 0xC0000000u;
            xflags |= ((chk == 0 ? 1u : 0u) | (row == 0 ? 4u : 0u) | (row == 3 ? 8u : 0u) | ((unsigned)chk << 4)) << (8 * m);
        }
        const unsigned plane4 = 4u * (unsigned)(Hs * Ws);

        // geometry of the (up to two) boxes that are fetched and wait for their transform: q0 the older, q1 the newer
        int q0_x0 = 0, q0_y0 = 0, q0_z0 = 0, q0_head = 0, q0_n = 0;     // head: ring position behind the box's last plane
        int q1_x0 = 0, q1_y0 = 0, q1_z0 = 0, q1_head = 0, q1_n = 0;

        // The fetch of one box in pieces (they ride between the wave's MFMAs; the SIMD partner's MFMAs cover them):
        //   0: geometry + the dY descriptor + the two LDS-DMA groups of dY;  1 + pi: the pi-th fetched plane: descriptor, ring
        //   slot, this wave's two or three LDS-DMA instructions (planes 2, 3; all four where the box starts a z column:
        //   otherwise planes 0, 1 are the previous box's 2, 3, already in the ring).
        bool c_fresh = true;
        int c_x0 = 0, c_y0 = 0, c_z0 = 0;
        unsigned c_emask = 0;
        // per z column (a column is nbz boxes of one sample: bases and in-plane offsets are computed where it starts, not per box)
        const float* col_dy = nullptr;  // sample n of dY
        const float* col_xb = nullptr;  // sample n of X, moved back by xmargin
        unsigned col_off = 0, col_xoff = 0;     // byte offset of (y0, x0) inside a plane of dY / X
        const unsigned dplane4 = 4u * (unsigned)(H * W);
        unsigned xvo[NXI];              // xvoff with the current column's border elements out of range
#pragma unroll
        for (int m = 0; m < NXI; ++m) xvo[m] = xvoff[m];
        constexpr int NFP = 5;
        auto fetch_piece = [&](auto is_fetcher, int dy_float, int piece) {       // (the role as a TYPE: as a runtime flag it kept the
                                                                                 //  fetch state live -- and spilled -- in waves 4 .. 7)
            if constexpr (!decltype(is_fetcher)::value) {   // (the cursor state every wave keeps: the transform pass reads it through fetch_done)
                if (piece == 0) { c_z0 = s_bz * 2; c_fresh = first || c_z0 == 0; first = false; }
                else if (piece - 1 < (c_fresh ? 4 : 2)) ++ring;
                return;
            }
            if (piece == 0) {
                c_x0 = s_bx * 16; c_y0 = s_by * 2; c_z0 = s_bz * 2;
                c_fresh = first || c_z0 == 0;
                first = false;
                if (c_fresh) {          // a new z column (once per nbz boxes): which of this lane's elements its x / y borders drop
                    c_emask = (c_x0 == 0 ? 1u : 0u) | (c_y0 == 0 ? 4u : 0u) | (c_y0 + 2 == H ? 8u : 0u);
                    const unsigned remq = (unsigned)(W - c_x0) >> 2;        // 16-byte pieces of the box's 16 columns inside the volume
#pragma unroll
                    for (int m = 0; m < NXI; ++m) {     // X chunk k holds x0 - 4 + 4 k ..: inside iff k <= remq (and k > 0 at the left border)
                        const unsigned fl = xflags >> (8 * m);
                        xvo[m] = ((fl & c_emask) || ((fl >> 4) & 7u) > remq) ? 0xC0000000u : xvoff[m];
                    }
                    {
                        const int r = lane >> 4, c = (lane >> 2) & 3, sx = lane & 3;
#pragma unroll
                        for (int m = 0; m < 4; ++m) {
                            const int co = co0 + 4 * (4 * fw + m) + c;
                            dvoff[m] = (co < a.Cout && (unsigned)sx < remq)
                                           ? (unsigned)co * S4 + 4u * (unsigned)(((r >> 1) * H + (r & 1)) * W + 4 * sx) : 0xC0000000u;
                        }
                    }
                    col_dy = uniform_ptr(a.dy + (size_t)s_n * a.Cout * S);
                    col_xb = uniform_ptr((const float*)((const char*)(xs + (size_t)s_n * Cs * Ss) - xmargin));
                    col_off = 4u * (unsigned)(c_y0 * W + c_x0);
                    col_xoff = 4u * (unsigned)(c_y0 * Ws + c_x0);
                }
                const __amdgpu_buffer_rsrc_t srd = make_rsrc(col_dy, (unsigned)a.Cout * S4);
                const unsigned off = col_off + (unsigned)c_z0 * dplane4;
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(srd, (lds_ptr_t)(lds + dy_float + (4 * fw + m) * DYG), 16, (int)dvoff[m], (int)off, 0, 0);
                return;
            }
            const int pi = piece - 1;
            if (pi >= 2 && !c_fresh) return;
            const int rz = c_fresh ? pi : pi + 2;
            const int gz = c_z0 - 1 + rz;
            const unsigned bytes = (unsigned)gz < (unsigned)D ? (unsigned)Cs * Ss4 + xmargin : 0u;      // a plane outside the volume: zeros
            const __amdgpu_buffer_rsrc_t xsrd = make_rsrc(col_xb, bytes);
            const unsigned soff = col_xoff + (unsigned)(c_z0 + rz) * plane4;
            const int slot_float = NDY * DYF + 2 * XF + (ring % NSLOT) * RAWP;      // (ring counts planes: non-negative)
            ++ring;
#pragma unroll
            for (int m = 0; m < NXI; ++m) {
                if (m == 1 && nxi < 2) continue;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(xsrd, (lds_ptr_t)(lds + slot_float + 256 * (fw + 4 * m)), 16, (int)xvo[m], (int)soff, 0, 0);
            }
        };
        auto fetch_done = [&](bool to_q0) {       // the cursor's box is fetched: remember it for its transform, move on
            if (to_q0) {
                q0_x0 = s_bx * 16; q0_y0 = s_by * 2; q0_z0 = s_bz * 2; q0_n = s_n; q0_head = ring;
            } else {
                q1_x0 = s_bx * 16; q1_y0 = s_by * 2; q1_z0 = s_bz * 2; q1_n = s_n; q1_head = ring;
            }
            if (++s_bz == a.nbz) {
                s_bz = 0;
                if (++s_bx == a.nbx) {
                    s_bx = 0;
                    if (++s_by == a.nby) { s_by = 0; ++s_n; }
                }
            }
        };

        // ---- the LDS -> LDS pass: patch p = (ci = p / 18, halo column hx = p % 18); thread tid < 256 (waves 0 .. 3) transforms
        // patch tid, and the last 32 patches (256 .. 287) go to one of those waves in turn (never to waves 4 .. 7: they carry
        // three quarters of the MFMAs).
        //   piece 4 u + 0: the 16 raw reads;  + 1: normalise + ReLU (the zero padding belongs to the ACTIVATED tensor) and B^T d
        //   along z;  + 2, + 3: (.) B along y of rows xi_z = 0, 1 / 2, 3 -> eight LDS stores each
        int p_raw[2], p_lds[2], p_row[2], p_hx[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int p = u == 0 ? (tid & 255) : 256 + (lane & 31);
            const int pci = p / 18, phx = p % 18;
            p_raw[u] = pci * (4 * RCS) + phx + 3;
            p_lds[u] = pci * CS + phx;
            p_row[u] = min(cs0 + pci, Cs - 1);
            p_hx[u] = cs0 + pci < Cs ? phx : -1000;      // (a channel beyond the tensor: treated like a column outside the volume)
        }
        const float* cf = LAZY ? (use2 ? a.coef2 : a.coef1) : nullptr;   // block-uniform; null: this source is plain
        const float lo = (LAZY && (use2 ? a.relu2 : a.relu1)) ? 0.f : -INFINITY;
        float rin[4][4];                // [plane rz][row ry] of the patch in work
        // geometry of the box being transformed (a copy: the fetch cursor moves on meanwhile)
        int t_x0 = 0, t_y0 = 0, t_z0 = 0, t_head = 0, t_n = 0, t_ord = 0;
        int cf_n = -1;                  // the sample whose coefficients are cached (lazy sources)
        float cf_a[2] = {1.f, 1.f}, cf_b[2] = {0.f, 0.f};
        auto transform_begin = [&](auto is_fetcher) {       // takes the older waiting box; the newer one moves up
            t_x0 = q0_x0; t_y0 = q0_y0; t_z0 = q0_z0; t_head = q0_head; t_n = q0_n;
            q0_x0 = q1_x0; q0_y0 = q1_y0; q0_z0 = q1_z0; q0_head = q1_head; q0_n = q1_n;
            ++t_ord;
            if constexpr (!decltype(is_fetcher)::value) return;
            if (LAZY && cf && t_n != cf_n) {        // a new sample (once per 10^4 boxes): its rows' {a, b}
                cf_n = t_n;
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const float2 ab = *reinterpret_cast<const float2*>(cf + 2 * ((int64_t)t_n * Cs + p_row[u]));
                    cf_a[u] = ab.x; cf_b[u] = ab.y;
                }
                // Waited for HERE, once per sample: left to the compiler, the wait sits at the first use in the transform pass of
                // EVERY box (the rarely taken branch merges there) as `s_waitcnt vmcnt(1)` -- and vmcnt counts the LDS-DMA fetch
                // of the boxes ahead too, so the transforming waves sat out most of a memory latency per box (+650 cycles).
                __builtin_amdgcn_s_waitcnt(0x0F70);          // vmcnt(0)
            }
        };
        auto transform_piece = [&](auto is_fetcher, int v_float, int piece8) {
            if constexpr (!decltype(is_fetcher)::value) return;
            const int u = piece8 >> 2, piece = piece8 & 3;
            if (u == 1 && ((t_ord & 3) != wave || lane >= 32)) return;
            if (piece == 0) {
#pragma unroll
                for (int rz = 0; rz < 4; ++rz) {
                    const float* pl = ldr + ((t_head - 4 + rz) % NSLOT) * RAWP + p_raw[u];      // (t_head >= 4)
#pragma unroll
                    for (int ry = 0; ry < 4; ++ry) rin[rz][ry] = pl[ry * RCS];
                }
            } else if (piece == 1) {
                if (LAZY && cf) {
                    const bool colok = (unsigned)(t_x0 - 1 + p_hx[u]) < (unsigned)W;
                    const float ca = cf_a[u], cb = colok ? cf_b[u] : 0.f, fl = colok ? lo : 0.f;   // (a column outside: zeros in, zeros out)
                    const bool yz_edge = t_y0 == 0 || t_y0 + 2 == H || t_z0 == 0 || t_z0 + 2 == D;
                    if (!yz_edge) {
                        const f32x2 ca2 = {ca, ca}, cb2 = {cb, cb}, fl2 = {fl, fl};
#pragma unroll
                        for (int rz = 0; rz < 4; ++rz) {
#pragma unroll
                            for (int h = 0; h < 2; ++h) {     // two rows at a time: v_pk_fma_f32 (max: per component)
                                const f32x2 v = {rin[rz][2 * h], rin[rz][2 * h + 1]};
                                const f32x2 w = __builtin_elementwise_fma(ca2, v, cb2);
                                rin[rz][2 * h] = fmaxf(w[0], fl2[0]);
                                rin[rz][2 * h + 1] = fmaxf(w[1], fl2[1]);
                            }
                        }
                    } else {
#pragma unroll
                        for (int rz = 0; rz < 4; ++rz) {
                            const bool zok = (unsigned)(t_z0 - 1 + rz) < (unsigned)D;
#pragma unroll
                            for (int ry = 0; ry < 4; ++ry) {
                                const bool ok = zok && (unsigned)(t_y0 - 1 + ry) < (unsigned)H;
                                rin[rz][ry] = ok ? fmaxf(fmaf(ca, rin[rz][ry], cb), fl) : 0.f;
                            }
                        }
                    }
                }
#pragma unroll
                for (int h = 0; h < 2; ++h) {         // B^T d along z, two rows at a time: v_pk_add_f32
                    const f32x2 d0 = {rin[0][2 * h], rin[0][2 * h + 1]}, d1 = {rin[1][2 * h], rin[1][2 * h + 1]};
                    const f32x2 d2 = {rin[2][2 * h], rin[2][2 * h + 1]}, d3 = {rin[3][2 * h], rin[3][2 * h + 1]};
                    const f32x2 o0 = d0 - d2, o1 = d1 + d2, o2 = d2 - d1, o3 = d1 - d3;
                    rin[0][2 * h] = o0[0]; rin[0][2 * h + 1] = o0[1]; rin[1][2 * h] = o1[0]; rin[1][2 * h + 1] = o1[1];
                    rin[2][2 * h] = o2[0]; rin[2][2 * h + 1] = o2[1]; rin[3][2 * h] = o3[0]; rin[3][2 * h + 1] = o3[1];
                }
            } else {
                float* o = lds + v_float + p_lds[u];
#pragma unroll
                for (int rz = 2 * (piece - 2); rz < 2 * (piece - 2) + 2; ++rz) {
                    const float d0 = rin[rz][0], d1 = rin[rz][1], d2 = rin[rz][2], d3 = rin[rz][3];
                    o[(4 * rz + 0) * XIS] = d0 - d2;
                    o[(4 * rz + 1) * XIS] = d1 + d2;
                    o[(4 * rz + 2) * XIS] = d2 - d1;
                    o[(4 * rz + 3) * XIS] = d1 - d3;
                }
            }
        };
        // where the pieces ride: behind group `slot` (0 .. 47: two MFMAs each) of a box
        constexpr int FSLOT0 = 1, TSLOT0 = 12, TSTEP = 4;       // fetch piece p behind slot FSLOT0 + 2 p, transform piece p behind TSLOT0 + TSTEP p

        // ---- compute role.  A: raw dY chunk of (co = 16 ct + i, row r, x = 4 ks + k) at float 4 (65 g + 16 r + 4 c + ks) + k,
        // g = 4 ct + i / 4, c = i % 4; this wave's co tiles are ct = 2 cohalf, 2 cohalf + 1.  Row xi_z = Q of E' = A e A^T:
        // (u0, u0 + u1, u0 - u1, u1) with (u0, u1) = e[0][:], e[0][:] + e[1][:], e[0][:] - e[1][:], e[1][:] for Q = 0 .. 3 -- the last
        // entry and the last row are the NEGATIVES of the true ones, put right in the epilogue.  B: V[xi = 4 Q + xi_y][ci][x + kx].
        // The pipeline is instantiated once per Q behind one wave-uniform branch: rows 0 and 3 need two of the four raw values
        // and no arithmetic for (u0, u1).
        const int abase = 4 * (65 * (i >> 2) + 4 * (i & 3)) + k + cohalf * (4 * DYG);      // first co tile: 0 (waves 0-3) / 1 (waves 4-7)
        const int bbase = 4 * q * XIS + i * CS + k;

        auto run = [&](auto role) {
            constexpr int Q = decltype(role)::value & 3;
            constexpr int NCT = (decltype(role)::value >> 2) ? 3 : 1;       // co tiles of this wave: the transforming waves 0 .. 3
            constexpr std::integral_constant<bool, (decltype(role)::value < 4)> IS_FETCHER{};
            f32x4 acc[NCT][12];
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                for (int g = 0; g < 12; ++g) acc[ct][g] = f32x4{0.f, 0.f, 0.f, 0.f};
            constexpr int R0 = Q == 3 ? 2 : 0;                      // take one, the fetching waves 4 .. 7 three: the pair's
            constexpr int NR = (Q == 0 || Q == 3) ? 2 : 4;          // non-matrix work is uneven the other way round
            float ar[2][NCT][NR];       // raw dY of the current / next k-step: [set][ct][row - R0]
            float bv[3];                // B operands: a ring over the groups
            // The last NDEF groups of a box are issued behind the barrier, after the next box's first operand reads: their MFMAs
            // cover the LDS latency every wave would otherwise sit out with an empty matrix pipe at the start of a box.
            constexpr int NDEF = NCT == 3 ? 2 : 4;
            float pav[NCT][4], pbv[NDEF];
            bool pending = false;

            // the MFMAs of one box (48 groups of NCT); `ride(slot)` runs behind group `slot`
            auto compute_box = [&](int dy_float, int v_float, auto&& ride) {
                const float* dyst = lds + dy_float;
                const float* vst = lds + v_float;
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                    for (int r = 0; r < NR; ++r) ar[0][ct][r] = dyst[abase + ct * (4 * DYG) + (R0 + r) * 64];
#pragma unroll
                for (int g = 0; g < 2; ++g) bv[g] = vst[bbase + (g & 3) * XIS + (g >> 2)];
                if (pending) {
#pragma unroll
                    for (int d = 0; d < NDEF; ++d)
#pragma unroll
                        for (int ct = 0; ct < NCT; ++ct)
                            acc[ct][12 - NDEF + d] = __builtin_amdgcn_mfma_f32_16x16x4f32(pav[ct][(12 - NDEF + d) & 3], pbv[d], acc[ct][12 - NDEF + d], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    float av[NCT][4];
#pragma unroll
                    for (int ct = 0; ct + 1 < NCT; ct += 2) {        // two co tiles at a time: v_pk_add_f32
                        const float* ea = ar[ks & 1][ct];
                        const float* eb = ar[ks & 1][ct + 1];
                        f32x2 u0, u1;
                        if (NR == 2) { u0 = f32x2{ea[0], eb[0]}; u1 = f32x2{ea[1], eb[1]}; }
                        else if (Q == 1) { u0 = f32x2{ea[0], eb[0]} + f32x2{ea[2], eb[2]}; u1 = f32x2{ea[1], eb[1]} + f32x2{ea[3], eb[3]}; }
                        else { u0 = f32x2{ea[0], eb[0]} - f32x2{ea[2], eb[2]}; u1 = f32x2{ea[1], eb[1]} - f32x2{ea[3], eb[3]}; }
                        const f32x2 s01 = u0 + u1, d01 = u0 - u1;
                        av[ct][0] = u0[0]; av[ct + 1][0] = u0[1];
                        av[ct][1] = s01[0]; av[ct + 1][1] = s01[1];
                        av[ct][2] = d01[0]; av[ct + 1][2] = d01[1];
                        av[ct][3] = u1[0]; av[ct + 1][3] = u1[1];
                    }
                    if (NCT & 1) {
                        constexpr int ct = NCT - 1;
                        const float* e = ar[ks & 1][ct];
                        float u0, u1;
                        if (NR == 2) { u0 = e[0]; u1 = e[1]; }
                        else if (Q == 1) { u0 = e[0] + e[2]; u1 = e[1] + e[3]; }
                        else { u0 = e[0] - e[2]; u1 = e[1] - e[3]; }
                        av[ct][0] = u0; av[ct][1] = u0 + u1; av[ct][2] = u0 - u1; av[ct][3] = u1;
                    }
#pragma unroll
                    for (int g = 0; g < 12; ++g) {         // g = 4 kx + xi_y
                        const int slot = ks * 12 + g;
                        if (ks < 3 && g >= 4 && g < 4 + 2 * NCT && ((g - 4) & 1) == 0) {   // raw dY of the next k-step: one co tile per group
                            const int ct = (g - 4) >> 1;
#pragma unroll
                            for (int r = 0; r < NR; ++r) ar[(ks + 1) & 1][ct][r] = dyst[abase + ct * (4 * DYG) + (R0 + r) * 64 + 4 * (ks + 1)];
                        }
                        if (slot + 2 < 48) {
                            const int gn = (g + 2) % 12, ksn = ks + (g + 2) / 12;
                            bv[(slot + 2) % 3] = vst[bbase + (gn & 3) * XIS + 4 * ksn + (gn >> 2)];
                        }
                        if (slot < 48 - NDEF) {
#pragma unroll
                            for (int ct = 0; ct < NCT; ++ct)
                                acc[ct][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ct][g & 3], bv[slot % 3], acc[ct][g], 0, 0, 0);
                        } else {
                            pbv[slot - (48 - NDEF)] = bv[slot % 3];
                            if (slot == 47) {
#pragma unroll
                                for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                                    for (int y = 0; y < 4; ++y) pav[ct][y] = av[ct][y];
                            }
                        }
                        ride(slot);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                pending = true;
            };

            // ---- pipeline.  Box j (counted from box_lo) uses dY stage j % NDY and V stage j % 2.  While box j is multiplied,
            // box j + 2 is fetched (dY stage (j + 2) % NDY, raw planes into the ring) and box j + 1 transformed (ring -> V stage
            // (j + 1) % 2); in front of the barrier this box's fetch instructions -- issued at its start, ~7,000 cycles earlier --
            // are waited for.
#pragma unroll
            for (int piece = 0; piece < NFP; ++piece) fetch_piece(IS_FETCHER, 0, piece);
            fetch_done(true);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            transform_begin(IS_FETCHER);
#pragma unroll
            for (int piece = 0; piece < 8; ++piece) transform_piece(IS_FETCHER, NDY * DYF, piece);
            if (nbox > 1) {
#pragma unroll
                for (int piece = 0; piece < NFP; ++piece) fetch_piece(IS_FETCHER, DYF, piece);
                fetch_done(true);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();

            int dy_cur = 0, dy_ld = 2 * DYF;            // dY stage of box j / of box j + 2
            for (int j = 0; j < nbox; ++j) {
                const bool has1 = (j + 1) < nbox, has3 = (j + 2) < nbox;      // (has3: a box to fetch)
                const int v_cur = NDY * DYF + (j & 1) * XF, v_nx = NDY * DYF + ((j + 1) & 1) * XF;
                if (has1) transform_begin(IS_FETCHER);        // (box j + 1: its fetch was waited for at the previous barrier)
                compute_box(dy_cur, v_cur, [&](int slot) {
                    if (has3 && slot >= FSLOT0 && slot < FSLOT0 + 2 * NFP && (slot - FSLOT0) % 2 == 0) fetch_piece(IS_FETCHER, dy_ld, (slot - FSLOT0) / 2);
                    if (has1 && slot >= TSLOT0 && slot < TSLOT0 + TSTEP * 8 && (slot - TSLOT0) % TSTEP == 0) transform_piece(IS_FETCHER, v_nx, (slot - TSLOT0) / TSTEP);
                });
                dy_cur = dy_cur + DYF == NDY * DYF ? 0 : dy_cur + DYF;
                dy_ld = dy_ld + DYF == NDY * DYF ? 0 : dy_ld + DYF;
                if (has1) {
                    if (has3) fetch_done(true);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __syncthreads();
                }
            }
            if (pending) {
#pragma unroll
                for (int d = 0; d < NDEF; ++d)
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct)
                        acc[ct][12 - NDEF + d] = __builtin_amdgcn_mfma_f32_16x16x4f32(pav[ct][(12 - NDEF + d) & 3], pbv[d], acc[ct][12 - NDEF + d], 0, 0, 0);
            }
#pragma unroll
            for (int ct = 0; ct < 3; ++ct)
#pragma unroll
                for (int g = 0; g < 12; ++g) fin[ct][g] = ct < NCT ? acc[ct < NCT ? ct : 0][g] : f32x4{0.f, 0.f, 0.f, 0.f};
        };
        switch (wave) {
            case 0: run(std::integral_constant<int, 0>{}); break;
            case 1: run(std::integral_constant<int, 1>{}); break;
            case 2: run(std::integral_constant<int, 2>{}); break;
            case 3: run(std::integral_constant<int, 3>{}); break;
            case 4: run(std::integral_constant<int, 4>{}); break;
            case 5: run(std::integral_constant<int, 5>{}); break;
            case 6: run(std::integral_constant<int, 6>{}); break;
            default: run(std::integral_constant<int, 7>{}); break;
        }
    } else {
#pragma unroll
        for (int ct = 0; ct < 3; ++ct)
#pragma unroll
            for (int g = 0; g < 12; ++g) fin[ct][g] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    // ---- epilogue: dg = G^T P G.  y direction inside the wave, z direction across the four xi_z waves that hold a co tile, through
    // LDS (one co tile at a time: [q][36][64 lanes]); wave q == ct of the owning half finishes co tile ct.
    __syncthreads();
    {
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            const bool owner = ct == 0 ? cohalf == 0 : cohalf == 1;
            if (owner) {
                float* mine = lds + (q * 36) * 64 + lane;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int lc = ct == 0 ? 0 : ct - 1;
                        const float p0 = fin[lc][4 * kx + 0][r], p1 = fin[lc][4 * kx + 1][r], p2 = fin[lc][4 * kx + 2][r],
                                    p3 = fin[lc][4 * kx + 3][r];
                        const float h = 0.5f * (p1 + p2);
                        mine[((kx * 3 + 0) * 4 + r) * 64] = p0 + h;
                        mine[((kx * 3 + 1) * 4 + r) * 64] = 0.5f * (p1 - p2);
                        mine[((kx * 3 + 2) * 4 + r) * 64] = h - p3;          // (xi_y = 3 was accumulated with the opposite sign)
                    }
            }
            __syncthreads();
            if (owner && q == ct) {
                const int ci = ci0 + i;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int co = co0 + ct * 16 + 4 * k + r;
                    if (ci < a.Cin && co < a.Cout) {
                        float* o = a.slabs + (((size_t)sp * a.Cout + co) * a.Cin + ci) * 27;
#pragma unroll
                        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                            for (int ky = 0; ky < 3; ++ky) {
                                const int e = ((kx * 3 + ky) * 4 + r) * 64 + lane;
                                const float u0 = lds[e], u1 = lds[36 * 64 + e], u2 = lds[2 * 36 * 64 + e], u3 = lds[3 * 36 * 64 + e];
                                const float h = 0.5f * (u1 + u2);
                                o[0 * 9 + ky * 3 + kx] = u0 + h;
                                o[1 * 9 + ky * 3 + kx] = 0.5f * (u1 - u2);
                                o[2 * 9 + ky * 3 + kx] = h - u3;       // (xi_z = 3 was accumulated with the opposite sign)
                            }
                    }
                }
            }
            __syncthreads();
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Table rows: a block walks a contiguous range of cdiv(nboxes, split) boxes
template <bool LAZY>
static WgradRow wgrad_wzy_row() {
    return {{DRAM_K3_WGRAD_WZY, "conv3d_k3_wgrad_wzy_kernel", 0, {}, LAZY}, [](WgradArgs& a, hipStream_t st) {
                return launch_kernel<conv3d_k3_wgrad_wzy_kernel<LAZY>, WgradWzyGeom::LDS_BYTES, 512>("conv3d_k3_wgrad(wzy)", wgrad_grid(a), st, a,
                                                                                                  cdiv(a.nboxes, a.split));
            }};
}
static const WgradRow kWgradWzyRowList[] = {wgrad_wzy_row<false>(), wgrad_wzy_row<true>()};
const KernelTable<WgradArgs> kWgradWzyRows = kernel_table(kWgradWzyRowList);

}  // namespace dram
