// What the translation units of the 3x3x3 convolution (conv3d_k3.hip, conv3d_k3_wgrad_wzy.hip) share on the host side: the kernel argument structs, the
// table rows that name and launch one kernel instantiation each, and the one launcher / grid check they all use.
#pragma once
#include "common.h"
#include <initializer_list>

namespace dram {

// channels [0,C1) live in p1 (spatial D,H,W); channels [C1,C1+C2) in p2 (spatial
// D2,H2,W2) seen through a crop window starting at (oz,oy,ox).
struct CatView {
    float* p1;
    float* p2;
    int C1, C2;
    int D2, H2, W2;
    int oz, oy, ox;
};

// a source or destination as the C ABI passes it (without a second tensor its extents and window are neutral)
inline CatView cat_view(const float* p1, int C1, const float* p2, int C2, int D2, int H2, int W2, int oz, int oy, int ox) {
    return CatView{const_cast<float*>(p1), const_cast<float*>(p2), C1, p2 ? C2 : 0, p2 ? D2 : 1, p2 ? H2 : 1,
                   p2 ? W2 : 1, p2 ? oz : 0, p2 ? oy : 0, p2 ? ox : 0};
}

struct ConvArgs {
    CatView src;
    CatView dst;
    const float* wt;    // [27][Cin][Cout]
    const float* bias;  // [Cout] or null
    int N, Cin, Cout, D, H, W;
    int nbx, nby, nbz, co_tiles;
    // "normalise + ReLU on load": source tensor k is the RAW output y of the producing conv and the operand of
    // this conv is act_k(coefk[row][0] * y + coefk[row][1]) per (n, c) row, ReLU if reluk (coefk null: the tensor
    // is used as it is).  The activated tensor of the norm -> ReLU between two convs is then never written.
    const float* coef1;
    const float* coef2;
    int relu1, relu2;
    // BatchNorm / GroupNorm statistics of the OUTPUT in the epilogue: per (row, box, wave) {mean, M2, count} of the
    // wave's 64 outputs of that channel -> stats[(row * nparts + part) * 3]; null: not wanted.
    float* stats;
    int nparts;
    // division by co_tiles / nbx / nby / nbz as a multiply + shift (the persistent (z,y) kernel decodes three item cursors per
    // item: 17 runtime integer divisions, each a v_rcp_iflag sequence with a VALU -> SALU round trip, ~2,000 cycles per item).
    // One 48-byte record {divisor, multiplier, shift} x 4, so that a decode reads it with three wide scalar loads.
    alignas(16) unsigned dv_d[4];
    alignas(16) unsigned dv_m[4];
    alignas(16) unsigned dv_s[4];
};

// x / d for x < 2^31 by a host-prepared multiply + shift (Granlund-Montgomery, branch-free): l = ceil(log2 d),
// m = floor(2^32 (2^l - d) / d) + 1, x / d = (mulhi(x, m) + x) >> l (d == 1: l = 0, m = 1: mulhi = 0).
static inline void fast_div_prepare(unsigned d, unsigned& m, unsigned& sh) {
    if (d == 0) d = 1;
    unsigned l = 0;
    while ((1ull << l) < d) ++l;
    m = (unsigned)(((((unsigned long long)1 << l) - d) << 32) / d + 1);
    sh = l;
}

struct WgradArgs {
    CatView src;      // x (possibly a virtual concatenation)
    const float* dy;  // [N][Cout][D][H][W]
    float* slabs;     // [SPLIT][Cout][Cin][27]
    int N, Cin, Cout, D, H, W;
    int nbx, nby, nbz, nboxes, split, ci_tiles, co_tiles;
    int ci_tile0;     // first 16-channel ci tile of this launch ((z,y) kernel: a launch may cover the tiles of ONE source only)
    // normalise + ReLU on load of x (see ConvArgs::coef1): source k holds the RAW conv output, the operand is
    // act(coefk[row][0] * x + coefk[row][1]); Winograd kernel only (the host materialises for the others)
    const float* coef1;
    const float* coef2;
    int relu1, relu2;
};

struct WgradC1Args {
    const float* x;   // [N][1][D][H][W]
    const float* dy;  // [N][Cout][D][H][W]
    float* slabs;     // [4*gridDim.x][Cout][27]
    int N, Cout, D, H, W;
    int nbx, nby, nbz, nboxes;
};

// ---------------------------------------------------------------------------------------------
// One row per kernel instantiation of the library.  A row is written once, next to the kernel, by an expression in
// which the template arguments appear once: it fills `targ` / `flag` and instantiates `launch` from the same
// arguments, so the name a choice query reports (kernel_name) is the instantiation a launch takes.
struct KernelId {
    int kind;           // DRAM_K3_*
    const char* base;   // the kernel's name as rocprofv3 prints it, without namespace, template and argument list
    int nprint;         // leading entries of targ that are template arguments (the rest only tells rows apart)
    int targ[5];        // box / tile shape of the instantiation
    int flag;           // trailing bool template argument (FUSED / LAZY); -1: the kernel has none
};
template <typename Args>
struct KernelRow {
    KernelId id;
    int (*launch)(Args&, hipStream_t);
};
template <typename Args>
struct KernelTable {
    const KernelRow<Args>* rows;
    int n;
    // the row whose shape starts with `targ` and whose flag is `flag`; null: the library has no such instantiation
    const KernelRow<Args>* find(std::initializer_list<int> targ, int flag = -1) const {
        for (int r = 0; r < n; ++r) {
            bool same = rows[r].id.flag == flag;
            int i = 0;
            for (const int t : targ) same = same && rows[r].id.targ[i++] == t;
            if (same) return &rows[r];
        }
        return nullptr;
    }
};
template <typename Args, int N>
constexpr KernelTable<Args> kernel_table(const KernelRow<Args> (&rows)[N]) {
    return KernelTable<Args>{rows, N};
}
typedef KernelRow<ConvArgs> FwdRow;
typedef KernelRow<WgradArgs> WgradRow;

// "base<1, 2, true>" as rocprofv3 spells an instantiation (a kernel that is no template: the base name alone)
inline void kernel_name(const KernelId& k, char* name, size_t cap) {
    if (!name || !cap) return;
    char buf[128];
    int n = snprintf(buf, sizeof(buf), "%s", k.base);
    const char* sep = "<";
    for (int i = 0; i < k.nprint; ++i, sep = ", ") n += snprintf(buf + n, sizeof(buf) - n, "%s%d", sep, k.targ[i]);
    if (k.flag >= 0) n += snprintf(buf + n, sizeof(buf) - n, "%s%s", sep, k.flag ? "true" : "false");
    if (k.nprint > 0 || k.flag >= 0) snprintf(buf + n, sizeof(buf) - n, ">");
    snprintf(name, cap, "%s", buf);
}

// the (z,y) backward-weights kernel's rows (conv3d_k3_wgrad_wzy.hip); every other table is in conv3d_k3.hip
extern const KernelTable<WgradArgs> kWgradWzyRows;

// ---------------------------------------------------------------------------------------------
// The one launcher: opt in to the kernel's dynamic LDS once per device (the flag is a static of this instantiation,
// i.e. per kernel), launch, report a launch error under `label`.
template <auto KERN, size_t LDS_BYTES, int BLOCK, typename... A>
static int launch_kernel(const char* label, dim3 grid, hipStream_t st, const A&... args) {
    if (LDS_BYTES > 0) {
        static LdsAttrOnce lds_once;
        if (const int rc = ensure_dynamic_lds((const void*)KERN, LDS_BYTES, lds_once, label)) return rc;
    }
    hipLaunchKernelGGL(KERN, grid, dim3(BLOCK), LDS_BYTES, st, args...);
    return check_launch(label);
}

// Forward launches: boxes per sample for a bx x by x bz box, channel tiles of `cob` channels, and the number of work
// items = blocks of a non-persistent kernel (the one grid-size check).
inline int conv_fwd_items(ConvArgs& a, int bx, int by, int bz, int cob, unsigned& items) {
    a.nbx = cdiv(a.W, bx);
    a.nby = cdiv(a.H, by);
    a.nbz = cdiv(a.D, bz);
    a.co_tiles = cdiv(a.Cout, cob);
    int64_t total = (int64_t)a.N * a.nbx * a.nby * a.nbz;
    if (total <= 0x7fffffffLL) total *= a.co_tiles;
    if (total > 0x7fffffffLL) {
        set_error("conv3d_k3_fwd: grid too large");
        return DRAM_EINVAL;
    }
    items = (unsigned)total;
    return DRAM_OK;
}
// Backward-weights launches: one block per (split, co tile, ci tile)
inline dim3 wgrad_grid(const WgradArgs& a) { return dim3((unsigned)(a.split * a.ci_tiles * a.co_tiles)); }

}  // namespace dram
