"""Cases, inputs, a float64 restatement and rounding bounds for the seven 1x1x1 conv kernels of csrc/head.hip
(conv1x1_fwd_kernel<false / true>, conv1x1_dgrad_kernel<false / true>, conv1x1_wgrad_kernel, conv1x1_wgrad_vec_kernel,
conv1x1_wgrad_multi_kernel; sum_partials_kernel closes every backward-weights launch).  Host only: numpy.

Shared by tests/test_k1_cases_cpu.py (the restatement against oracle autograd, the exactness precondition, every case's
kernel label against the library's own answer, the coverage claims) and tests/test_gpu_k1_kernels.py.

Two kinds of inputs per case:
  * exact: integer-valued float32 x, w, bias, dy (and, for a lazy case, integer {a, b} rows), small enough that every partial
    sum any kernel can form stays below 2^24 in magnitude -- asserted from the fp64 sums of absolute values, which bound every
    partial sum whatever the order.  Every fp32 operation is then exact and the device result must equal the fp64 reference
    BIT FOR BIT: a wrong tail, a dropped or doubled channel, a wrong pass, a mis-indexed partial has no tolerance to hide in;
  * real: standard normal inputs, compared within  |got - ref| <= k * 2^-24 * sum |terms|  per element, k the number of
    fp32 roundings on the longest path a term takes through that kernel (below, read from the kernel).

Which kernel a case reaches is not restated here: the label is compared with dram_conv3d_k1_fwd_choice /
dram_conv3d_k1_bwd_choice, the rule the launches themselves go through."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

# ------------------------------------------------------------------------------------------------ the kernels' constants
K1_MAXCO = 8                    # csrc/common.h: output channels per pass of the forward and backward-data kernels
THREADS = 256
WG_VPT = 8                      # csrc/head.hip: voxels per thread of the scalar and the one-output backward-weights kernels
WG_VPB = THREADS * WG_VPT       # 2048 voxels per block; dram_conv3d_k1_bwd_ws_bytes is sized for it
WG_CT = 16                      # input channels per tile of conv1x1_wgrad_vec_kernel
WM_CO, WM_CT = 8, 8             # output / input channels per block of conv1x1_wgrad_multi_kernel
WM_VPB = 8192                   # its voxels per block
WM_ROUND = 4 * THREADS          # ... walked in rounds of one float4 per thread
U = 2.0 ** -24                  # unit roundoff of float32
EXACT_LIMIT = 2 ** 24

FWD_KERNELS = ("conv1x1_fwd_kernel<false>", "conv1x1_fwd_kernel<true>")                    # dram_conv3d_k1_fwd_choice
BWD_KERNELS = ("conv1x1_dgrad_kernel<false>", "conv1x1_dgrad_kernel<true>", "conv1x1_wgrad_kernel",
               "conv1x1_wgrad_vec_kernel", "conv1x1_wgrad_multi_kernel")                    # dram_conv3d_k1_bwd_choice
DGRAD_KERNELS, WGRAD_KERNELS = BWD_KERNELS[:2], BWD_KERNELS[2:]
KERNELS = FWD_KERNELS + BWD_KERNELS


def cdiv(a, b):
    return -(-a // b)


def passes(Cout):
    return cdiv(Cout, K1_MAXCO)


# ------------------------------------------------------------------------------------------------ k: fp32 roundings per term
# Each rounding is of relative size <= U of a partial sum that is itself <= sum |terms|, so a term that passes through k
# roundings gives |got - exact| <= ((1 + U)^k - 1) * sum |terms| = k U sum |terms| to first order (the remainder is below
# k^2 U / 2 < 1e-4 of ONE of those k units for every k here).  A fused multiply-add rounds once.
#
# conv1x1_fwd_kernel: acc = bias (loaded, exact), then ONE chain of Cin fmaf over the input channels; the passes split the
#   OUTPUT channels, so the chain is Cin long whatever Cout is.  Cin roundings, and one unit spare for the remainder.
def k_fwd(Cin):
    return Cin + 1


# conv1x1_dgrad_kernel: per pass r = 0, then nco <= MAXCO fmaf (the first rounds its product); every pass after the first adds
#   the dx it finds: one more rounding for everything summed so far.  The longest path is a term of pass 0:
#   min(Cout, MAXCO) + (passes - 1) roundings, and one unit spare.  (Fewer than the Cout + passes of a single chain.)
def k_dgrad(Cout):
    return min(Cout, K1_MAXCO) + (passes(Cout) - 1) + 1


# Backward-weights: a block's partial sum in fp32, the partials of a result added in fp64 in a fixed order (sum_partials_kernel:
#   2^-53 each, nothing next to U) and rounded to fp32 once.
#   conv1x1_wgrad_kernel (scalar): s = 0, WG_VPT = 8 fmaf per thread; block_sum_256 = 6 butterfly levels over 64 lanes, then
#     red[0] + red[1] + red[2] + red[3] LEFT TO RIGHT: a term of wave 0 goes through 3 additions; the final cast.  8 + 6 + 3 + 1.
#     (The bias column: 7 additions per thread, the first being 0 + g, then the same 6 + 3 + 1: shorter.)
#   conv1x1_wgrad_vec_kernel: g0.x * a.x and 7 fmaf = 8 per thread; wave_sum 6; (red[0] + red[1]) + (red[2] + red[3]): 2; cast.
#     8 + 6 + 2 + 1.  (Bias column: a tree of depth 3 over the thread's 8 values, then 6 + 2 + 1.)
#   conv1x1_wgrad_multi_kernel: acc = 0, then 4 fmaf per round over WM_VPB / WM_ROUND = 8 rounds = 32 per thread; wave_sum 6;
#     (red[0] + red[1]) + (red[2] + red[3]): 2; cast.  32 + 6 + 2 + 1.  (Bias column: 2 + 7 per thread, then 6 + 2 + 1.)
K_WGRAD = {
    "conv1x1_wgrad_kernel": WG_VPT + 6 + 3 + 1,
    "conv1x1_wgrad_vec_kernel": WG_VPT + 6 + 2 + 1,
    "conv1x1_wgrad_multi_kernel": 4 * (WM_VPB // WM_ROUND) + 6 + 2 + 1,
}
assert K_WGRAD == {"conv1x1_wgrad_kernel": 18, "conv1x1_wgrad_vec_kernel": 17, "conv1x1_wgrad_multi_kernel": 41}


def bound(k, sum_abs):
    """Elementwise bound on |got - ref|; sum_abs the fp64 sum of |terms| of each element."""
    return k * U * sum_abs


# ------------------------------------------------------------------------------------------------ the cases
# op "fwd": x_shift / out_shift are the bytes x / y sit off a 16-byte boundary.  op "bwd": x_shift, out_shift (dx), dy_shift;
# every backward case asks for dx, dw and dbias in one call, `kernel` is the kernel the case was built for, the other one of
# the call is asked of the library.  lazy: 0 = the plain entry; 1 = the _lazy entry with a coefficient row per (n, c), ReLU on.
Case = namedtuple("Case", "id op N Cin Cout S x_shift out_shift dy_shift bias lazy kernel")


def _fwd(cid, N, Cin, Cout, S, kernel, x=0, y=0, bias=True, lazy=0):
    return Case(cid, "fwd", N, Cin, Cout, S, x, y, 0, bias, lazy, kernel)


def _bwd(cid, N, Cin, Cout, S, kernel, x=0, dx=0, dy=0, lazy=0):
    return Case(cid, "bwd", N, Cin, Cout, S, x, dx, dy, True, lazy, kernel)


FS, FV = FWD_KERNELS
DS, DV, WS, WV, WM = BWD_KERNELS

_FWD = [
    # 693 = 2 * 256 + 181: three blocks of the scalar kernel, the last with 181 threads; 11 outputs = a pass of 8 and one of 3
    _fwd("f_scalar_co11", 2, 5, 11, 693, FS),
    # 1028 = 257 float4: rows of whole 16-byte pieces, scalar only because y (resp. x) is 4 bytes off; 9 outputs = 8 + 1
    _fwd("f_scalar_y_off", 1, 4, 9, 1028, FS, y=4),
    _fwd("f_scalar_x_off", 1, 4, 2, 1028, FS, x=4),
    # the float4 kernel: a second block with ONE live thread; 17 outputs = 8 + 8 + 1: a third pass
    _fwd("f_vec_co17", 2, 3, 17, 1028, FV),
    # exactly one and exactly two full passes: no tail pass
    _fwd("f_scalar_co8", 1, 5, 8, 693, FS),
    _fwd("f_vec_co16", 1, 3, 16, 1028, FV),
    _fwd("f_vec_nobias", 2, 6, 3, 1028, FV, bias=False),
    _fwd("f_scalar_nobias", 1, 6, 10, 257, FS, bias=False),
    _fwd("f_vec_tiny", 3, 1, 1, 4, FV),                       # one input channel, one thread per sample
    # the lazy entry (normalise + ReLU on load) through both kernels, two passes
    _fwd("f_vec_lazy", 2, 5, 11, 1028, FV, lazy=1),
    _fwd("f_scalar_lazy", 2, 5, 11, 693, FS, lazy=1),
]

_DGRAD = [
    # dx is NaN before every call: pass 0 must overwrite, the later passes must add (`accumulate = co0 > 0`)
    _bwd("d_scalar_co11", 2, 5, 11, 693, DS),                 # scalar read-modify-write of pass 1 (3 outputs)
    _bwd("d_vec_co17", 2, 3, 17, 1028, DV),                   # float4 read-modify-write of passes 1 and 2
    _bwd("d_scalar_dx_off", 1, 4, 9, 1028, DS, dx=4),         # scalar only because dx is 4 bytes off (dy and x aligned)
    _bwd("d_vec_co8", 2, 5, 8, 1028, DV),                     # exactly one pass: nothing accumulates
    _bwd("d_vec_co16", 1, 3, 16, 1028, DV),                   # exactly two
]

# conv1x1_wgrad_vec_kernel (Cout = 1): channel tiles of WG_CT = 16 x voxel blocks of 2048, two float4 per thread (e0 = 4 tid,
# e1 = 1024 + 4 tid)
_VEC_CIN = (7, 16, 17, 40)            # a tail alone; exactly one tile; two tiles, tail 1; three tiles, tail 8
_VEC_S = (4, 1028, 2052)              # one thread; one block where thread 0 alone holds a second float4; two blocks, the
#                                       second with one live thread
_WVEC = [_bwd(f"wv_ci{ci}_s{s}", 2, ci, 1, s, WV) for ci in _VEC_CIN for s in _VEC_S]

# conv1x1_wgrad_multi_kernel: tiles of 8 x 8 channels in blockIdx.z, blocks of 8192 voxels in rounds of 1024
_MULTI_CH = ((1, 2), (8, 8), (9, 9), (20, 17))   # the smallest Cout that selects it; exact tiles; 2 x 2 tiles with tails of
#                                                  1; 3 x 3 tiles with tails 4 and 1
_MULTI_S = (4, 3080, 8196)            # one thread; three full rounds and a round of two threads; two blocks, the second with
#                                       one float4
_WMULTI = [_bwd(f"wm_ci{ci}_co{co}_s{s}", 2, ci, co, s, WM) for ci, co in _MULTI_CH for s in _MULTI_S]
_WMULTI.append(_bwd("wm_ci9_co9_s3080_lazy", 2, 9, 9, 3080, WM, lazy=1))

_WSCALAR = [
    _bwd("ws_co3_s4099", 2, 7, 3, 4099, WS),                  # S % 4 != 0; three blocks, the last with 3 voxels
    _bwd("ws_co9_dy_off", 2, 9, 9, 2052, WS, dy=4),           # S % 4 == 0: scalar because dy is 4 bytes off ...
    _bwd("ws_co9_x_off", 2, 9, 9, 2052, WS, x=4),             # ... because x is
]

_WLAZY = [
    _bwd("ws_co1_lazy", 2, 7, 1, 4099, WS, lazy=1),
    _bwd("wv_ci17_s2052_lazy", 2, 17, 1, 2052, WV, lazy=1),   # (the tail-channel clamp also picks the coefficient row)
]

CASES = _FWD + _DGRAD + _WVEC + _WMULTI + _WSCALAR + _WLAZY
IDS = [c.id for c in CASES]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
FWD_CASES = [c for c in CASES if c.op == "fwd"]
BWD_CASES = [c for c in CASES if c.op == "bwd"]


def library_kernels(case):
    """The kernels the library says the case's call launches: (forward,) or (backward-data, backward-weights)."""
    from dram_amd import _lib
    mis = lambda shift: int(shift % 16 != 0)
    if case.op == "fwd":
        rc = _lib.lib.dram_conv3d_k1_fwd_choice(mis(case.x_shift), mis(case.out_shift), case.S)
        assert rc >= 0, _lib.lib.dram_last_error()
        return (FWD_KERNELS[rc],)
    out = []
    for which in (0, 1):
        rc = _lib.lib.dram_conv3d_k1_bwd_choice(mis(case.dy_shift), mis(case.x_shift), mis(case.out_shift), case.Cin, case.Cout,
                                                case.S, which)
        assert rc >= 0, _lib.lib.dram_last_error()
        out.append(BWD_KERNELS[rc])
    assert out[0] in DGRAD_KERNELS and out[1] in WGRAD_KERNELS
    return tuple(out)


def multi_rounds(S):
    """conv1x1_wgrad_multi_kernel on a row of S voxels: per block (full rounds of 256 float4, threads in the ragged round)."""
    out = []
    for b in range(cdiv(S, WM_VPB)):
        n = min(WM_VPB, S - b * WM_VPB)
        out.append((n // WM_ROUND, (n % WM_ROUND) // 4))
    return out


def partial_floats(case, kernel):
    """Floats of the workspace that the backward-weights kernel of a call writes."""
    vpb = WM_VPB if kernel == WM else WG_VPB
    return case.N * cdiv(case.S, vpb) * case.Cout * (case.Cin + 1)


def ws_floats(case):
    """dram_conv3d_k1_bwd_ws_bytes / 4: sized for WG_VPB whatever kernel runs."""
    return case.N * cdiv(case.S, WG_VPB) * case.Cout * (case.Cin + 1)


# ------------------------------------------------------------------------------------------------ inputs
Inputs = namedtuple("Inputs", "x w bias dy coef")     # float32 numpy: x [N, Cin, S] (RAW for a lazy case), w [Cout, Cin],
#                                                       bias [Cout] or None, dy [N, Cout, S], coef [N * Cin, 2] or None


def _seed(case, kind):
    return [IDS.index(case.id), {"exact": 1, "real": 2}[kind]]


def activated(x, coef, relu=True):
    """The operand a lazy tensor stands for, in the dtype of x: max(a * x + b, relu ? 0 : -inf) per (n, c) row."""
    if coef is None:
        return x
    N, Cin, S = x.shape
    a = coef[:, 0].reshape(N, Cin, 1).astype(x.dtype)
    b = coef[:, 1].reshape(N, Cin, 1).astype(x.dtype)
    v = a * x + b
    return np.maximum(v, 0) if relu else v


@lru_cache(maxsize=None)
def exact_inputs(cid):
    """Integer-valued inputs; asserts the exactness precondition."""
    c = BY_ID[cid]
    rng = np.random.default_rng(_seed(c, "exact"))
    ints = lambda lo, hi, shape: rng.integers(lo, hi + 1, shape).astype(np.float32)
    x = ints(-4, 4, (c.N, c.Cin, c.S))
    w = ints(-3, 3, (c.Cout, c.Cin))
    bias = ints(-5, 5, (c.Cout,)) if c.bias else None
    dy = ints(-4, 4, (c.N, c.Cout, c.S))
    coef = None
    if c.lazy:      # a in -2..2 with at least one 0 and one negative row, b in -3..3: act(a * x + b) is an integer <= 11
        coef = np.stack([ints(-2, 2, (c.N * c.Cin,)), ints(-3, 3, (c.N * c.Cin,))], 1)
        coef[0], coef[1] = (0.0, 2.0), (-2.0, 1.0)
    inp = _freeze(Inputs(x, w, bias, dy, coef))
    assert exactness_margin(c, inp) < EXACT_LIMIT, cid
    return inp


@lru_cache(maxsize=None)
def real_inputs(cid):
    """Standard normal inputs.  A lazy case has no coef here: the GPU test materialises the operand on the device
    (dram_row_affine_act) and hands it in as x, so the reference sees the very float32 values the kernels consume."""
    c = BY_ID[cid]
    rng = np.random.default_rng(_seed(c, "real"))
    rn = lambda shape: rng.standard_normal(shape, dtype=np.float32)
    return _freeze(Inputs(rn((c.N, c.Cin, c.S)), rn((c.Cout, c.Cin)), rn((c.Cout,)) if c.bias else None,
                          rn((c.N, c.Cout, c.S)), None))


def _freeze(inp):
    for a in inp:
        if a is not None:
            a.setflags(write=False)
    return inp


# ------------------------------------------------------------------------------------------------ the restatement
def restate(x, w, bias, dy):
    """y = W x + b, dx = W^T dy, dw = sum_{n,s} dy x, db = sum_{n,s} dy in float64, and the sums of |terms| of each element.
    x is the operand itself (an activated one for a lazy case).  dy is None for a forward case."""
    x, w = x.astype(np.float64), w.astype(np.float64)
    out = {"y": np.einsum("oc,ncs->nos", w, x), "y_abs": np.einsum("oc,ncs->nos", np.abs(w), np.abs(x))}
    if bias is not None:
        b = bias.astype(np.float64)[None, :, None]
        out["y"], out["y_abs"] = out["y"] + b, out["y_abs"] + np.abs(b)
    if dy is not None:
        dy = dy.astype(np.float64)
        out["dx"], out["dx_abs"] = np.einsum("oc,nos->ncs", w, dy), np.einsum("oc,nos->ncs", np.abs(w), np.abs(dy))
        out["dw"], out["dw_abs"] = np.einsum("nos,ncs->oc", dy, x), np.einsum("nos,ncs->oc", np.abs(dy), np.abs(x))
        out["db"], out["db_abs"] = dy.sum((0, 2)), np.abs(dy).sum((0, 2))
    return out


def reference(case, inp):
    """restate() on the case's operand: act(coef * x) for a lazy case with coefficients."""
    return restate(activated(inp.x, inp.coef), inp.w, inp.bias, inp.dy if case.op == "bwd" else None)


def exactness_margin(case, inp):
    """The largest sum of |terms| over every output element of the case: no partial sum of any route exceeds it."""
    ref = reference(case, inp)
    return max(float(ref[k].max()) for k in ref if k.endswith("_abs"))


@lru_cache(maxsize=None)
def exact_reference(cid):
    """reference() of the exact inputs, computed once and shared; nobody writes to it."""
    ref = reference(BY_ID[cid], exact_inputs(cid))
    for v in ref.values():
        v.setflags(write=False)
    return ref
