"""The fused engine's normalise-on-load kernels, each through the C ABI on its own.

A fused 3x3x3 conv leaves its RAW output and per-part moments; dram_norm_finalize_parts turns the moments into per-row
{a, b}; every consumer applies max(a*y + b, relu ? 0 : -inf) while it loads (include/dram_hip.h, "Lazy" tensors).  Here
  * every on-load consumer other than the 3x3x3 convs (those: tests/test_gpu_parity.py) is compared bit for bit
    (torch.equal) with the plain entry point on the materialised operand xa = dram_row_affine_act(raw, coef, relu) -- the
    header's promise -- and against an fp64 evaluation of op(act(a * raw + b)) at the plain op's own tolerance;
  * dram_row_affine_act itself, dram_norm_finalize_parts and dram_bn_parts_stats are compared with fp64;
  * the norm backward recomputes its ReLU mask from {a, b}: it is run with gamma of either sign and an exact zero.
The coefficient tables (tests/onload_reference.py coef_table) have rows with a < 0, a == 0, b of either sign and, under
ReLU, a row whose activated values are all 0.  Every output is filled with NaN before the call (an element that is not
written fails) and sits between guard words (a write outside the tensor fails).  There is no launch counter for these
kernels: the comment next to each shape says which kernel the host-side rule sends it to, and why.

Each test prints an `onload-accuracy:` line per case before it asserts (run with -s to see the figures)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import dram_oracle as O
from gpu_buffers import DEV, GUARD, NAN, Placed, call, g, lazy_operand, materialise, p, stream   # noqa: F401
from onload_reference import BATCH, GROUP, STAT_CASES, act64, make_parts, norm_reference, stat_case_data, stat_of_row
from test_gpu_parity import TOL, check, rel_err

pytestmark = pytest.mark.gpu


def report(line):
    print("onload-accuracy: " + line)


def ordered(t):
    """float32 -> int64 that is monotone in the value (both zeros at 0): differences count units in the last place."""
    i = t.contiguous().view(torch.int32).to(torch.int64)
    return torch.where(i >= 0, i, -(i & 0x7FFFFFFF))


# ------------------------------------------------------------------ dram_row_affine_act
# S, bytes off alignment, the kernel the launch takes (CHUNK = 4096 floats per block; vector kernel: S % 4 == 0 and both
# pointers 16-byte aligned, csrc/norm.hip vec_ok)
AFFINE_ROWS = [
    (12, 0, "row_affine_act_kernel<true>"),        # one thread holds all of the row
    (4096, 0, "row_affine_act_kernel<true>"),      # exactly one chunk
    (4100, 0, "row_affine_act_kernel<true>"),      # a second chunk of 4 elements: one 16-byte store
    (4097, 0, "row_affine_act_kernel<false>"),     # S % 4 != 0: scalar kernel, a second chunk of one element
    (693, 0, "row_affine_act_kernel<false>"),      # scalar kernel, one partial chunk
    (4100, 4, "row_affine_act_kernel<false>"),     # S % 4 == 0 but the pointers are 4 bytes off: scalar kernel
]


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("rows", [1, 37])
@pytest.mark.parametrize("S,shift,kernel", AFFINE_ROWS)
def test_row_affine_act(S, shift, kernel, rows, relu):
    """y = act(a*x + b) against float32(a64 * x64 + b64) clamped at 0 under ReLU.  fmaf rounds once, the fp64 path twice
    (53 bits, then 24): they differ, by one unit in the last place, only where the 53-bit sum lands on a float32 midpoint
    -- about 2^-29 per element.  Allowed: <= 1 ulp, in at most 1 element per 100 000.  The ReLU mask must be exact."""
    raw, coef, _ = lazy_operand((rows, 1, S), 100 + S, shift)
    y = Placed((rows, 1, S), shift)
    call("dram_row_affine_act", p(raw), p(coef), p(y.t), relu, rows, S)
    torch.cuda.synchronize()
    assert y.intact()
    got = y.t.cpu().view(rows, S)
    v64 = act64(raw.cpu().view(rows, S), coef.cpu(), 0)
    ref = (v64.clamp_min(0.0) if relu else v64).float()
    assert not bool(torch.isnan(got).any())
    dist = (ordered(got) - ordered(ref)).abs()
    off = int((dist > 0).sum())
    report(f"row_affine_act S={S} shift={shift} rows={rows} relu={relu} [{kernel}]: max {int(dist.max())} ulp, "
           f"{off} of {got.numel()} elements differ from float32(fp64)")
    assert int(dist.max()) <= 1
    assert off * 100000 <= got.numel()
    if relu:
        assert torch.equal(got == 0, v64 <= 0)


# ------------------------------------------------------------------ max-pool
POOL_SHAPES = [
    (2, 3, 6, 10, 12),      # 6 rows: every special row
    (1, 5, 7, 9, 11),       # odd sizes: the last plane / row / column is cropped
    (1, 2, 16, 16, 34),     # 8*8*17 = 1088 outputs per plane: five blocks, the last with 64 outputs
    (1, 1, 2, 2, 2),        # one window
]


def routed_index(idx_flat, shape):
    """ATen's flat input index per pooled cell -> dz*4 + dy*2 + dx inside the cell's window."""
    D, H, W = shape[2:]
    Do, Ho, Wo = D // 2, H // 2, W // 2
    z, y, x = idx_flat // (H * W), (idx_flat // W) % H, idx_flat % W
    zo = torch.arange(Do).view(1, 1, Do, 1, 1)
    yo = torch.arange(Ho).view(1, 1, 1, Ho, 1)
    xo = torch.arange(Wo).view(1, 1, 1, 1, Wo)
    local = (z - 2 * zo) * 4 + (y - 2 * yo) * 2 + (x - 2 * xo)
    assert bool(((z - 2 * zo) >> 1 == 0).all() and ((y - 2 * yo) >> 1 == 0).all() and ((x - 2 * xo) >> 1 == 0).all())
    return local.to(torch.uint8)


def pool_fwd(shape, relu, seed=200):
    """(raw, coef, special, xa, out, idx) of the lazy forward, checked against the plain entry on xa."""
    N, C, D, H, W = shape
    oshape = (N, C, D // 2, H // 2, W // 2)
    raw, coef, special = lazy_operand(shape, seed)
    xa = materialise(raw, coef, relu)
    res = {}
    for name in ("lazy", "plain"):
        out, idx = Placed(oshape), Placed(oshape, dtype=torch.uint8)
        if name == "lazy":     # maxpool2_fwd_kernel with coef
            call("dram_maxpool3d_2_fwd_lazy", p(raw), p(coef), relu, p(out.t), p(idx.t), N, C, D, H, W)
        else:
            call("dram_maxpool3d_2_fwd", p(xa), p(out.t), p(idx.t), N, C, D, H, W)
        torch.cuda.synchronize()
        assert out.intact() and idx.intact(), (shape, name)
        res[name] = (out.t, idx.t)
    assert torch.equal(res["lazy"][0], res["plain"][0]), shape
    assert torch.equal(res["lazy"][1], res["plain"][1]), shape
    return raw, coef, special, xa, res["lazy"][0], res["lazy"][1]


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_maxpool_fwd_lazy(shape, relu):
    """maxpool2_fwd_kernel with `coef`: values and routing of max_pool3d(act(a*raw + b)).  A kernel that compared raw values
    would route a < 0 rows to the raw maximum and rows that ReLU flattens to a raw position instead of the first zero."""
    N, C = shape[:2]
    raw, coef, special, xa, out, idx = pool_fwd(shape, relu)
    xa_c, out_c, idx_c = xa.cpu(), out.cpu(), idx.cpu()
    ref, ref_idx = F.max_pool3d(xa_c, 2, return_indices=True)
    assert torch.equal(out_c, ref)                                   # exact: the maximum of eight float32 values
    assert torch.equal(idx_c, routed_index(ref_idx, shape))          # ATen's first maximum in (z, y, x) scan order
    rows_out, rows_idx = out_c.flatten(0, 1), idx_c.flatten(0, 1)
    if "dead" in special and relu:
        assert bool((rows_out[special["dead"]] == 0).all()) and bool((rows_idx[special["dead"]] == 0).all())
    if "zero" in special:
        assert bool((rows_idx[special["zero"]] == 0).all())
        assert bool((rows_out[special["zero"]] == coef[special["zero"], 1].cpu()).all())
    # a < 0: the activation decreases with the raw value, so the pooled value is the activated raw MINIMUM of the window
    _, min_idx = F.max_pool3d(-raw.cpu(), 2, return_indices=True)
    at_min = xa_c.flatten(2).gather(2, min_idx.flatten(2)).view_as(out_c).flatten(0, 1)
    neg = (coef[:, 0] < 0).cpu()
    assert bool(neg[special["neg"]]) and torch.equal(rows_out[neg], at_min[neg])
    # and against fp64: pooling commutes with the (monotone) rounding to float32
    ref64 = F.max_pool3d(act64(raw.cpu().flatten(0, 1), coef.cpu(), relu).view(*shape), 2)
    dist = (ordered(out_c) - ordered(ref64.float())).abs()
    report(f"maxpool_fwd_lazy {shape} relu={relu} [maxpool2_fwd_kernel, coef]: equal to the plain entry on xa; "
           f"max {int(dist.max())} ulp from float32(fp64), {int((dist > 0).sum())} of {out_c.numel()} elements differ")
    assert int(dist.max()) <= 1 and int((dist > 0).sum()) * 100000 <= out_c.numel()


POOL_BWD_CASES = [
    # shape, bytes off alignment of dx, the kernel the launch takes (vector kernel: W % 4 == 0, dout 8-byte, idx 2-byte and dx
    # 16-byte aligned; csrc/resample.hip maxpool_bwd_run)
    ((2, 3, 6, 10, 12), 0, "maxpool2_bwd_vec_kernel"),
    ((1, 2, 7, 9, 12), 0, "maxpool2_bwd_vec_kernel"),     # ... with a cropped last plane and row: quads without a pooled cell
    ((1, 5, 7, 9, 11), 0, "maxpool2_bwd_kernel"),         # W = 11: scalar kernel, cropped plane / row / column
    ((2, 3, 6, 10, 12), 4, "maxpool2_bwd_kernel"),        # W = 12 but dx 4 bytes off: scalar kernel
]


@pytest.mark.parametrize("shape,shift,kernel", POOL_BWD_CASES)
def test_maxpool_bwd_acc(shape, shift, kernel):
    """dx += scatter(dout) with `accumulate`: exactly one gradient is added per window, so the result is dx0 + the plain
    backward bit for bit, and the positions beyond the floor-cropped extent keep dx0."""
    N, C, D, H, W = shape
    _, _, _, _, _, idx = pool_fwd(shape, 1, seed=230)
    dout = torch.randn(N, C, D // 2, H // 2, W // 2, generator=g(231)).to(DEV)
    dx0 = torch.randn(*shape, generator=g(232))
    plain = Placed(shape)
    call("dram_maxpool3d_2_bwd", p(dout), p(idx), p(plain.t), N, C, D, H, W)
    acc = Placed(shape, shift, src=dx0)
    call("dram_maxpool3d_2_bwd_acc", p(dout), p(idx), p(acc.t), N, C, D, H, W)
    torch.cuda.synchronize()
    assert plain.intact() and acc.intact()
    assert not bool(torch.isnan(plain.t).any())
    assert int((plain.t != 0).sum()) == int((dout != 0).sum())          # one routed gradient per window
    assert torch.equal(acc.t, dx0.to(DEV) + plain.t)
    got = acc.t.cpu()
    De, He, We = 2 * (D // 2), 2 * (H // 2), 2 * (W // 2)
    assert torch.equal(got[:, :, De:], dx0[:, :, De:]) and torch.equal(got[:, :, :, He:], dx0[:, :, :, He:])
    assert torch.equal(got[..., We:], dx0[..., We:])
    report(f"maxpool_bwd_acc {shape} dx shift={shift} [{kernel}, accumulate]: equal to dx0 + plain backward")


# ------------------------------------------------------------------ trilinear, align_corners=True
# Which of the three kernels tri_fwd_launch (csrc/resample.hip) takes; scale = (in - 1) / (out - 1) per axis.
#   x4 path  : W_in >= 4, W_out % 4 == 0, x scale <= 0.6, y 16-byte aligned
#   tile     : the x4 conditions and z scale <= 0.5, y scale <= 0.5, W_in % 4 == 0, W_in <= 128, x 16-byte aligned
#   general  : everything else
TRI_CASES = [
    # source shape, output size, kernel
    ((1, 3, 8, 12, 64), (16, 24, 128), "trilinear_fwd_tile_kernel"),     # scales 7/15, 11/23, 63/127 <= 0.5, W_in 64: tile; 3 planes
                                                                          # in one group of TT_CPT = 4
    ((2, 5, 5, 11, 8), (10, 23, 24), "trilinear_fwd_tile_kernel"),       # scales 4/9, 10/22, 7/23, W_in 8: tile; ragged tiles in z
                                                                          # (10 = 2*4 + 2) and y (23 = 2*8 + 7); 10 planes = 4 + 4 + 2
    ((3, 3, 5, 4, 6), (7, 8, 12), "trilinear_fwd_x4_kernel"),            # x scale 5/11, W_out 12: x4 path; W_in 6 % 4 != 0 (and z
                                                                          # scale 4/6 > 0.5): not tile; 9 planes = TRI_CPT 8 + 1
    ((1, 2, 5, 4, 8), (7, 8, 16), "trilinear_fwd_x4_kernel"),            # W_in 8 would suit the tile kernel; z scale 4/6 > 0.5 does not
    ((1, 3, 5, 6, 5), (9, 13, 10), "trilinear_fwd_kernel"),              # W_out 10 % 4 != 0: general kernel
    ((1, 2, 8, 7, 9), (4, 5, 3), "trilinear_fwd_kernel"),                # downsample (x scale 4 > 0.6): general kernel
    ((2, 5, 3, 4, 4), (5, 6, 7), "trilinear_fwd_kernel"),                # 10 planes = TRI_CPT 8 + 2 in the general kernel
]


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("shape,size,kernel", TRI_CASES)
def test_trilinear_fwd_lazy(shape, size, kernel, relu):
    """Every plane has its own {a, b}: a kernel that reads the coefficients of the wrong plane inside its plane group (4 in
    the tile kernel, 8 in the other two) or past a group's tail differs from the plain entry on xa."""
    N, C, D, H, W = shape
    raw, coef, special = lazy_operand(shape, 300)
    xa = materialise(raw, coef, relu)
    assert raw.data_ptr() % 16 == 0 and xa.data_ptr() % 16 == 0
    res = {}
    for name in ("lazy", "plain"):
        y = Placed((N, C) + size)
        if name == "lazy":
            call("dram_upsample_trilinear_ac_fwd_lazy", p(raw), p(coef), relu, p(y.t), N, C, D, H, W, *size)
        else:
            call("dram_upsample_trilinear_ac_fwd", p(xa), p(y.t), N, C, D, H, W, *size)
        torch.cuda.synchronize()
        assert y.intact(), (shape, name)
        res[name] = y.t
    ref = O.upsample_trilinear_ac(act64(raw.cpu().flatten(0, 1), coef.cpu(), relu).view(*shape), size=size)
    mx, l2 = rel_err(res["lazy"], ref)
    report(f"trilinear_fwd_lazy {shape}->{size} relu={relu} [{kernel}, coef]: max-rel {mx:.2e} rel-L2 {l2:.2e} vs fp64 "
           f"(plain entry on xa: max-rel {rel_err(res['plain'], ref)[0]:.2e})")
    assert torch.equal(res["lazy"], res["plain"])
    check(res["lazy"], ref, f"trilinear lazy {shape}->{size} relu={relu}", tol=1e-5)
    if "dead" in special and relu:
        assert bool((res["lazy"].flatten(0, 1)[special["dead"]] == 0).all())
    if "zero" in special:   # a constant plane b: three blends of at most five roundings each (1 - l1, two products, their sum,
        b = float(coef[special["zero"], 1])   # the tile kernel's multiplied-out weights) keep every output within 16 * 2^-24 * b
        assert float((res["lazy"].flatten(0, 1)[special["zero"]] - b).abs().max()) <= 16 * 2.0 ** -24 * b


# ------------------------------------------------------------------ 1x1x1 conv (the head)
K1_FWD_CASES = [
    # N, Cin, Cout, S, kernel
    (2, 64, 1, 4100, "conv1x1_fwd_kernel<true>"),     # the head: 1025 float4 per row = five blocks, the last with one thread
    (1, 5, 3, 693, "conv1x1_fwd_kernel<false>"),      # S % 4 != 0: scalar kernel
    (2, 13, 11, 1000, "conv1x1_fwd_kernel<true>"),    # two passes of MAXCO = 8 output channels, the second with 3
    (3, 1, 1, 12, "conv1x1_fwd_kernel<true>"),        # one input channel, three threads per sample
]


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("N,Ci,Co,S,kernel", K1_FWD_CASES)
def test_conv1x1_fwd_lazy(N, Ci, Co, S, kernel, relu):
    raw, coef, _ = lazy_operand((N, Ci, S), 400)
    xa = materialise(raw, coef, relu)
    w = torch.randn(Co, Ci, generator=g(402)).to(DEV)
    bias = torch.randn(Co, generator=g(403)).to(DEV)
    res = {}
    for name in ("lazy", "plain"):
        y = Placed((N, Co, S))
        if name == "lazy":
            call("dram_conv3d_k1_fwd_lazy", p(raw), p(coef), relu, p(w), p(bias), p(y.t), N, Ci, Co, S)
        else:
            call("dram_conv3d_k1_fwd", p(xa), p(w), p(bias), p(y.t), N, Ci, Co, S)
        torch.cuda.synchronize()
        assert y.intact(), name
        res[name] = y.t
    x64 = act64(raw.cpu().flatten(0, 1), coef.cpu(), relu).view(N, Ci, S)
    ref = torch.einsum("oc,ncs->nos", w.double().cpu(), x64) + bias.double().cpu()[None, :, None]
    mx, l2 = rel_err(res["lazy"], ref)
    report(f"conv1x1_fwd_lazy N={N} Cin={Ci} Cout={Co} S={S} relu={relu} [{kernel}, coef]: max-rel {mx:.2e} rel-L2 {l2:.2e} vs fp64")
    assert torch.equal(res["lazy"], res["plain"])
    check(res["lazy"], ref, "k1 lazy fwd vs fp64", tol=TOL)


K1_BWD_CASES = [
    # N, Cin, S, bytes off alignment of x, backward-weights kernel (Cout = 1; csrc/head.hip conv1x1_bwd_run: the vector kernel
    # needs S % 4 == 0 and 16-byte aligned dy and x; WG_VPB = 2048 voxels per block)
    (2, 64, 2 * 2048 + 12, 0, "conv1x1_wgrad_vec_kernel"),     # three blocks, the last with 12 voxels = three threads
    (2, 7, 4099, 0, "conv1x1_wgrad_kernel"),                   # S % 4 != 0: scalar kernel, three blocks
    (2, 64, 2 * 2048 + 12, 4, "conv1x1_wgrad_kernel"),         # the first case with x 4 bytes off: scalar kernel
]


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("N,Ci,S,shift,kernel", K1_BWD_CASES)
def test_conv1x1_bwd_lazy_one_output(N, Ci, S, shift, kernel, relu):
    """The head has ONE output channel: the multi-output kernel that test_conv1x1_bwd_lazy_several_outputs covers does not
    run.  The materialised operand sits at the same misalignment as the raw one, so both calls take the same kernel."""
    from dram_amd import _lib
    Co = 1
    raw, coef, _ = lazy_operand((N, Ci, S), 500, shift)
    xa = materialise(raw, coef, relu, shift)
    dy = torch.randn(N, Co, S, generator=g(502)).to(DEV)
    w = torch.randn(Co, Ci, generator=g(503)).to(DEV)
    nbytes = _lib.lib.dram_conv3d_k1_bwd_ws_bytes(N, Ci, Co, S)
    assert nbytes == N * 3 * Co * (Ci + 1) * 4
    res = {}
    for name in ("lazy", "plain"):
        dx, dw, db = Placed((N, Ci, S)), Placed((Co, Ci)), Placed((Co,))
        ws = Placed((nbytes // 4,))
        if name == "lazy":
            call("dram_conv3d_k1_bwd_lazy", p(dy), p(raw), p(coef), relu, p(w), p(dx.t), p(dw.t), p(db.t), p(ws.t), nbytes, N, Ci, Co, S)
        else:
            call("dram_conv3d_k1_bwd", p(dy), p(xa), p(w), p(dx.t), p(dw.t), p(db.t), p(ws.t), nbytes, N, Ci, Co, S)
        torch.cuda.synchronize()
        assert dx.intact() and dw.intact() and db.intact() and ws.intact(), name
        res[name] = (dx.t, dw.t, db.t)
    x64 = act64(raw.cpu().flatten(0, 1), coef.cpu(), relu).view(N, Ci, S)
    ref_dw = torch.einsum("nos,ncs->oc", dy.double().cpu(), x64)
    ref_db = dy.double().cpu().sum((0, 2))
    ref_dx = torch.einsum("oc,nos->ncs", w.double().cpu(), dy.double().cpu())
    e = [rel_err(res["lazy"][i], r)[0] for i, r in ((1, ref_dw), (2, ref_db), (0, ref_dx))]
    report(f"conv1x1_bwd_lazy N={N} Cin={Ci} Cout=1 S={S} x shift={shift} relu={relu} [{kernel}, coef]: max-rel vs fp64 "
           f"dw {e[0]:.2e} dbias {e[1]:.2e} dx {e[2]:.2e}")
    for i, what in enumerate(("dx", "dw", "dbias")):
        assert torch.equal(res["lazy"][i], res["plain"][i]), what
    check(res["lazy"][1], ref_dw, "k1 lazy dw vs fp64", tol=TOL)
    check(res["lazy"][2], ref_db, "k1 lazy dbias vs fp64", tol=TOL)
    check(res["lazy"][0], ref_dx, "k1 lazy dx vs fp64", tol=TOL)


# ------------------------------------------------------------------ coefficient producers from synthetic partials
EPS = 1e-5
MOMENTUM = float(np.float32(0.1))       # the entry point takes a float


def affine_params(C):
    """gamma of mixed sign with an exact zero at channel 2, beta non-zero."""
    gamma = torch.rand(C, generator=g(601)) + 0.5
    gamma[0::4] *= -1.0
    gamma[1] = gamma[1].abs()
    gamma[2] = 0.0
    beta = torch.randn(C, generator=g(602)) * 0.5
    beta = torch.where(beta.abs() < 0.05, torch.full_like(beta, 0.3), beta)
    return gamma, beta


def run_finalize(parts, kind, G, N, C, S, gamma, beta, running, ws_short=0):
    """dram_norm_finalize_parts on a float32 partials buffer; returns (rc, mean, rstd, rowcoef, running_mean, running_var)."""
    from dram_amd import _lib
    nparts = parts.shape[1]
    nstat = C if kind == BATCH else N * G
    dparts = parts.to(DEV).contiguous()
    mean, rstd, coef = Placed((nstat,)), Placed((nstat,)), Placed((N * C, 2))
    nbytes = _lib.lib.dram_norm_parts_ws_bytes(N, C, nparts)
    assert nbytes == N * C * -(-nparts // 2048) * 3 * 8
    ws = Placed((nbytes // 4,))
    rm = Placed((C,), src=running[0]) if running else None
    rv = Placed((C,), src=running[1]) if running else None
    dgamma, dbeta = (None if gamma is None else gamma.to(DEV)), (None if beta is None else beta.to(DEV))
    rc = _lib.lib.dram_norm_finalize_parts(p(dparts), nparts, p(dgamma), p(dbeta), p(mean.t), p(rstd.t), p(coef.t),
                                           p(rm.t) if running else None, p(rv.t) if running else None, MOMENTUM, EPS, kind, G, N, C, S,
                                           p(ws.t), nbytes - ws_short, stream())
    torch.cuda.synchronize()
    for t in (mean, rstd, coef, ws) + ((rm, rv) if running else ()):
        assert t.intact()
    return rc, mean.t.cpu(), rstd.t.cpu(), coef.t.cpu(), rm.t.cpu() if running else None, rv.t.cpu() if running else None, ws.t


def run_bn_parts_stats(parts, N, C, S, ws_short=0):
    from dram_amd import _lib
    nparts = parts.shape[1]
    dparts = parts.to(DEV).contiguous()
    out = Placed((2 * C,), dtype=torch.float64)
    nbytes = _lib.lib.dram_norm_parts_ws_bytes(N, C, nparts)
    ws = Placed((nbytes // 4,))
    rc = _lib.lib.dram_bn_parts_stats(p(dparts), nparts, p(out.t), N, C, S, p(ws.t), nbytes - ws_short, stream())
    torch.cuda.synchronize()
    assert out.intact() and ws.intact()
    return rc, out.t.cpu().view(C, 2)


def maxrel(got, ref):
    return ((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("case", STAT_CASES, ids=[c[0] for c in STAT_CASES])
def test_norm_finalize_parts(case, affine):
    """parts_reduce_kernel + norm_finalize_parts_kernel (and bn_parts_moments_kernel for the BatchNorm cases) against Chan's
    combine of the SAME float32 partials in fp64 (onload_reference.combine), so the kernel's own error is the fp64 merge
    order plus at most four float32 roundings per output: 4 * 2^-24 < 1e-6 of the output's largest magnitude.  BatchNorm
    runs with running statistics when affine, with NULL otherwise."""
    name, kind, G, N, C, S, nparts, offset = case
    y, cuts = stat_case_data(case)
    parts = make_parts(y, cuts)
    gamma, beta = affine_params(C) if affine else (None, None)
    running = (torch.randn(C, generator=g(603)) * 0.1, torch.rand(C, generator=g(604)) + 0.5) if (kind == BATCH and affine) else None
    rc, mean, rstd, coef, rm, rv, _ = run_finalize(parts, kind, G, N, C, S, gamma, beta, running)
    assert rc == 0
    st, ref_rstd, ref_coef = norm_reference(parts, kind, G, N, C, gamma, beta, EPS)
    errs = {"mean": maxrel(mean, st["mean"]), "rstd": maxrel(rstd, ref_rstd), "a": maxrel(coef[:, 0], ref_coef[:, 0]),
            "b": maxrel(coef[:, 1], ref_coef[:, 1])}
    if running:
        errs["running_mean"] = maxrel(rm, (1.0 - MOMENTUM) * running[0].double() + MOMENTUM * st["mean"])
        errs["running_var"] = maxrel(rv, (1.0 - MOMENTUM) * running[1].double() + MOMENTUM * st["var_unbiased"])
    if kind == BATCH:
        rc2, mm = run_bn_parts_stats(parts, N, C, S)
        assert rc2 == 0
        errs["bn_parts_stats mean"] = maxrel(mm[:, 0], st["mean"])
        errs["bn_parts_stats M2"] = maxrel(mm[:, 1], st["m2"])
    report(f"norm_finalize_parts {name} kind={'bn' if kind == BATCH else 'gn'} G={G} N={N} C={C} S={S} nparts={nparts} "
           f"affine={affine} [parts_reduce_kernel x{-(-nparts // 2048)} groups, norm_finalize_parts_kernel"
           f"{', bn_parts_moments_kernel' if kind == BATCH else ''}]: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= (1e-12 if k.startswith("bn_parts_stats") else 1e-6), (k, v)
    if affine:      # gamma == 0: a is an exact zero and b is beta itself
        z = (torch.arange(N * C) % C) == 2
        assert bool((coef[z, 0] == 0).all()) and torch.equal(coef[z, 1], beta[2].expand(int(z.sum())))
        assert bool((coef[:, 0] < 0).any()) and bool((coef[:, 0] > 0).any())


@pytest.mark.parametrize("name", ["bn_p7", "gn_g2_c6", "bn_p2049"])
def test_norm_parts_missing_count_poisons_one_statistic(name):
    """One row whose counts add up to S - 1 (a partial went missing): exactly that row's statistic is NaN -- save_mean,
    save_rstd and the {a, b} of every row of the statistic, so that no consumer applies a silently biased normalisation --
    and every other statistic stays finite and correct.  dram_bn_parts_stats poisons that channel."""
    case = next(c for c in STAT_CASES if c[0] == name)
    _, kind, G, N, C, S, nparts, _ = case
    y, cuts = stat_case_data(case)
    parts = make_parts(y, cuts)
    row = N * C - 2
    piece = int(torch.nonzero(parts[row, :, 2] >= 2)[-1])
    parts[row, piece, 2] -= 1.0
    assert float(parts[row, :, 2].sum()) == S - 1
    gamma, beta = affine_params(C)
    running = (torch.zeros(C), torch.ones(C)) if kind == BATCH else None
    rc, mean, rstd, coef, rm, rv, _ = run_finalize(parts, kind, G, N, C, S, gamma, beta, running)
    assert rc == 0
    srow = stat_of_row(kind, G, N, C)
    bad = int(srow[row])
    good = torch.arange(mean.numel()) != bad
    assert bool(torch.isnan(mean[bad])) and bool(torch.isnan(rstd[bad]))
    assert bool(torch.isnan(coef[srow == bad]).all())
    st, ref_rstd, ref_coef = norm_reference(parts, kind, G, N, C, gamma, beta, EPS)
    assert bool(torch.isfinite(mean[good]).all() and torch.isfinite(rstd[good]).all() and torch.isfinite(coef[srow != bad]).all())
    assert maxrel(mean[good], st["mean"][good]) <= 1e-6 and maxrel(rstd[good], ref_rstd[good]) <= 1e-6
    assert maxrel(coef[srow != bad], ref_coef[srow != bad]) <= 1e-6
    if kind == BATCH:
        rc2, mm = run_bn_parts_stats(parts, N, C, S)
        assert rc2 == 0 and bool(torch.isnan(mm[bad]).all()) and bool(torch.isfinite(mm[good]).all())
        assert maxrel(mm[good, 0], st["mean"][good]) <= 1e-12 and maxrel(mm[good, 1], st["m2"][good]) <= 1e-12
    report(f"norm_finalize_parts {name} with one count short in row {row}: statistic {bad} is NaN, the other "
           f"{int(good.sum())} agree with fp64")


def test_norm_parts_workspace_too_small():
    """One byte less than dram_norm_parts_ws_bytes: DRAM_EWS, and nothing is launched (every output keeps its NaN fill)."""
    from dram_amd import _lib
    case = next(c for c in STAT_CASES if c[0] == "bn_p2049")
    _, kind, G, N, C, S, nparts, _ = case
    y, cuts = stat_case_data(case)
    parts = make_parts(y, cuts)
    rc, mean, rstd, coef, _, _, ws = run_finalize(parts, kind, G, N, C, S, None, None, None, ws_short=1)
    assert rc == -2 and b"workspace" in _lib.lib.dram_last_error()
    assert bool(torch.isnan(mean).all() and torch.isnan(rstd).all() and torch.isnan(coef).all() and torch.isnan(ws).all())
    rc, mm = run_bn_parts_stats(parts, N, C, S, ws_short=1)
    assert rc == -2 and bool(torch.isnan(mm).all())
    assert _lib.lib.dram_norm_parts_ws_bytes(N, C, 0) == 0


# ------------------------------------------------------------------ norm backward: the ReLU mask recomputed from {a, b}
NORM_BWD_SHAPES = [
    (2, 4, 5, 9, 93),       # S = 4185: scalar kernels (S % 4 != 0), a second chunk of 89 elements
    (3, 4, 4, 33, 32),      # S = 4224: vector kernels, a second chunk of 128 elements
]


def norm_bwd_params(C):
    gamma = torch.tensor([-1.3, 0.7, 0.0, -0.6])[:C].clone()
    beta = torch.tensor([0.25, -0.4, 0.3, 0.5])[:C].clone()
    return gamma, beta


def grad_checks(tag, mod, ref, y, yr, xg, xr, kernels):
    e = {"y": rel_err(y, yr)[0], "dx": rel_err(xg.grad, xr.grad)[0], "dgamma": rel_err(mod.weight.grad, ref.weight.grad)[0],
         "dbeta": rel_err(mod.bias.grad, ref.bias.grad)[0]}
    report(f"{tag} [{kernels}]: max-rel vs fp64 " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    check(y, yr, tag + " fwd")
    check(xg.grad, xr.grad, tag + " dx")
    check(mod.weight.grad, ref.weight.grad, tag + " dgamma")
    check(mod.bias.grad, ref.bias.grad, tag + " dbeta")


@pytest.mark.parametrize("shape", NORM_BWD_SHAPES)
def test_batchnorm_relu_backward_mixed_sign_gamma(shape):
    """HipBatchNorm3d(relu=True), training and eval mode, against nn.BatchNorm3d + F.relu in fp64 on the CPU: with gamma < 0 the
    mask [a*x + b > 0] keeps the elements BELOW the mean, with gamma == 0 it is all or nothing (the sign of beta)."""
    from dram_amd.modules import HipBatchNorm3d
    C = shape[1]
    kernels = "row_bwd_reduce_kernel / row_bwd_apply_kernel<%s>" % ("true" if shape[2] * shape[3] * shape[4] % 4 == 0 else "false")
    x = torch.randn(*shape, generator=g(701)) * 1.7 + 0.6
    gy = torch.randn(*shape, generator=g(702))
    gamma, beta = norm_bwd_params(C)
    ref = torch.nn.BatchNorm3d(C)
    ref.weight.data, ref.bias.data = gamma.clone(), beta.clone()
    mod = HipBatchNorm3d(C)
    mod.load_state_dict(ref.state_dict())
    mod, ref = mod.to(DEV), ref.double()
    xr = x.double().requires_grad_(True)
    yr = F.relu(ref(xr))
    yr.backward(gy.double())
    xg = x.to(DEV).requires_grad_(True)
    y = mod(xg, relu=True)
    y.backward(gy.to(DEV))
    grad_checks(f"bn+relu train {shape}", mod, ref, y, yr, xg, xr, kernels)
    check(mod.running_mean, ref.running_mean, "bn running_mean")
    check(mod.running_var, ref.running_var, "bn running_var")
    assert bool((y[:, 2] == float(beta[2])).all())                                 # gamma == 0, beta > 0: the constant beta
    ref.eval(), mod.eval()
    xr2, xg2 = x.double().requires_grad_(True), x.to(DEV).requires_grad_(True)
    yr2 = F.relu(ref(xr2))
    yr2.backward(gy.double())
    y2 = mod(xg2, relu=True)
    y2.backward(gy.to(DEV))
    report(f"bn+relu eval {shape} [{kernels}]: max-rel vs fp64 y {rel_err(y2, yr2)[0]:.2e} dx {rel_err(xg2.grad, xr2.grad)[0]:.2e}")
    check(y2, yr2, "bn eval fwd")
    check(xg2.grad, xr2.grad, "bn eval dx")


@pytest.mark.parametrize("groups", ["one", "two", "all"])
@pytest.mark.parametrize("shape", NORM_BWD_SHAPES)
def test_groupnorm_relu_backward_mixed_sign_gamma(shape, groups):
    from dram_amd.modules import HipGroupNorm
    C = shape[1]
    G = {"one": 1, "two": 2, "all": C}[groups]
    kernels = "row_bwd_reduce_kernel / row_bwd_apply_kernel<%s>" % ("true" if shape[2] * shape[3] * shape[4] % 4 == 0 else "false")
    x = torch.randn(*shape, generator=g(711)) * 2.0 - 0.4
    gy = torch.randn(*shape, generator=g(712))
    gamma, beta = norm_bwd_params(C)
    ref = torch.nn.GroupNorm(G, C)
    ref.weight.data, ref.bias.data = gamma.clone(), beta.clone()
    mod = HipGroupNorm(G, C)
    mod.load_state_dict(ref.state_dict())
    mod, ref = mod.to(DEV), ref.double()
    xr = x.double().requires_grad_(True)
    yr = F.relu(ref(xr))
    yr.backward(gy.double())
    xg = x.to(DEV).requires_grad_(True)
    y = mod(xg, relu=True)
    y.backward(gy.to(DEV))
    grad_checks(f"gn+relu G={G} {shape}", mod, ref, y, yr, xg, xr, kernels)
