"""The row kernels beyond their first chunk: PReLU forward / backward (csrc/act.hip), global max forward / backward
(csrc/act.hip), lobe-masked mean forward / backward and the per-channel sum (csrc/head.hip), ReLU forward / backward
(csrc/norm.hip), through dram_amd.functional and, where there is no wrapper, the C ABI.

They cut an (n, c) row of S floats into chunks of 8192 or walk it in a grid-stride loop capped at 1024 or 8192 blocks, write
per-chunk partials at part[row * nchunks + chunk] and finish in a second kernel that finds rows, chunks and PReLU parameters
by division and modulo.  The shapes here (tests/row_kernel_cases.py) are the smallest that reach each of those paths: S one
below, at and one above a chunk and 3 chunks + 77; 69 rows / 70 channels (a second finalise block of 64); more than 256
partials per PReLU parameter; one row past each block cap; global max with the maximum on either end, on one thread twice,
on two threads, and rows of equal values, -inf, +inf and NaN.

Structural cases use integer-valued inputs on which fp32 addition is exact in any order (row_kernel_cases.py's docstring;
tests/test_row_kernels_cpu.py asserts the condition), so a dropped, repeated or misplaced element changes the answer and the
check is torch.equal: no tolerance.  One randn case per reduction checks precision against fp64 under a bound derived from
the kernels' summation order (row_kernel_cases.sum_bound).  Outputs handed over by this file are filled with NaN first."""
import pytest
import torch
import torch.nn.functional as F

import row_kernel_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def p(t):
    return None if t is None else t.data_ptr()


def call(name, *args):
    from dram_amd import _lib
    _lib.call(name, *args, torch.cuda.current_stream().cuda_stream)


def ws_bytes(name, N, C, S):
    from dram_amd import _lib
    return int(getattr(_lib.lib, name)(N, C, S))


def nan_buffer(nbytes):
    return torch.full((max(nbytes // 4, 4),), NAN, dtype=torch.float32, device=DEV)


# ------------------------------------------------------------------------------------------------ masked mean
def masked_mean_abi(x, m):
    """dram_masked_mean_fwd on NaN-filled outputs and workspace -> (out, msum) on the host."""
    N, C = x.shape[:2]
    S = x.numel() // (N * C)
    out, msum = nan_buffer(N * C * 4)[:N * C], nan_buffer(N * 4)[:N]
    nb = ws_bytes("dram_masked_mean_ws_bytes", N, C, S)
    assert nb == N * C * -(-S // K.CHUNK) * 2 * 4
    ws = nan_buffer(nb)
    call("dram_masked_mean_fwd", p(x), p(m), p(out), p(msum), p(ws), nb, N, C, S)
    torch.cuda.synchronize()
    return out.cpu().view(N, C), msum.cpu()


@pytest.mark.parametrize("case", K.MASKED_MEAN_CASES, ids=lambda c: c[0])
def test_masked_mean_chunks_bit_exact(case):
    """69 rows x 1, 1, 2 and 4 chunks (the last of 8191 / 8192 / 1 / 77 elements), a mask per sample, sample 1 with ONE
    voxel, in the last chunk.  out, msum and dx bit for bit; fp32 division on the device is correctly rounded (the library
    is built without fast-math), so dx needs no ulp of slack."""
    from dram_amd import functional as HF
    _, N, C, S = case
    x, dout, m = K.ints((N, C, S), K.DATA_MAX, 11), K.ints((N, C), K.COT_MAX, 12), K.masks(N, S, 13)
    ref = K.masked_mean_ref(x, m, dout)
    xg = x.view(N, C, 1, 1, S).to(DEV).requires_grad_(True)
    mg = m.view(N, 1, 1, 1, S).to(DEV)
    out = HF.masked_mean(xg, mg)
    out.backward(dout.to(DEV))
    assert torch.equal(out.detach().cpu(), ref["out"])
    assert torch.equal(xg.grad.cpu().view(N, C, S), ref["dx"])
    out2, msum = masked_mean_abi(xg.detach(), mg)
    assert torch.equal(out2, ref["out"]) and torch.equal(msum, ref["msum"])


def test_masked_mean_all_ones_is_global_avg():
    """models.pooling_dense_features 'global_avg': the all-ones mask at 4 chunks, against float32(exact sum / S)."""
    import models
    x = K.ints((3, 23) + K.DHW_MULTI, K.DATA_MAX, 14)
    dout = K.ints((3, 23), K.COT_MAX, 18)
    ref = K.masked_mean_ref(x.view(3, 23, -1), torch.ones(3, K.S_MULTI), dout)
    xg = x.to(DEV).requires_grad_(True)
    out = models.pooling_dense_features(xg, None, "global_avg")
    out.backward(dout.to(DEV))
    assert torch.equal(out.detach().cpu(), ref["out"])
    assert torch.equal(xg.grad.cpu().view(3, 23, -1), ref["dx"])


def test_masked_mean_per_channel_mask_branch():
    """models.pooling_dense_features with a [B, C, ...] mask: one masked mean of N rows per channel, 4 chunks each."""
    import models
    N, C = 3, 4
    x, dout = K.ints((N, C) + K.DHW_MULTI, K.DATA_MAX, 11), K.ints((N, C), K.COT_MAX, 12)
    m = K.masks(N * C, K.S_MULTI, 13).view((N, C) + K.DHW_MULTI)
    ref = K.masked_mean_ref(x.view(N, C, -1), m.view(N, C, -1), dout)
    xg = x.to(DEV).requires_grad_(True)
    out = models.pooling_dense_features(xg, m.to(DEV))
    out.backward(dout.to(DEV))
    assert torch.equal(out.detach().cpu(), ref["out"])
    assert torch.equal(xg.grad.cpu().view(N, C, -1), ref["dx"])


def test_masked_mean_backward_past_the_block_cap():
    """One row of 1024 * 256 + 300 voxels: masked_mean_bwd_kernel's grid is capped at 1024 blocks, the last 300 elements are
    written in a second lap."""
    from dram_amd import functional as HF
    S = K.S_MEAN_BWD
    x, dout, m = K.ints((1, 1, S), K.DATA_MAX, 21), torch.tensor([[3.0]]), K.masks(1, S, 22)
    m[0, S - 300:] = 1.0
    ref = K.masked_mean_ref(x, m, dout)
    xg = x.view(1, 1, 1, 1, S).to(DEV).requires_grad_(True)
    out = HF.masked_mean(xg, m.view(1, 1, 1, 1, S).to(DEV))
    out.backward(dout.to(DEV))
    assert torch.equal(out.detach().cpu(), ref["out"])
    assert torch.equal(xg.grad.cpu().view(1, 1, S), ref["dx"])


# ------------------------------------------------------------------------------------------------ channel sum
def channel_sum(x):
    N, C, S = x.shape
    out = nan_buffer(C * 4)[:C]
    nb = ws_bytes("dram_channel_sum_ws_bytes", N, C, S)
    assert nb == N * C * -(-S // K.CHUNK) * 4
    ws = nan_buffer(nb)
    call("dram_channel_sum", p(x), p(out), p(ws), nb, N, C, S)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("case", K.CHANNEL_SUM_CASES, ids=lambda c: c[0])
def test_channel_sum_chunks_bit_exact(case):
    """2 x 70 rows: channel c adds rows c and 70 + c; 70 channels need a second finalise block (6 live threads)."""
    _, N, C, S = case
    x = K.ints((N, C, S), K.DATA_MAX, 15)
    assert torch.equal(channel_sum(x.to(DEV)), K.channel_sum_ref(x))


# ------------------------------------------------------------------------------------------------ PReLU
def run_prelu(x, a, dy, x_grad):
    from dram_amd import functional as HF
    xg = x.to(DEV).requires_grad_(x_grad)
    ag = a.to(DEV).requires_grad_(True)
    y = HF.prelu(xg, ag)
    y.backward(dy.to(DEV))
    return y.detach().cpu(), None if xg.grad is None else xg.grad.cpu(), ag.grad.cpu()


@pytest.mark.parametrize("x_grad", [True, False], ids=["dx", "no_dx"])
@pytest.mark.parametrize("case", K.PRELU_CHUNK_CASES + K.PRELU_DA_CASES, ids=lambda c: c[0])
def test_prelu_chunks_bit_exact(case, x_grad):
    """Forward, dx and da for one slope and one per channel, at every chunk count of S_CHUNKED and at the three shapes
    that make prelu_da_kernel loop (more than 256 partials per parameter) and decompose rows as r * C + p.  Without
    x.requires_grad the backward kernel gets dx == nullptr and must still produce the same da."""
    _, N, C, nparam, S = case
    x, dy, a = K.ints((N, C, S), K.DATA_MAX, 16), K.ints((N, C, S), K.COT_MAX, 17), K.slopes(nparam)
    ref = K.prelu_ref(x, a, dy)
    y, dx, da = run_prelu(x, a, dy, x_grad)
    assert torch.equal(y, ref["y"])
    assert torch.equal(da, ref["da"])
    if x_grad:
        assert torch.equal(dx, ref["dx"])
    else:
        assert dx is None


def test_prelu_forward_past_the_block_cap():
    """One row of 1024 * 2048 + 517 voxels: 1024 blocks, every thread 8 elements and the first 517 a ninth."""
    S = K.S_STREAM
    x, dy, a = K.ints((1, 1, S), K.DATA_MAX, 23), K.ints((1, 1, S), K.COT_MAX, 24), K.slopes(1)
    ref = K.prelu_ref(x, a, dy)
    y, dx, da = run_prelu(x, a, dy, True)
    assert torch.equal(y, ref["y"]) and torch.equal(dx, ref["dx"]) and torch.equal(da, ref["da"])


# ------------------------------------------------------------------------------------------------ global max
def run_global_max(x, dout):
    from dram_amd import functional as HF
    xg = x.to(DEV).requires_grad_(True)
    out = HF.global_max(xg)
    out.backward(dout.to(DEV))
    return out.detach().cpu(), xg.grad.cpu()


@pytest.mark.parametrize("case", K.GMAX_CASES, ids=lambda c: f"{c[0]}-S{c[1]}")
def test_global_max_matches_adaptive_max_pool3d(case):
    """Values, int64 indices and dx of 5 rows against F.adaptive_max_pool3d(x, 1, return_indices=True) and its autograd on
    the CPU, bit for bit: first maximum among equal values (within one thread, across two threads through the tree -- the
    lower index also when it sits on the higher thread), index 0 of an all -inf row, and ATen's NaN rule: a NaN beats any
    number and the LAST NaN of the row is kept."""
    pattern, S = case
    x, want = K.gmax_input(pattern, S)
    dout = K.ints((1, K.GMAX_ROWS), K.COT_MAX, 19)
    xc = x.clone().requires_grad_(True)
    val, idx = F.adaptive_max_pool3d(xc, 1, return_indices=True)
    val.backward(dout.view_as(val))
    assert torch.equal(idx.view(1, -1), want)

    from dram_amd import functional as HF
    xg = x.to(DEV).requires_grad_(True)
    out = HF.global_max(xg)
    got_idx = out.grad_fn.saved_tensors[0].cpu()
    out.backward(dout.to(DEV))
    assert got_idx.dtype == torch.int64 and torch.equal(got_idx, want), (got_idx.tolist(), want.tolist())
    assert K.same_values(out.detach().cpu(), val.detach().view(1, -1))
    assert torch.equal(xg.grad.cpu(), xc.grad)


def test_global_max_backward_past_the_block_cap():
    """One row of 1024 * 2048 + 517 voxels with the maximum in the second lap of global_max_bwd_kernel's capped grid."""
    S = K.S_STREAM
    x = K.ints((1, 1, 1, 1, S), K.DATA_MAX, 25)
    x.view(-1)[S - 2] = 9.0
    out, dx = run_global_max(x, torch.tensor([[3.0]]))
    want = torch.zeros(S)
    want[S - 2] = 3.0
    assert out.tolist() == [[9.0]] and torch.equal(dx.view(-1), want)


# ------------------------------------------------------------------------------------------------ ReLU
@pytest.mark.parametrize("n", K.RELU_SIZES)
def test_relu_bit_exact(n):
    """HF.relu forward and backward against torch.relu and its autograd on finite inputs with exact zeros, at 1, 255 and 257
    elements and past the 8192-block cap of the grid-stride loop (the last 1000 elements take a second lap).  NaN handling
    of the fmaxf that every fused kernel shares is not this test's: there is no NaN in the input."""
    from dram_amd import functional as HF
    x, dy = K.relu_input(n, 26)
    xc = x.clone().requires_grad_(True)
    yc = torch.relu(xc)
    yc.backward(dy)
    xg = x.to(DEV).requires_grad_(True)
    y = HF.relu(xg)
    y.backward(dy.to(DEV))
    assert torch.equal(y.detach().cpu(), yc.detach())
    assert torch.equal(xg.grad.cpu(), xc.grad)
    assert bool((xc.grad[x == 0] == 0).all())


# ------------------------------------------------------------------------------------------------ real-valued, derived bound
def check_bound(kind, got, ref, sum_abs):
    err, bound = (got.double() - ref).abs(), K.sum_bound(sum_abs, ref)
    print(f"row-kernel-accuracy: {kind}: worst err / bound {(err / bound).max().item():.3f}, "
          f"worst err {err.max().item():.3e}, over max |ref| {(err.max() / ref.abs().max()).item():.2e}")
    assert got.dtype == torch.float32 and got.shape == ref.shape
    assert bool(torch.isfinite(got).all()) and bool((err <= bound).all()), (kind, (err / bound).max().item())


def test_masked_mean_real_values_within_the_derived_bound():
    """randn at 4 chunks against fp64: |got - ref| <= (41 + 2) * 2^-24 * sum |terms| + 2^-24 * |ref| per row (derivation at
    row_kernel_cases.sum_bound)."""
    from dram_amd import functional as HF
    t, ref, sum_abs = K.real_case("masked_mean")
    check_bound("masked_mean", HF.masked_mean(t["x"].to(DEV), t["m"].to(DEV)).cpu(), ref, sum_abs)


def test_channel_sum_real_values_within_the_derived_bound():
    t, ref, sum_abs = K.real_case("channel_sum")
    check_bound("channel_sum", channel_sum(t["x"].to(DEV)), ref, sum_abs)


def test_prelu_da_real_values_within_the_derived_bound():
    t, ref, sum_abs = K.real_case("prelu_da")
    _, _, da = run_prelu(t["x"], t["a"], t["dy"], False)
    check_bound("prelu_da", da, ref, sum_abs)
