"""Every row of the nine 3x3x3 conv kernel tables launched once, in-process, on the case tests/conv_row_cases.py files under its
name (tests/test_conv_rows_cpu.py proves without a device that the table covers the library's rows and that the plan sends each
case to its row).  Each launch is bracketed by the library's launch counters: exactly the row's family moves, by one; and the
library's choice, asked again for the device tensors of the launch (their real alignment), names the row itself.

Outputs, statistics partials, dW and its partial slabs hold NaN before the launch, so an unwritten element fails.  dW and the
slabs are allocated inside conv3d_k3_launch_wgrad, in that order: with the allocator's cache emptied, blocks of their sizes are
taken in the same order, filled with NaN and freed just before the launch.  The launch's two requests then meet the free lists
the poisoned ones met and get the same blocks; the test asserts that for dW (the same address) and that the launch made the
allocator reserve no new memory.

References in fp64 on the CPU over the activated, cropped and concatenated operand: torch.nn.functional.conv3d for a forward,
conv_transpose3d for backward-data, autograd of conv3d for dW.  Bound: `check` of test_gpu_parity.py at its 1e-4 (max-abs over
max |reference|, and relative L2), the bound every other test of these kernels uses.  Statistics as test_gpu_fwd_blocks.py checks
them (`_check_stats`; `_act` and `_window` come from there too, while its `_counted` looks the family up in that file's own
table, so the one below takes it from the ledger).  A failure names where the worst element lies: the channel tile and the box
of a forward row, the (co, ci) tile and the tap of a backward-weights row.
"""
import time

import pytest
import torch
import torch.nn.functional as F

import conv_row_cases as RC
import test_conv_rows_cpu as LEDGER
import test_gpu_fwd_blocks as FB
from conv_row_cases import CASES
from onload_reference import coef_table
from test_gpu_parity import TOL, check, rel_err

NAN = float("nan")


def _rand(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _place(t, off):
    """A device copy of `t` whose base pointer is `off` bytes past a 16-byte boundary."""
    store = torch.empty(t.numel() + 4, device="cuda")
    v = store[off // 4:off // 4 + t.numel()].view_as(t)
    v.copy_(t)
    assert v.data_ptr() % 16 == off
    return v


def _inputs(row):
    """CPU tensors of a row's case: x1, x2 (or None), w[Cout][C1 + C2][3][3][3] and the coefficient tables of the two sources."""
    c = CASES[row]
    seed = 1000 * (list(CASES).index(row) + 1)
    x1 = _rand(seed + 1, c.N, c.C1, *c.dhw)
    x2 = _rand(seed + 2, c.N, c.C2, *(a + b for a, b in zip(c.dhw, c.excess))) if c.C2 else None
    w = _rand(seed + 3, c.Cout, c.C1 + c.C2, 3, 3, 3) / ((c.C1 + c.C2) * 27) ** 0.5
    g = torch.Generator().manual_seed(seed + 4)
    coef1 = coef_table(c.N * c.C1, g)[0].reshape(-1)
    coef2 = coef_table(c.N * c.C2, g)[0].reshape(-1) if c.C2 else None
    return x1, x2, w, coef1, coef2


def _operand(row, x1, x2, coef1, coef2):
    """fp64 x1 ++ crop(x2), lazily normalised when coefficients are given: the first source with ReLU, the second without."""
    c = CASES[row]
    xin = FB._act(x1, coef1, True)
    if c.C2:
        xin = torch.cat([xin, FB._act(FB._window(x2, c.dhw), coef2, False)], 1)
    return xin


def _counted(row, launch):
    """Run `launch`; exactly the row's family moved, by one."""
    from dram_amd import functional as HF
    torch.cuda.synchronize()
    before = HF.conv_launch_counts()
    out = launch()
    torch.cuda.synchronize()
    after = HF.conv_launch_counts()
    moved = {k: after[k] - before[k] for k in range(HF.K3_KINDS) if after[k] != before[k]}
    assert moved == {LEDGER.family(row): 1}, (row, moved)
    return out


def _worst(got, ref):
    d = (got.detach().double().cpu() - ref).abs()
    return [int(v) for v in torch.unravel_index(torch.argmax(d), d.shape)]       # (a NaN counts as the maximum)


def _where_fwd(row, channel0=0):
    (bx, by, bz), tile = RC.geometry(row)

    def where(got, ref):
        n, ch, z, y, x = _worst(got, ref)
        return (f"sample {n}, channel {ch + channel0} = channel tile {(ch + channel0) // tile} of {tile}, "
                f"box (z, y, x) = ({z // bz}, {y // by}, {x // bx}) of {bx}x{by}x{bz}, voxel ({z}, {y}, {x})")
    return where


def _where_wgrad(row):
    _, (tco, tci) = RC.geometry(row)

    def where(got, ref):
        co, ci, kz, ky, kx = _worst(got, ref)
        return f"dW[{co}][{ci}] = co tile {co // tco} of {tco}, ci tile {ci // tci} of {tci}, tap ({kz}, {ky}, {kx}); summed over every box"
    return where


def _verify(got, ref, what, where, label="conv-row"):
    mx, l2 = rel_err(got, ref)
    print(f"{label}: {what}: max-rel {mx:.3e}, rel-L2 {l2:.3e}")
    if not (mx <= TOL and l2 <= TOL):
        what += " -- worst at " + where(got, ref)
    check(got, ref, what)


def _forward(row, x1, x2, w, bias=None, lazy=None, stats=False):
    from dram_amd import functional as HF
    from dram_amd import _lib
    c = CASES[row]
    src = HF.CatView(_place(x1, c.off), None if x2 is None else x2.cuda(), c.dhw, channels=c.C1 + c.C2)
    assert src.off == (FB.CROP if c.C2 else (0, 0, 0))
    assert HF.conv_fwd_kernel_name(c.dhw, c.Cout, c.C1 + c.C2, fused=lazy is not None, src=src.src) == row
    wt = HF._pack(w.cuda(), 0)
    y = torch.full((c.N, c.Cout, *c.dhw), NAN, device="cuda")
    nparts = _lib.lib.dram_conv3d_k3_stats_parts(c.C1 + c.C2, c.Cout, *c.dhw) if stats else 0
    parts = torch.full((c.N * c.Cout * nparts * 3,), NAN, device="cuda") if stats else None
    b = None if bias is None else bias.cuda()
    _counted(row, lambda: HF.conv3d_k3_launch_fwd(src, wt, b, y, lazy=lazy, parts=parts, nparts=nparts))
    return y, parts, nparts


def _run_fwd(row, label="conv-row"):
    c = CASES[row]
    x1, x2, w, _, _ = _inputs(row)
    bias = _rand(7, c.Cout)
    ref = F.conv3d(_operand(row, x1, x2, None, None), w.double(), bias.double(), padding=1)
    y, _, _ = _forward(row, x1, x2, w, bias=bias)
    _verify(y, ref, row, _where_fwd(row), label)


def _run_fused(row):
    c = CASES[row]
    x1, x2, w, coef1, coef2 = _inputs(row)
    if c.C1 + c.C2 == 1:        # the first-layer kernels take a plain source: the statistics epilogue only
        coef1 = None
    ref = F.conv3d(_operand(row, x1, x2, coef1, coef2), w.double(), None, padding=1)
    lazy = (None if coef1 is None else coef1.cuda(), 1, None if coef2 is None else coef2.cuda(), 0)
    y, parts, nparts = _forward(row, x1, x2, w, lazy=lazy, stats=True)
    _verify(y, ref, row, _where_fwd(row))
    FB._check_stats(parts, nparts, y, c.dhw, row)


def _run_bwd_data(row):
    """dx of y = conv3d(x1 ++ crop(x2), w) from dy: channels [0, C1) into dx1, the rest into the crop window of dx2, which holds
    NaN inside the window and 0 outside before the launch; outside stays exactly 0."""
    from dram_amd import functional as HF
    c = CASES[row]
    x1, x2, w, _, _ = _inputs(row)
    dy = _rand(8, c.N, c.Cout, *c.dhw)
    ref = F.conv_transpose3d(dy.double(), w.double(), None, padding=1)
    dx1 = torch.full(tuple(x1.shape), NAN, device="cuda")
    dx2 = torch.zeros(tuple(x2.shape), device="cuda")
    FB._window(dx2, c.dhw).fill_(NAN)
    wt = HF._pack(w.cuda(), 1)
    dyd = _place(dy, c.off)
    assert HF.conv_fwd_kernel_name(c.dhw, c.C1 + c.C2, c.Cout, dst_split=HF.CatView(dx1, dx2, c.dhw).split, src=(dyd, None, 0)) == row
    _counted(row, lambda: HF.conv3d_k3_launch_bwd_data(dyd, wt, dx1, dx2))
    _verify(torch.cat([dx1, FB._window(dx2, c.dhw)], 1), ref, row, _where_fwd(row))
    outside = dx2.cpu().clone()
    FB._window(outside, c.dhw).zero_()
    assert bool((outside == 0).all()), f"{row}: dx2 written outside its crop window"


def _run_wgrad(row):
    from dram_amd import functional as HF
    from dram_amd import _lib
    c = CASES[row]
    ci = c.C1 + c.C2
    x1, x2, w, coef1, coef2 = _inputs(row)
    if not c.lazy:
        coef1 = coef2 = None
    dy = _rand(8, c.N, c.Cout, *c.dhw)
    wr = torch.zeros(c.Cout, ci, 3, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv3d(_operand(row, x1, x2, coef1, coef2), wr, None, padding=1).backward(dy.double())
    src = HF.CatView(_place(x1, c.off), None if x2 is None else x2.cuda(), c.dhw, channels=ci)
    assert src.off == (FB.CROP if c.C2 else (0, 0, 0))
    dyd = _place(dy, c.off)
    lazy = (None if coef1 is None else coef1.cuda(), 1, None if coef2 is None else coef2.cuda(), 0)
    assert HF.conv_wgrad_kernel_name(c.N, c.dhw, c.Cout, c.C1, c.C2, lazy=c.lazy) == row
    wd = torch.empty(c.Cout, ci, 3, 3, 3, device="cuda")
    # NaN in the blocks the launch is about to take for dW and for the partial slabs (the launch's own requests, in its order)
    ws_bytes = max(int(_lib.lib.dram_conv3d_k3_wgrad_ws_bytes(c.N, ci, c.Cout, *c.dhw)), 16)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    poison_dw = torch.empty_like(wd).fill_(NAN)
    poison_ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    poison_ws.view(torch.float32).fill_(NAN)
    where_dw, reserved = poison_dw.data_ptr(), torch.cuda.memory_reserved()
    torch.cuda.synchronize()
    del poison_dw, poison_ws
    dw = _counted(row, lambda: HF.conv3d_k3_launch_wgrad(src, dyd, wd, lazy=lazy))
    assert dw.data_ptr() == where_dw and torch.cuda.memory_reserved() == reserved, f"{row}: the launch did not take the poisoned blocks"
    _verify(dw, wr.grad, row, _where_wgrad(row))


@pytest.mark.gpu
@pytest.mark.parametrize("row", list(CASES))
def test_row(row):
    t0 = time.perf_counter()
    mode = CASES[row].mode
    if mode == "fwd":
        _run_fwd(row)
    elif mode == "fused":
        _run_fused(row)
    elif mode == "fwd+fused":       # rows without a FUSED template argument: once with bias, once with statistics
        _run_fwd(row, label="conv-row (bias launch)")
        _run_fused(row)
    elif mode == "bwd-data":
        _run_bwd_data(row)
    else:
        assert mode == "wgrad", mode
        _run_wgrad(row)
    print(f"conv-row-seconds: {row}: {time.perf_counter() - t0:.2f}")
