"""The seven 1x1x1 conv kernels of csrc/head.hip through the C ABI, one case per route, output pass and channel tail
(tests/k1_cases.py; tests/test_k1_cases_cpu.py proves each case's route from the library's own answer).

Every tensor sits between guard words at the misalignment the case asks for, every output is NaN before the call -- dx too:
the first backward-data pass must overwrite it and the later ones add to it -- and the workspace is exactly
dram_conv3d_k1_bwd_ws_bytes long.  Integer-valued inputs must reproduce the fp64 reference bit for bit; standard normal
inputs must stay within k * 2^-24 * sum |terms| per element, k per kernel as derived in tests/k1_cases.py.  A lazy case also
has to equal the plain entry on the materialised operand bit for bit.

Each case prints a `k1-accuracy:` line before it asserts (run with -s to see the figures; profiles/k1_accuracy.txt)."""
from collections import namedtuple

import numpy as np
import pytest
import torch

from dram_amd import _lib

import k1_cases as K
from gpu_buffers import Placed, lazy_operand, materialise, p, stream

pytestmark = pytest.mark.gpu
CASES = pytest.mark.parametrize("case", K.CASES, ids=K.IDS)
BWD = lambda ids: pytest.mark.parametrize("case", [K.BY_ID[i] for i in ids], ids=ids)
OUTS = ("dx", "dw", "db")
Dev = namedtuple("Dev", "x w bias dy coef")      # device tensors of a call; coef: None for the plain entry


def report(line):
    print("k1-accuracy: " + line)


def place(case, inp, x=None, coef=None):
    """The inputs on the device at the case's misalignments; x / coef replace those of `inp` when given (device tensors)."""
    put = lambda a, shift=0: None if a is None else Placed(a.shape, shift, src=torch.from_numpy(np.array(a))).t
    return Dev(put(inp.x, case.x_shift) if x is None else x, put(inp.w), put(inp.bias),
               put(inp.dy, case.dy_shift) if case.op == "bwd" else None, put(inp.coef) if coef is None else coef)


def run_fwd(case, t, lazy):
    dims = (case.N, case.Cin, case.Cout, case.S)
    y = Placed((case.N, case.Cout, case.S), case.out_shift)
    assert t.x.data_ptr() % 16 == case.x_shift and y.t.data_ptr() % 16 == case.out_shift
    if lazy:
        rc = _lib.lib.dram_conv3d_k1_fwd_lazy(p(t.x), p(t.coef), 1, p(t.w), p(t.bias), p(y.t), *dims, stream())
    else:
        rc = _lib.lib.dram_conv3d_k1_fwd(p(t.x), p(t.w), p(t.bias), p(y.t), *dims, stream())
    torch.cuda.synchronize()
    assert rc == 0, _lib.lib.dram_last_error()
    assert y.intact()
    return {"y": y.t.cpu()}


def run_bwd(case, t, lazy, outs=OUTS, ws_short=0):
    """One backward call that asks for `outs`; the others are NULL.  Returns (rc, the three poisoned-then-written buffers on
    the host, the workspace on the host).  No workspace is handed over when neither dw nor dbias is asked for."""
    dims = (case.N, case.Cin, case.Cout, case.S)
    bufs = {"dx": Placed((case.N, case.Cin, case.S), case.out_shift), "dw": Placed((case.Cout, case.Cin)), "db": Placed((case.Cout,))}
    nbytes = _lib.lib.dram_conv3d_k1_bwd_ws_bytes(*dims)
    assert nbytes == 4 * K.ws_floats(case)
    ws = Placed((nbytes // 4,))
    ptr = lambda name: p(bufs[name].t) if name in outs else None
    wsargs = (p(ws.t), nbytes - ws_short) if ("dw" in outs or "db" in outs) else (None, 0)
    assert t.x.data_ptr() % 16 == case.x_shift and t.dy.data_ptr() % 16 == case.dy_shift
    assert bufs["dx"].t.data_ptr() % 16 == case.out_shift
    if lazy:
        rc = _lib.lib.dram_conv3d_k1_bwd_lazy(p(t.dy), p(t.x), p(t.coef), 1, p(t.w), ptr("dx"), ptr("dw"), ptr("db"), *wsargs, *dims,
                                              stream())
    else:
        rc = _lib.lib.dram_conv3d_k1_bwd(p(t.dy), p(t.x), p(t.w), ptr("dx"), ptr("dw"), ptr("db"), *wsargs, *dims, stream())
    torch.cuda.synchronize()
    assert all(b.intact() for b in bufs.values()) and ws.intact(), case.id      # exactly ws_bytes: nothing behind them
    return rc, {k: b.t.cpu() for k, b in bufs.items()}, ws.t.cpu()


def run(case, t, lazy):
    if case.op == "fwd":
        return run_fwd(case, t, lazy), None
    rc, got, ws = run_bwd(case, t, lazy)
    assert rc == 0, _lib.lib.dram_last_error()
    return got, ws


def k_of(case, name, kernels):
    return {"y": K.k_fwd(case.Cin), "dx": K.k_dgrad(case.Cout)}.get(name) or K.K_WGRAD[kernels[1]]


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def workspace_use(case, kernels, ws):
    """The partials occupy the front of the workspace and the rest keeps its NaN fill."""
    used = K.partial_floats(case, kernels[1])
    assert not bool(torch.isnan(ws[:used]).any()), case.id
    assert bool(torch.isnan(ws[used:]).all()), case.id
    return used


# ------------------------------------------------------------------------------------------------ every case, exact inputs
@CASES
def test_exact_inputs_bit_for_bit(case):
    """Integer-valued inputs: no fp32 operation on any route rounds, so the result is the fp64 reference whatever the order
    of the sums.  NaN left anywhere (an element not written, a first pass that added to what it found) differs too."""
    kernels = K.library_kernels(case)
    assert case.kernel in kernels
    inp, ref = K.exact_inputs(case.id), K.exact_reference(case.id)
    got, ws = run(case, place(case, inp), case.lazy)
    wrong = {}
    for name, v in got.items():
        want = torch.from_numpy(ref[name].astype(np.float32))
        wrong[name] = (int((v != want).sum()), v.numel(), torch.equal(v, want))
    tail = ""
    if ws is not None:
        used = workspace_use(case, kernels, ws)
        tail = f"; {used} of {ws.numel()} workspace floats written"
    report(f"{case.id} exact [{', '.join(kernels)}]: " + ", ".join(f"{n} {w[0]} of {w[1]} differ" for n, w in wrong.items()) + tail)
    assert all(w[2] for w in wrong.values()), (case.id, wrong)


# ------------------------------------------------------------------------------------------------ every case, real inputs
@CASES
def test_real_inputs_within_the_derived_bound(case):
    """|got - ref| <= k * 2^-24 * sum |terms| per element against the fp64 restatement of the very float32 operands.  A lazy
    case runs on raw ~ N(0, 1) with a coefficient table that has a < 0, a == 0 and all-clamped rows: it must equal the plain
    entry on the materialised operand bit for bit, and that operand is what the reference is evaluated on."""
    kernels = K.library_kernels(case)
    inp = K.real_inputs(case.id)
    if case.lazy:
        raw, coef, _ = lazy_operand((case.N, case.Cin, case.S), 7000 + K.IDS.index(case.id), case.x_shift)
        xa = materialise(raw, coef, 1, case.x_shift)
        got, _ = run(case, place(case, inp, x=raw, coef=coef), True)
        plain, _ = run(case, place(case, inp, x=xa), False)
        assert all(same_bits(got[n], plain[n]) for n in got), case.id
        x = xa.cpu().numpy()
    else:
        got, _ = run(case, place(case, inp), False)
        x = inp.x
    ref = K.restate(x, inp.w, inp.bias, inp.dy if case.op == "bwd" else None)
    rows, ok = [], True
    for name, v in got.items():
        k = k_of(case, name, kernels)
        err = np.abs(v.numpy().astype(np.float64) - ref[name])
        bnd = K.bound(k, ref[name + "_abs"])
        finite = bool(np.isfinite(v.numpy()).all())
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bnd > 0, err / bnd, np.where(err == 0, 0.0, np.inf))
        worst = float(np.nan_to_num(ratio, nan=np.inf).max())
        rows.append(f"{name} k={k} max |err| / bound {worst:.3f} (max |err| {float(np.nan_to_num(err, nan=np.inf).max()):.2e})")
        ok = ok and finite and bool((err <= bnd).all())
    report(f"{case.id} real [{', '.join(kernels)}]{' = plain entry on the materialised operand' if case.lazy else ''}: " + "; ".join(rows))
    assert ok, (case.id, rows)


# ------------------------------------------------------------------------------------------------ the workspace contract
@BWD(["wv_ci17_s2052", "wm_ci9_co9_s3080", "wm_ci20_co17_s8196", "ws_co9_dy_off"])
def test_workspace_of_exactly_the_stated_size(case):
    """dram_conv3d_k1_bwd_ws_bytes is sized for blocks of 2048 voxels; the multi-output kernel writes one partial row per
    8192.  The exact size is accepted, the guard words behind it are intact (run_bwd), and the floats past
    N * ceil(S / 8192) * Cout * (Cin + 1) still hold their poison after a multi-kernel run."""
    kernels = K.library_kernels(case)
    rc, got, ws = run_bwd(case, place(case, K.real_inputs(case.id)), False)
    assert rc == 0
    used = workspace_use(case, kernels, ws)
    if kernels[1] == K.WM:
        assert used == case.N * K.cdiv(case.S, 8192) * case.Cout * (case.Cin + 1)
        if case.S > 2048:
            assert used < ws.numel()
    else:
        assert used == ws.numel()
    assert not any(bool(torch.isnan(v).any()) for v in got.values())


@BWD(["wv_ci17_s2052", "wm_ci9_co9_s3080", "ws_co9_dy_off", "d_vec_co17"])
@pytest.mark.parametrize("outs", [OUTS, ("dw",), ("db",)], ids=lambda o: "+".join(o))
def test_workspace_one_byte_short_is_refused_and_nothing_is_written(case, outs):
    rc, got, ws = run_bwd(case, place(case, K.real_inputs(case.id)), False, outs=outs, ws_short=1)
    assert rc == -2 and b"conv3d_k1_bwd: workspace too small" in _lib.lib.dram_last_error()
    assert all(bool(torch.isnan(v).all()) for v in got.values()), "a refused call wrote to an output"
    assert bool(torch.isnan(ws).all())


# ------------------------------------------------------------------------------------------------ optional outputs
@BWD(["wv_ci17_s2052", "wm_ci9_co9_s3080"])
def test_optional_outputs(case):
    """dw only, dbias only (sum_partials_kernel with dw == NULL), dx only (no workspace at all), dw + dbias without dx: what
    is asked for has the bits of the call that asks for everything, what is not stays untouched."""
    t = place(case, K.real_inputs(case.id))
    rc, full, _ = run_bwd(case, t, False)
    assert rc == 0 and not any(bool(torch.isnan(v).any()) for v in full.values())
    for outs in (("dw",), ("db",), ("dx",), ("dw", "db")):
        rc, got, ws = run_bwd(case, t, False, outs=outs)
        assert rc == 0, (outs, _lib.lib.dram_last_error())
        for name in OUTS:
            if name in outs:
                assert same_bits(got[name], full[name]), (case.id, outs, name)
            else:
                assert bool(torch.isnan(got[name]).all()), (case.id, outs, name)
        if outs == ("dx",):
            assert bool(torch.isnan(ws).all())
    report(f"{case.id} optional outputs: dw | db | dx | dw+db each bit-equal to the call with all three")


# ------------------------------------------------------------------------------------------------ fixed-order sums
@pytest.mark.parametrize("cid", ["f_vec_co17", "d_vec_co17", "ws_co9_dy_off", "wv_ci40_s2052", "wm_ci20_co17_s8196"])
def test_two_runs_give_the_same_bits(cid):
    case = K.BY_ID[cid]
    t = place(case, K.real_inputs(cid))
    a, _ = run(case, t, False)
    b, _ = run(case, t, False)
    assert all(same_bits(a[n], b[n]) for n in a), cid
