"""The clipping restatement (tests/clip_restatement.py) against torch.nn.utils.clip_grad_norm_ on the CPU, and the host side
of the device clipping: table and argument checks of the new entry points, the partial count, set_grad_clip's place outside
the state dict, rejections.  No kernel runs."""
import math

import numpy as np
import pytest
import torch

import clip_restatement as C
import optim_restatement as R
from dram_amd import _lib
from dram_amd import optim as DO

SIZES = [1, 5, 4090, 2, 1]                      # 4099 elements
NORM_TYPES = [2.0, math.inf]


def _grads(seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return [(scale * rng.standard_normal(n)).astype(np.float32) for n in SIZES]


def _torch_clip(grads, max_norm, norm_type, dtype):
    ps = [torch.nn.Parameter(torch.zeros(g.shape, dtype=dtype)) for g in grads]
    for p, g in zip(ps, grads):
        p.grad = torch.from_numpy(g).to(dtype, copy=True)
    norm = torch.nn.utils.clip_grad_norm_(ps, max_norm, norm_type)
    return norm, [p.grad.numpy() for p in ps]


@pytest.mark.parametrize("norm_type", NORM_TYPES)
@pytest.mark.parametrize("max_norm", [0.5, 1e3])        # clipping active (norm ~ 64 or ~ 4) and inactive
def test_restatement_is_torch_in_fp64(norm_type, max_norm):
    grads = _grads(1)
    norm, gs = _torch_clip(grads, max_norm, norm_type, torch.float64)
    want, c, scaled = C.clipped(grads, max_norm, norm_type)
    assert (c < 1.0) == (max_norm == 0.5)
    assert float(norm) == pytest.approx(want, rel=1e-12, abs=0)
    for a, b, g in zip(gs, scaled, grads):
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=0)
        # and so the coefficient itself
        np.testing.assert_allclose(a, g.astype(np.float64) * c, rtol=1e-12, atol=0)


def test_restatement_coefficient_keeps_nan_and_clamps():
    for t in (np.float32, np.float64):
        assert math.isnan(C.clip_coef(float("nan"), 1.0, t))
        assert C.clip_coef(float("inf"), 1.0, t) == 0.0
        assert C.clip_coef(0.0, 1.0, t) == 1.0
        assert C.clip_coef(1.0, 1e-3, t) < 1.0
    assert C.clip_coef(2.0, 1.0).dtype == np.float32
    # the three fp32 operations, spelled out
    n = np.float32(3.25)
    assert C.clip_coef(n, 0.7) == np.float32(0.7) / (n + np.float32(1e-6))
    assert math.isnan(C.total_norm([np.array([1.0, float("nan")], np.float32)], math.inf))
    assert math.isnan(C.total_norm([np.array([1.0, float("nan")], np.float32)], 2.0))
    assert C.total_norm([np.array([1.0, float("-inf")], np.float32)], 2.0) == math.inf
    assert C.total_norm([np.array([1e20, 1e20], np.float32)], 2.0) == pytest.approx(math.sqrt(2) * float(np.float32(1e20)), rel=1e-15)
    assert C.total_norm([], 2.0) == 0.0 and C.total_norm([], math.inf) == 0.0


@pytest.mark.parametrize("seed,scale", [(2, 1.0), (3, 1e-3), (4, 1e4)])
def test_torch_fp32_stays_inside_its_bound(seed, scale):
    """torch's own fp32 CPU evaluation (a norm per tensor, the norm of those) against the fp64 restatement: inside
    clip_restatement.torch_fp32_norm_bound, a count of ITS roundings (14.5 u here).  The same accounting, for a kernel that
    adds in fp64, leaves one fp32 rounding: norm_bound, which the GPU tests apply.  The inf-norm is exact for both."""
    grads = _grads(seed, scale)
    norm, _ = _torch_clip(grads, 1.0, 2.0, torch.float32)
    want = C.total_norm(grads, 2.0)
    bound = C.torch_fp32_norm_bound(want, SIZES)
    err = abs(float(norm) - want)
    print(f"torch fp32 2-norm: |err| = {err / (C.U * want):.3f} u, bound {bound / (C.U * want):.3f} u")
    assert err <= bound
    assert bound <= 16 * C.U * want                      # "a few ulps", not a tolerance
    assert C.norm_bound(want, SIZES, 2.0) <= 1.01 * C.U * want
    norm, _ = _torch_clip(grads, 1.0, math.inf, torch.float32)
    assert float(norm) == C.total_norm(grads, math.inf) and C.norm_bound(want, SIZES, math.inf) == 0.0


def _row(g=16, n=4, p=0):
    return DO._ENTRY.pack(p, g, 0, 0, 0, n, 0.0, 0.0)


def test_table_and_argument_errors_are_reported_without_a_gpu():
    q = 16                                               # a dummy non-null, aligned device pointer: nothing is launched
    calls = {
        "dram_optim_grad_norm": lambda table, count: _lib.call("dram_optim_grad_norm", table, count, 2, q, 0, None),
        "dram_optim_grad_scale": lambda table, count: _lib.call("dram_optim_grad_scale", table, count, q, None),
    }
    for name, fn in calls.items():
        with pytest.raises(_lib.DramHipError, match="null table"):
            fn(None, 1)
        with pytest.raises(_lib.DramHipError, match="tensors in one table"):
            fn(_row() * (DO.TABLE_CAPACITY + 1), DO.TABLE_CAPACITY + 1)
        with pytest.raises(_lib.DramHipError, match="tensors in one table"):
            fn(_row(), 0)
        with pytest.raises(_lib.DramHipError, match="tensor 1: element count"):
            fn(_row() + _row(n=0), 2)
        with pytest.raises(_lib.DramHipError, match="element count"):
            fn(_row(n=1 << 31), 1)
        with pytest.raises(_lib.DramHipError, match="tensor 0: gradient pointer not 4-byte aligned"):
            fn(_row(g=18), 1)
        with pytest.raises(_lib.DramHipError, match="null gradient pointer"):
            fn(_row(g=0), 1)
    # p, m, v, vmax are not required: the rows above have them NULL and fail for other reasons only
    with pytest.raises(_lib.DramHipError, match="negative partial_offset"):
        _lib.call("dram_optim_grad_norm", _row(), 1, 2, q, -1, None)
    with pytest.raises(_lib.DramHipError, match="null partials"):
        _lib.call("dram_optim_grad_norm", _row(), 1, 2, None, 0, None)
    for kind in (1, 3, -1):
        with pytest.raises(_lib.DramHipError, match="norm kind"):
            _lib.call("dram_optim_grad_norm", _row(), 1, kind, q, 0, None)
        with pytest.raises(_lib.DramHipError, match="norm kind"):
            _lib.call("dram_optim_grad_norm_finish", q, 1, kind, 1.0, q, None)
    with pytest.raises(_lib.DramHipError, match="null out"):
        _lib.call("dram_optim_grad_norm_finish", q, 1, 2, 1.0, None, None)
    with pytest.raises(_lib.DramHipError, match="null partials"):
        _lib.call("dram_optim_grad_norm_finish", None, 1, 0, 1.0, q, None)
    with pytest.raises(_lib.DramHipError, match="0 partials"):
        _lib.call("dram_optim_grad_norm_finish", q, 0, 2, 1.0, q, None)
    with pytest.raises(_lib.DramHipError, match="null gscale"):
        _lib.call("dram_optim_grad_scale", _row(), 1, None, None)
    # the scaled update entries check their table as the unscaled ones do
    with pytest.raises(_lib.DramHipError, match="tensors in one table"):
        _lib.call("dram_optim_adam_scaled", b"\0" * 56, DO.TABLE_CAPACITY + 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 0, 0, q, None)
    with pytest.raises(_lib.DramHipError, match="null pointer"):
        _lib.call("dram_optim_sgd_scaled", b"\0" * 56, 1, 1e-3, 0.9, 0.0, 0.0, 0, 0, q, None)
    with pytest.raises(_lib.DramHipError, match="gscale not 4-byte aligned"):
        _lib.call("dram_optim_sgd_scaled", DO._ENTRY.pack(16, 16, 0, 0, 0, 4, 0.0, 0.0), 1, 1e-3, 0.0, 0.0, 0.0, 0, 0, 18, None)


def test_partial_count_query():
    sizes = [1, 4095, 4096, 4097, 65536 + 7, 3]
    table = b"".join(_row(g=16 + 4 * i, n=n) for i, n in enumerate(sizes))
    want = sum((n + 4095) // 4096 for n in sizes)
    assert want == 1 + 1 + 1 + 2 + 17 + 1 == C.partial_count(sizes)
    assert _lib.lib.dram_optim_grad_norm_partials(table, len(sizes)) == want
    assert _lib.lib.dram_optim_grad_norm_partials(_row(n=(1 << 31) - 1), 1) == 1 << 19
    assert _lib.lib.dram_optim_grad_norm_partials(_row(n=0), 1) == 0
    assert b"element count" in _lib.lib.dram_last_error()
    assert C.OCHUNK == 4096 and C.KINDS == DO._NORM_KINDS


@pytest.mark.parametrize("case", ["adam", "adam_all", "adamw_wd_amsgrad", "sgd_momentum"])
def test_set_grad_clip_stays_out_of_the_state_dict(case):
    kind, kw = R.CASES[case]
    theirs = {"adam": torch.optim.Adam, "adamw": torch.optim.AdamW, "sgd": torch.optim.SGD}[kind]
    ours = {"adam": DO.Adam, "adamw": DO.AdamW, "sgd": DO.SGD}[kind]
    p, q = torch.nn.Parameter(torch.zeros(5)), torch.nn.Parameter(torch.zeros(5))
    ref, opt = theirs([p], lr=R.LR, **kw), ours([q], lr=R.LR, **kw)
    assert opt._clip is None and opt.last_grad_norm is None            # off by default
    opt.set_grad_clip(0.5, math.inf)
    assert opt._clip == (0.5, 0)
    a, b = opt.state_dict(), ref.state_dict()
    assert a["param_groups"] == b["param_groups"] and list(a["param_groups"][0]) == list(b["param_groups"][0])
    assert a["state"] == b["state"] == {}
    assert list(opt.param_groups[0]) == list(ref.param_groups[0])
    ref.load_state_dict(a)
    opt.load_state_dict(b)
    assert opt._clip == (0.5, 0)                                        # loading a checkpoint leaves the setting alone
    opt.set_grad_clip(None)
    assert opt._clip is None
    with pytest.raises(NotImplementedError, match="2.0 and inf"):
        opt.set_grad_clip(1.0, 3)
    assert opt._clip is None


def test_unsupported_norm_type_names_what_is_supported():
    p = torch.nn.Parameter(torch.zeros(3))
    p.grad = torch.ones(3)
    for nt in (3, 1.0, 0.5, -math.inf):
        with pytest.raises(NotImplementedError, match="supports 2.0 and inf"):
            DO.clip_grad_norm_([p], 1.0, norm_type=nt)
    assert torch.equal(p.grad, torch.ones(3))


def test_cpu_tensors_raise_and_nothing_needs_no_device():
    p = torch.nn.Parameter(torch.zeros(3))
    p.grad = torch.ones(3)
    for nt in NORM_TYPES:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            DO.clip_grad_norm_([p], 1.0, norm_type=nt)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            DO.clip_grad_norm_(p, 1.0, norm_type=nt, foreach=True)
    assert torch.equal(p.grad, torch.ones(3))
    d = torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))
    d.grad = torch.ones(3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DO.clip_grad_norm_([d], 1.0)
    # nothing to clip: a zero tensor, as torch returns
    q = torch.nn.Parameter(torch.zeros(3))
    for params in ([], [q]):
        out = DO.clip_grad_norm_(params, 1.0)
        ref = torch.nn.utils.clip_grad_norm_(params, 1.0)
        assert out.shape == ref.shape == () and out.dtype == ref.dtype and float(out) == float(ref) == 0.0
    # the fused route refuses CPU tensors as step() always did, before any state exists
    opt = DO.Adam([p], lr=1e-3)
    opt.set_grad_clip(1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
    assert len(opt.state[p]) == 0
    p.grad = None
    opt.step()
    assert float(opt.last_grad_norm) == 0.0
    assert "clip_grad_norm_" in DO.__all__
