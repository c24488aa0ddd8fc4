"""The optimiser restatement (tests/optim_restatement.py) against torch's own optimisers on the CPU, the fp32 error bound
against torch's fp32 ones, and the host side of dram_amd.optim: state layout, validation, rejections.  No kernel runs."""
import numpy as np
import pytest
import torch

import optim_restatement as R
from dram_amd import optim as DO

TORCH = {"adam": torch.optim.Adam, "adamw": torch.optim.AdamW, "sgd": torch.optim.SGD}
OURS = {"adam": DO.Adam, "adamw": DO.AdamW, "sgd": DO.SGD}
N = 4099


def _torch_run(kind, kw, p0, gs, dtype, lr=R.LR, skip=()):
    p = torch.nn.Parameter(torch.from_numpy(p0).to(dtype, copy=True))
    opt = TORCH[kind]([p], lr=lr, **kw)
    for i, g in enumerate(gs):
        p.grad = None if i in skip else torch.from_numpy(g).to(dtype)
        opt.step()
    return p, opt


def _state_arrays(kind, opt, p):
    st = opt.state[p]
    if kind == "sgd":
        return {"buf": st["momentum_buffer"].numpy()} if "momentum_buffer" in st else {}
    out = {"m": st["exp_avg"].numpy(), "v": st["exp_avg_sq"].numpy()}
    if "max_exp_avg_sq" in st:
        out["vmax"] = st["max_exp_avg_sq"].numpy()
    return out


def _pin(case, p0, gs, check):
    kind, kw = R.CASES[case]
    p, opt = _torch_run(kind, kw, p0, gs, torch.float64, skip=(2,))
    run = R.make_run(kind, kw, p0)
    for i, g in enumerate(gs):
        run.step(None if i == 2 else g, R.LR)
    check("p", p.detach().numpy(), run.p)
    for k, a in _state_arrays(kind, opt, p).items():
        check(k, a, getattr(run, k))
    if kind != "sgd":
        assert float(opt.state[p]["step"]) == run.t == 4


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_restatement_is_torch_in_fp64(case):
    """5 steps (the third without a gradient) of torch's optimiser in fp64 on the CPU: the restatement agrees to 1e-12
    relative, element by element.  torch orders the arithmetic differently (m by lerp), so a relative tolerance on the RESULT
    has a meaning only where nothing cancels: here every gradient (after maximize) has the sign of its parameter, so that
    g', m, buf and the weight-decay term are sums of like-signed terms, and |p| >= 0.1 stays far above the updates."""
    p0, gs = R.make_inputs(N, seed=11)
    sign = -1.0 if R.CASES[case][1].get("maximize") else 1.0
    p0 = (0.1 + np.abs(p0)).astype(np.float32)
    gs = [(sign * (1e-3 + np.abs(g))).astype(np.float32) for g in gs]
    _pin(case, p0, gs, lambda k, a, b: np.testing.assert_allclose(a, b, rtol=1e-12, atol=0, err_msg=k))


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_restatement_is_torch_in_fp64_with_cancellation(case):
    """The same on the inputs of the other tests, where m and buf do cancel: 1e-12 relative to the operands' magnitude
    (|g| <= 0.06 and |p| <= 0.5 there, so every operand of m, v and buf is below 0.1)."""
    p0, gs = R.make_inputs(N, seed=11)
    assert max(np.abs(g).max() for g in gs) <= 0.06 and np.abs(p0).max() <= 0.5
    _pin(case, p0, gs, lambda k, a, b: np.testing.assert_allclose(a, b, rtol=1e-12, atol=0 if k == "p" else 1e-13, err_msg=k))


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_torch_fp32_stays_inside_the_bound(case):
    """The bound of optim_restatement (a count of fp32 roundings on operand magnitudes) holds for torch's own fp32 CPU
    optimisers on the test inputs, after 1 and after 5 steps: a condition on bound and inputs, which the GPU tests then
    apply to the kernel unchanged."""
    kind, kw = R.CASES[case]
    p0, gs = R.make_inputs(N, seed=12)
    for steps in (1, 5):
        p, opt = _torch_run(kind, kw, p0, gs[:steps], torch.float32)
        run = R.make_run(kind, kw, p0)
        for g in gs[:steps]:
            run.step(g, R.LR)
        checks = [("p", p.detach().numpy(), run.p, run.Ep)]
        st = _state_arrays(kind, opt, p)
        if kind == "sgd":
            if "buf" in st:
                checks.append(("buf", st["buf"], run.buf, run.Eb))
        else:
            checks += [("m", st["m"], run.m, run.Em), ("v", st["v"], run.v, run.Ev)]
            if "vmax" in st:
                checks.append(("vmax", st["vmax"], run.vmax, run.Evmax))
        for name, got, want, bound in checks:
            ok, worst = R.within(got, want, bound)
            print(f"{case} steps={steps} {name}: worst |err| / bound = {worst:.3f}")
            assert ok, (case, steps, name, worst)
            # a rounding-error bound, not a tolerance: for the typical element a few dozen u of the operands' magnitude
            # (|p| ~ 0.1, |g| ~ 0.01); single elements exceed that where weight decay makes g' cancel in front of m / sqrt(v)
            assert np.median(bound) <= 64 * R.U * (0.1 if name == "p" else 0.01), (case, steps, name)


def test_bound_is_on_operands_not_on_the_result():
    """m cancels to 0 for g' = -b1 m / (1 - b1); the bound on it must not."""
    m = np.full(4, 0.25)
    run = R.AdamRun(np.ones(4), betas=(0.5, 0.999), m=m, v=np.ones(4), step=3)
    run.step(-m.astype(np.float32), 1e-3)
    assert (run.m == 0).all() and (run.Em >= 4 * R.U * 0.25).all()


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_state_dict_layout_is_torch(case):
    """Parameter groups and (for a state loaded from torch) per-parameter state carry torch's keys, dtypes and devices."""
    kind, kw = R.CASES[case]
    p0, gs = R.make_inputs(5, seed=1, steps=1)
    p, ref = _torch_run(kind, kw, p0, gs, torch.float32)
    q = torch.nn.Parameter(torch.from_numpy(p0).clone())
    ours = OURS[kind]([q], lr=R.LR, **kw)
    assert isinstance(ours, torch.optim.Optimizer) and isinstance(ours, TORCH[kind])
    a, b = ours.state_dict(), ref.state_dict()
    assert list(a["param_groups"][0]) == list(b["param_groups"][0])
    assert a["param_groups"][0] == b["param_groups"][0]
    ours.load_state_dict(b)
    a = ours.state_dict()
    assert a["param_groups"] == b["param_groups"] and a["state"].keys() == b["state"].keys()
    for k, v in b["state"].get(0, {}).items():
        w = a["state"][0][k]
        assert (w.dtype, w.device, w.shape) == (v.dtype, v.device, v.shape), k
        assert torch.equal(w, v), k
    ref2 = TORCH[kind]([p], lr=0.5)
    ref2.load_state_dict(a)                                   # and back
    assert ref2.state_dict()["param_groups"] == b["param_groups"]


@pytest.mark.parametrize("kind,kw", [
    ("adam", {"lr": -1.0}), ("adam", {"eps": -1.0}), ("adam", {"betas": (1.0, 0.9)}), ("adam", {"betas": (0.9, -0.1)}),
    ("adam", {"weight_decay": -1.0}), ("adam", {"betas": (0.9, 1)}), ("adamw", {"lr": -1.0}), ("adamw", {"betas": (0.9, 1.0)}),
    ("adamw", {"weight_decay": -0.5}), ("sgd", {"lr": -1.0}), ("sgd", {"momentum": -0.1}), ("sgd", {"weight_decay": -0.1}),
    ("sgd", {"nesterov": True}), ("sgd", {"nesterov": True, "momentum": 0.9, "dampening": 0.1}),
])
def test_constructor_validation_is_torch(kind, kw):
    p = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(Exception) as theirs:
        TORCH[kind]([p], **kw)
    with pytest.raises(type(theirs.value)) as ours:
        OURS[kind]([p], **kw)
    assert str(ours.value) == str(theirs.value)


def test_param_groups_and_defaults():
    a, b = torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2))
    opt = DO.Adam([{"params": [a]}, {"params": [b], "lr": 1e-5, "weight_decay": 0.1}], lr=1e-4)
    assert [g["lr"] for g in opt.param_groups] == [1e-4, 1e-5] and [g["weight_decay"] for g in opt.param_groups] == [0, 0.1]
    ref = torch.optim.Adam([a])
    assert {k: v for k, v in DO.Adam([a]).param_groups[0].items() if k != "params"} == \
        {k: v for k, v in ref.param_groups[0].items() if k != "params"}
    import dram_amd
    assert dram_amd.Adam is DO.Adam and dram_amd.AdamW is DO.AdamW and dram_amd.SGD is DO.SGD
    assert DO.TABLE_CAPACITY >= 1


def test_rejections_name_the_reason():
    p = torch.nn.Parameter(torch.zeros(3))
    for cls in (DO.Adam, DO.AdamW, DO.SGD):
        with pytest.raises(TypeError, match="lr must be a Python number"):
            cls([p], lr=torch.tensor(1e-3))
        opt = cls([p], lr=1e-3)
        p.grad = torch.zeros(3)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            opt.step()
        assert len(opt.state[p]) == 0                        # nothing was touched
        opt.param_groups[0]["lr"] = torch.tensor(1e-3)
        with pytest.raises(TypeError, match="lr must be a Python number"):
            opt.step()
        p.grad = None
        opt.param_groups[0]["lr"] = 1e-3
        opt.step()                                            # no gradient anywhere: nothing to do, nothing raised


def test_table_errors_are_reported_without_a_gpu():
    from dram_amd import _lib
    with pytest.raises(_lib.DramHipError, match="tensors in one table"):
        _lib.call("dram_optim_adam", b"\0" * 56, DO.TABLE_CAPACITY + 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 0, 0, None)
    with pytest.raises(_lib.DramHipError, match="null pointer"):
        _lib.call("dram_optim_sgd", b"\0" * 56, 1, 1e-3, 0.9, 0.0, 0.0, 0, 0, None)
    row = DO._ENTRY.pack(16, 16, 16, 16, 0, 0, 1.0, 1.0)
    with pytest.raises(_lib.DramHipError, match="element count"):
        _lib.call("dram_optim_adam", row, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 0, 0, None)
    row = DO._ENTRY.pack(16, 16, 16, 16, 0, 4, 1.0, 1.0)
    with pytest.raises(_lib.DramHipError, match="max-second-moment"):
        _lib.call("dram_optim_adam", row, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 1, 0, None)
