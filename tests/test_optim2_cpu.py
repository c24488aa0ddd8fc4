"""The RAdam and AdaBound restatements (tests/optim2_restatement.py) against their pins on the CPU, the fp32 error bound
against fp32 runs of the pins, and the host side of dram_amd.optim.RAdam / AdaBound.  No kernel runs.

RAdam is pinned by torch.optim.RAdam.  AdaBound is pinned by the `adabound` package where it can be imported; it is not a
dependency of this project, and where it is missing THE DEFINITION in optim2_restatement's docstring is the pin: `_Transcript`
below is that definition as plain torch operations, in the order of the package's 0.0.5 step(), and stands in for it."""
import math

import numpy as np
import pytest
import torch

import optim2_restatement as R
import optim_restatement as R1
from dram_amd import optim as DO

try:
    from adabound import AdaBound as _PackageAdaBound
except ImportError:
    _PackageAdaBound = None

N = 4099


class _Transcript(torch.optim.Optimizer):
    """AdaBound as the definition states it, one plain torch operation per term, in the dtype of the parameter."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), final_lr=0.1, gamma=1e-3, eps=1e-8, weight_decay=0, amsbound=False):
        super().__init__(params, dict(lr=lr, betas=betas, final_lr=final_lr, gamma=gamma, eps=eps, weight_decay=weight_decay,
                                      amsbound=amsbound))
        self.base_lrs = [g["lr"] for g in self.param_groups]

    @torch.no_grad()
    def step(self):
        for group, base_lr in zip(self.param_groups, self.base_lrs):
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(p), torch.zeros_like(p)
                    if group["amsbound"]:
                        st["max_exp_avg_sq"] = torch.zeros_like(p)
                st["step"] += 1
                t = st["step"]
                g = p.grad
                if group["weight_decay"] != 0:
                    g = g.add(p, alpha=group["weight_decay"])
                st["exp_avg"].mul_(b1).add_(g, alpha=1 - b1)
                st["exp_avg_sq"].mul_(b2).addcmul_(g, g, value=1 - b2)
                vuse = st["exp_avg_sq"]
                if group["amsbound"]:
                    torch.maximum(st["max_exp_avg_sq"], st["exp_avg_sq"], out=st["max_exp_avg_sq"])
                    vuse = st["max_exp_avg_sq"]
                den = vuse.sqrt().add_(group["eps"])
                step_size = group["lr"] * math.sqrt(1 - b2 ** t) / (1 - b1 ** t)
                final = group["final_lr"] * group["lr"] / base_lr
                lower = final * (1 - 1 / (group["gamma"] * t + 1))
                upper = final * (1 + 1 / (group["gamma"] * t))
                rate = torch.full_like(den, step_size).div_(den).clamp_(lower, upper)
                p.add_(-(rate * st["exp_avg"]))


ADABOUND_PIN = _PackageAdaBound or _Transcript
TORCH = {"radam": torch.optim.RAdam, "adabound": ADABOUND_PIN}
OURS = {"radam": DO.RAdam, "adabound": DO.AdaBound}


def _pin_run(kind, kw, p0, gs, dtype, lr=None, skip=(), state=None, lrs=None):
    p = torch.nn.Parameter(torch.from_numpy(p0).to(dtype, copy=True))
    opt = TORCH[kind]([p], lr=R.LR[kind] if lr is None else lr, **kw)
    if state is not None:
        opt.state[p] = {"step": torch.tensor(float(state["step"])), "exp_avg": torch.from_numpy(state["m"]).to(dtype, copy=True),
                        "exp_avg_sq": torch.from_numpy(state["v"]).to(dtype, copy=True)}
    for i, g in enumerate(gs):
        if lrs is not None:
            opt.param_groups[0]["lr"] = lrs[i]
        p.grad = None if i in skip else torch.from_numpy(g).to(dtype)
        opt.step()
    return p, opt


def _state_arrays(opt, p):
    st = opt.state[p]
    out = {"m": st["exp_avg"].numpy(), "v": st["exp_avg_sq"].numpy()}
    if "max_exp_avg_sq" in st:
        out["vmax"] = st["max_exp_avg_sq"].numpy()
    return out


def _like_signed(case, p0, gs):
    """Parameters >= 0.1 and gradients that (after maximize) have their sign, kept away from 0: nothing cancels."""
    sign = -1.0 if R.CASES[case][1].get("maximize") else 1.0
    return (0.1 + np.abs(p0)).astype(np.float32), [(sign * (1e-3 + np.abs(g))).astype(np.float32) for g in gs]


def _pin(case, p0, gs, check):
    kind, kw = R.CASES[case]
    p, opt = _pin_run(kind, kw, p0, gs, torch.float64, skip=(2,))
    run = R.make_run(kind, kw, p0)
    for i, g in enumerate(gs):
        run.step(None if i == 2 else g, R.LR[kind])
    check("p", p.detach().numpy(), run.p)
    for k, a in _state_arrays(opt, p).items():
        check(k, a, getattr(run, k))
    assert float(opt.state[p]["step"]) == run.t == R.STEPS - 1
    return run


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_restatement_is_its_pin_in_fp64(case):
    """8 steps (the third without a gradient) of the pin in fp64 on the CPU: the restatement agrees to 1e-12 relative, element
    by element, on inputs where nothing cancels (see test_optim_cpu.test_restatement_is_torch_in_fp64).  RAdam's runs cross
    the rectification switch: both branches occur."""
    kind = R.CASES[case][0]
    p0, gs = _like_signed(case, *R.inputs(kind, N, seed=11))
    run = _pin(case, p0, gs, lambda k, a, b: np.testing.assert_allclose(a, b, rtol=1e-12, atol=0, err_msg=k))
    if kind == "radam":
        assert run.rectified[0] is False and run.rectified[-1] is True, run.rectified


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_restatement_is_its_pin_in_fp64_with_cancellation(case):
    """The same on the inputs of the other tests, where m does cancel: 1e-12 relative to the operands' magnitude (RAdam:
    |g| <= 0.06, |p| <= 0.5; AdaBound: |g| <= 16 and rates <= 0.6, so every operand is below 16)."""
    kind = R.CASES[case][0]
    p0, gs = R.inputs(kind, N, seed=11)
    top = max(np.abs(g).max() for g in gs)
    assert top <= (0.06 if kind == "radam" else 16.0) and np.abs(p0).max() <= 0.5
    scale = 0.1 if kind == "radam" else 16.0
    _pin(case, p0, gs, lambda k, a, b: np.testing.assert_allclose(
        a, b, rtol=1e-12, atol=1e-12 * scale * (scale if k in ("v", "vmax") else 1.0), err_msg=k))


def test_radam_switches_at_step_6_with_the_default_betas():
    assert [R.rectification(t, 0.999)[1] is not None for t in range(1, 9)] == [False] * 5 + [True] * 3
    rho, rect = R.rectification(6, 0.999)
    assert 5.0 < rho < 6.0 and 0.0 < rect < 1.0
    assert [R.rectification(t, 0.95)[1] is not None for t in (5, 6)] == [False, True]


def _check_fp32(case, what, p, opt, run):
    checks = [("p", p.detach().numpy(), run.p, run.Ep)]
    st = _state_arrays(opt, p)
    checks += [("m", st["m"], run.m, run.Em), ("v", st["v"], run.v, run.Ev)]
    if "vmax" in st:
        checks.append(("vmax", st["vmax"], run.vmax, run.Evmax))
    for name, got, want, bound in checks:
        ok, worst = R.within(got, want, bound)
        print(f"{case} {what} {name}: worst |err| / bound = {worst:.3f}")
        assert ok, (case, what, name, worst)


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_fp32_pin_stays_inside_the_bound(case):
    """The bound of optim2_restatement holds for the pin's own fp32 CPU run on the test inputs after 1, 5 (RAdam: the last
    unrectified step) and 8 steps: a condition on bound and inputs, which the GPU tests then apply to the kernel unchanged."""
    kind, kw = R.CASES[case]
    p0, gs = R.inputs(kind, N, seed=12)
    for steps in (1, 5, R.STEPS):
        p, opt = _pin_run(kind, kw, p0, gs[:steps], torch.float32)
        run = R.make_run(kind, kw, p0)
        for g in gs[:steps]:
            run.step(g, R.LR[kind])
        _check_fp32(case, f"steps={steps}", p, opt, run)
        if kind == "radam":
            # a rounding-error bound, not a tolerance (the figure test_optim_cpu holds Adam's to)
            assert np.median(run.Ep) <= 64 * R.U * 0.1 and np.median(run.Em) <= 64 * R.U * 0.01, (case, steps)
            assert run.rectified[-1] == (steps > 5)
        else:
            # relative to what the step touches: the parameter and the update, whose rate the upper bound caps
            assert np.median(run.Ep) <= 64 * R.U * (0.1 + np.median(np.abs(run.p - p0))), (case, steps)


def test_radam_from_a_loaded_state_with_step_100():
    """exp_avg, exp_avg_sq and step = 100 loaded, then 3 steps: rectified from the first (rho_t ~ 86), fp64 to 1e-12 on
    like-signed inputs and fp32 within the bound."""
    rng = np.random.default_rng(13)
    p0, gs = _like_signed("radam", *R.inputs("radam", N, seed=14, steps=3))
    state = {"step": 100, "m": (0.01 * (0.5 + rng.random(N))).astype(np.float32), "v": (1e-4 * (0.5 + rng.random(N))).astype(np.float32)}
    runs = {}
    for dtype in (torch.float64, torch.float32):
        p, opt = _pin_run("radam", {}, p0, gs, dtype, state=state)
        run = R.RAdamRun(p0, m=state["m"], v=state["v"], step=100)
        for g in gs:
            run.step(g, R.LR["radam"])
        assert float(opt.state[p]["step"]) == run.t == 103 and run.rectified == [True] * 3
        if dtype == torch.float64:
            np.testing.assert_allclose(p.detach().numpy(), run.p, rtol=1e-12, atol=0)
            np.testing.assert_allclose(opt.state[p]["exp_avg_sq"].numpy(), run.v, rtol=1e-12, atol=0)
        else:
            _check_fp32("radam", "step=100", p, opt, run)
        runs[dtype] = run
    # the loaded step count matters at this bound: the same three steps from step 0 are far outside it
    fresh = R.RAdamRun(p0, m=state["m"], v=state["v"])
    for g in gs:
        fresh.step(g, R.LR["radam"])
    assert not R.within(fresh.p, runs[torch.float32].p, runs[torch.float32].Ep)[0]


@pytest.mark.parametrize("case", ["adabound", "adabound_wd", "adabound_amsbound", "adabound_betas_eps", "adabound_all"])
def test_adabound_inputs_reach_all_three_regimes(case):
    """At some step at least 10 % of the elements are clamped at lower, at some step 10 % at upper and at some step 10 % are
    unclamped -- on the restatement, for the inputs and sizes the CPU and the GPU tests use."""
    kind, kw = R.CASES[case]
    for n, seed in ((N, 12), (1025, 3001), (65536 + 7, 3007), (864, 3008)):
        p0, gs = R.inputs(kind, n, seed=seed)
        run = R.make_run(kind, kw, p0)
        for g in gs:
            run.step(g, R.LR[kind])
        best = [max(f[k] for f in run.regimes) for k in range(3)]
        print(f"{case} n={n}: largest fraction at lower {best[0]:.2f}, unclamped {best[1]:.2f}, at upper {best[2]:.2f}; "
              f"step 1: {run.regimes[0]}")
        assert min(best) >= 0.10, (case, n, best)


def test_adabound_whose_bounds_do_not_bind_is_adam_without_eps():
    """eps = 0, gamma = 1e-12 (lower ~ 1e-13, upper ~ 1e11) and gradients that are nowhere zero: no element is clamped and the
    update is Adam's with eps = 0.  In fp64 the restatement agrees with torch.optim.Adam to 1e-12; torch's fp32 Adam lies
    within the AdaBound bound plus the Adam bound of the restatement (each run is within its own bound of the same fp64
    values), and the fp32 AdaBound pin within the AdaBound bound alone."""
    kw = {"eps": 0.0, "gamma": 1e-12}
    lr = R.LR["adabound"]
    p0, gs = R.inputs("adabound", N, seed=15, steps=5)
    gs = [np.where(g == 0, np.float32(1e-3), g) for g in gs]
    run, adam = R.AdaBoundRun(p0, lr, **kw), R1.AdamRun(p0, eps=0.0)
    for g in gs:
        run.step(g, lr)
        adam.step(g, lr)
    assert all(f == (0.0, 1.0, 0.0) for f in run.regimes), run.regimes
    ref = torch.nn.Parameter(torch.from_numpy(p0).double())
    opt = torch.optim.Adam([ref], lr=lr, eps=0.0)
    for g in gs:
        ref.grad = torch.from_numpy(g).double()
        opt.step()
    np.testing.assert_allclose(ref.detach().numpy(), run.p, rtol=1e-12, atol=1e-13)
    ref = torch.nn.Parameter(torch.from_numpy(p0).clone())
    opt = torch.optim.Adam([ref], lr=lr, eps=0.0)
    for g in gs:
        ref.grad = torch.from_numpy(g)
        opt.step()
    d = np.abs(ref.detach().numpy().astype(np.float64) - run.p)
    print(f"torch.optim.Adam(eps=0) fp32 against the AdaBound restatement: worst |err| / (bound + Adam's bound) = "
          f"{(d / (run.Ep + adam.Ep)).max():.3f}")
    assert (d <= run.Ep + adam.Ep).all()
    p, o = _pin_run("adabound", kw, p0, gs, torch.float32)
    _check_fp32("adabound", "unbound", p, o, run)
    assert np.median(run.Ep) <= 64 * R.U * 0.1


def test_adabound_bounds_scale_with_the_schedule():
    """final = final_lr * lr / base_lr: under ExponentialLR(gamma=0.9) stepped after every update both bounds are 0.9^k times
    those of the constant-lr run at the same step, in the restatement and in the pin (fp64, 1e-12)."""
    kind, kw = R.CASES["adabound"]
    lr0 = R.LR[kind]
    p0, gs = _like_signed("adabound", *R.inputs(kind, N, seed=16, steps=4))
    lrs = [lr0 * 0.9 ** k for k in range(4)]
    sched, const = R.make_run(kind, kw, p0), R.make_run(kind, kw, p0)
    for g, lr in zip(gs, lrs):
        sched.step(g, lr)
        const.step(g, lr0)
    for k in range(4):
        for a, b in zip(sched.bounds[k], const.bounds[k]):
            assert a == pytest.approx(b * 0.9 ** k, rel=1e-14)
    p, opt = _pin_run(kind, kw, p0, gs, torch.float64, lrs=lrs)
    assert opt.base_lrs == [lr0]
    np.testing.assert_allclose(p.detach().numpy(), sched.p, rtol=1e-12, atol=0)
    assert not np.allclose(sched.p, const.p, rtol=1e-6, atol=0)
    # the class under test keeps the construction-time rate beside a scheduler that rewrites param_groups
    q = torch.nn.Parameter(torch.zeros(3))
    ours = DO.AdaBound([{"params": [q]}, {"params": [torch.nn.Parameter(torch.zeros(2))], "lr": 5e-4}], lr=lr0, final_lr=0.01)
    s = torch.optim.lr_scheduler.ExponentialLR(ours, gamma=0.9)
    ours.step()
    s.step()
    assert ours.base_lrs == [lr0, 5e-4]
    assert [g["lr"] for g in ours.param_groups] == pytest.approx([0.9 * lr0, 0.9 * 5e-4], rel=1e-12)
    assert "base_lrs" not in ours.state_dict() and "base_lrs" not in ours.state_dict()["param_groups"][0]
    ours.add_param_group({"params": [torch.nn.Parameter(torch.zeros(1))], "lr": 2e-3})
    assert ours.base_lrs == [lr0, 5e-4, 2e-3]


@pytest.mark.parametrize("case", sorted(R.RADAM_CASES))
def test_radam_state_dict_layout_is_torch(case):
    """Parameter groups and per-parameter state carry torch's keys, dtypes and devices; torch's checkpoint loads into ours and
    ours into torch's."""
    kind, kw = R.CASES[case]
    p0, gs = R.inputs(kind, 5, seed=1, steps=1)
    p, ref = _pin_run(kind, kw, p0, gs, torch.float32)
    q = torch.nn.Parameter(torch.from_numpy(p0).clone())
    ours = DO.RAdam([q], lr=R.LR[kind], **kw)
    assert isinstance(ours, torch.optim.RAdam)
    a, b = ours.state_dict(), ref.state_dict()
    assert list(a["param_groups"][0]) == list(b["param_groups"][0])
    assert a["param_groups"][0] == b["param_groups"][0]
    ours.load_state_dict(b)
    a = ours.state_dict()
    assert a["param_groups"] == b["param_groups"] and a["state"].keys() == b["state"].keys()
    assert sorted(a["state"][0]) == ["exp_avg", "exp_avg_sq", "step"]
    for k, v in b["state"][0].items():
        w = a["state"][0][k]
        assert (w.dtype, w.device, w.shape) == (v.dtype, v.device, v.shape), k
        assert torch.equal(w, v), k
    ref2 = torch.optim.RAdam([p], lr=0.5)
    ref2.load_state_dict(a)                                   # and back
    assert ref2.state_dict()["param_groups"] == b["param_groups"]
    assert torch.equal(ref2.state[p]["exp_avg_sq"], ref.state[p]["exp_avg_sq"]) and float(ref2.state[p]["step"]) == 1.0


def test_adabound_state_dict_round_trip():
    """A checkpoint as the package writes it (step a Python int) loads into ours, whose step() takes the int over as the host
    fp32 scalar; ours loads into the pin and into a second one of ours."""
    kind, kw = R.CASES["adabound_amsbound"]
    p0, gs = R.inputs(kind, 5, seed=2, steps=2)
    p, ref = _pin_run(kind, kw, p0, gs, torch.float32)
    b = ref.state_dict()
    assert b["state"][0]["step"] == 2
    q = torch.nn.Parameter(torch.from_numpy(p0).clone())
    ours = DO.AdaBound([q], lr=0.5, gamma=0.1)
    assert list(ours.state_dict()["param_groups"][0]) == ["lr", "betas", "final_lr", "gamma", "eps", "weight_decay", "amsbound",
                                                          "params"]
    ours.load_state_dict(b)
    g0 = ours.param_groups[0]
    assert (g0["lr"], g0["gamma"], g0["amsbound"], g0["final_lr"]) == (R.LR[kind], 0.5, True, 0.1)
    assert ours.base_lrs == [0.5]                             # an attribute of the object, not of the checkpoint
    st = ours.state[q]
    assert sorted(st) == ["exp_avg", "exp_avg_sq", "max_exp_avg_sq", "step"]
    for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
        assert torch.equal(st[k], ref.state[p][k]) and st[k].dtype == torch.float32
    step = DO._host_step(st, "test")
    assert torch.is_tensor(step) and step.dtype == torch.float32 and step.device.type == "cpu" and float(step) == 2.0
    assert st["step"] is step
    a = ours.state_dict()
    back = ADABOUND_PIN([p], lr=0.25)
    back.load_state_dict(a)
    assert float(back.state[p]["step"]) == 2.0 and torch.equal(back.state[p]["max_exp_avg_sq"], ref.state[p]["max_exp_avg_sq"])
    again = DO.AdaBound([torch.nn.Parameter(torch.zeros(5))])
    again.load_state_dict(a)
    assert again.state_dict()["param_groups"] == a["param_groups"]
    old = {"state": {}, "param_groups": [{k: v for k, v in a["param_groups"][0].items() if k != "amsbound"}]}
    again.load_state_dict(old)                               # a checkpoint from before amsbound existed
    assert again.param_groups[0]["amsbound"] is False


@pytest.mark.parametrize("kw", [{"lr": -1.0}, {"eps": -1.0}, {"betas": (1.0, 0.9)}, {"betas": (0.9, -0.1)}, {"betas": (0.9, 1)},
                                {"weight_decay": -1.0}])
def test_radam_constructor_validation_is_torch(kw):
    p = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(ValueError) as theirs:
        torch.optim.RAdam([p], **kw)
    with pytest.raises(ValueError) as ours:
        DO.RAdam([p], **kw)
    assert str(ours.value) == str(theirs.value)


@pytest.mark.parametrize("kw,word", [({"lr": -1.0}, "learning rate"), ({"eps": -1.0}, "epsilon"), ({"betas": (1.0, 0.9)}, "index 0"),
                                     ({"betas": (-0.1, 0.9)}, "index 0"), ({"betas": (0.9, 1.0)}, "index 1"),
                                     ({"betas": (0.9, -0.5)}, "index 1"), ({"final_lr": -0.1}, "final learning rate"),
                                     ({"gamma": 1.0}, "gamma"), ({"gamma": -0.1}, "gamma")])
def test_adabound_constructor_validation(kw, word):
    p = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(ValueError, match=word):
        DO.AdaBound([p], **kw)
    if _PackageAdaBound is not None:
        with pytest.raises(ValueError):
            _PackageAdaBound([p], **kw)


def test_defaults_and_export():
    import dram_amd
    assert dram_amd.RAdam is DO.RAdam and dram_amd.AdaBound is DO.AdaBound
    assert {"RAdam", "AdaBound"} <= set(dram_amd.__all__) and {"RAdam", "AdaBound"} <= set(DO.__all__)
    a = torch.nn.Parameter(torch.zeros(3))
    assert {k: v for k, v in DO.RAdam([a]).param_groups[0].items() if k != "params"} == \
        {k: v for k, v in torch.optim.RAdam([a]).param_groups[0].items() if k != "params"}
    assert {k: v for k, v in DO.AdaBound([a]).param_groups[0].items() if k != "params"} == \
        {"lr": 1e-3, "betas": (0.9, 0.999), "final_lr": 0.1, "gamma": 1e-3, "eps": 1e-8, "weight_decay": 0, "amsbound": False}
    # the two settings of the reference's OPTIMIZER block
    opt = DO.AdaBound([a], lr=0.0001, final_lr=0.01)
    assert opt.base_lrs == [0.0001] and opt.param_groups[0]["final_lr"] == 0.01
    assert DO.RAdam([a], lr=0.0001).param_groups[0]["lr"] == 0.0001
    for cls in (DO.RAdam, DO.AdaBound):
        assert issubclass(cls, torch.optim.Optimizer) and callable(cls([a]).set_grad_clip)
        opt = cls([a])
        assert opt._clip is None and opt.last_grad_norm is None and opt.last_clip_coef is None
        opt.set_grad_clip(1.0, math.inf)
        assert opt._clip == (1.0, 0) and "_clip" not in opt.state_dict()


def test_rejections_name_the_reason():
    p = torch.nn.Parameter(torch.zeros(3))
    for cls in (DO.RAdam, DO.AdaBound):
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
    for entry, scalars in (("dram_optim_radam", (1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 0)),
                           ("dram_optim_adabound", (0.9, 0.999, 1e-8, 0.0, 0, 0.01, 0.2))):
        for suffix, tail in (("", (None,)), ("_scaled", (None, None))):
            with pytest.raises(_lib.DramHipError, match="tensors in one table"):
                _lib.call(entry + suffix, b"\0" * 56, DO.TABLE_CAPACITY + 1, *scalars, *tail)
            with pytest.raises(_lib.DramHipError, match="null pointer"):
                _lib.call(entry + suffix, b"\0" * 56, 1, *scalars, *tail)
            row = DO._ENTRY.pack(16, 16, 16, 0, 0, 4, 1.0, 1.0)
            with pytest.raises(_lib.DramHipError, match="second-moment"):
                _lib.call(entry + suffix, row, 1, *scalars, *tail)
            row = DO._ENTRY.pack(16, 16, 16, 16, 0, 0, 1.0, 1.0)
            with pytest.raises(_lib.DramHipError, match="element count"):
                _lib.call(entry + suffix, row, 1, *scalars, *tail)
    row = DO._ENTRY.pack(16, 16, 16, 16, 0, 4, 1.0, 0.0)
    with pytest.raises(_lib.DramHipError, match="max-second-moment"):
        _lib.call("dram_optim_adabound", row, 1, 0.9, 0.999, 1e-8, 0.0, 1, 0.01, 0.2, None)
    with pytest.raises(_lib.DramHipError, match="above upper bound"):
        _lib.call("dram_optim_adabound", row, 1, 0.9, 0.999, 1e-8, 0.0, 0, 0.3, 0.2, None)
    with pytest.raises(_lib.DramHipError, match="gscale not 4-byte aligned"):
        _lib.call("dram_optim_radam_scaled", row, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 0, 2, None)
