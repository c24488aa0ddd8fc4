"""dram_amd.optim.RAdam and AdaBound (csrc/optim.hip) on the device against the fp64 restatement of
tests/optim2_restatement.py, under the rounding-error bound that tests/test_optim2_cpu.py holds the fp32 CPU runs of their pins
to; the clipped step bit for bit against clip-then-step; one DataParallelTrainer step with each.

AdaBound's pin is the definition in optim2_restatement's docstring (the `adabound` package is not a dependency of this
project; where it can be imported the CPU test holds the restatement against it)."""
import math

import numpy as np
import pytest
import torch

import optim2_restatement as R
from test_gpu_optim import SHAPES, Layout, _bits

pytestmark = pytest.mark.gpu

DEV = "cuda"
CHECK_AT = (1, 5, 6, R.STEPS)                # RAdam's default betas: step 5 is the last unrectified one, step 6 the first rectified
STATE_KEYS = (("m", "exp_avg"), ("v", "exp_avg_sq"), ("vmax", "max_exp_avg_sq"))
NONE_AT = {2: tuple(range(R.STEPS)), 6: (2,)}     # tensor 2 never has a gradient; tensor 6 misses the third step


def _do():
    from dram_amd import optim as DO
    return DO


def _cls(kind):
    DO = _do()
    return {"radam": DO.RAdam, "adabound": DO.AdaBound}[kind]


class Harness:
    """test_gpu_optim.Harness for the two optimisers of this file: `shapes` tensors under one optimiser of ours, every quantity
    (p, g, m, v, vmax) laid out as `layouts` says (a name, or a dict per quantity), one restatement run per tensor.  Tensor i
    gets no gradient at the steps listed in none_at.get(i, ())."""

    def __init__(self, kind, kw, shapes, layouts, seed, groups=None, state=None, none_at=None):
        rng = np.random.default_rng(seed)
        self.kind, self.kw, self.shapes = kind, kw, shapes
        self.none_at = none_at or {}
        groups = groups or [(list(range(len(shapes))), {})]
        hyper = {i: over for idx, over in groups for i in idx}
        names = ["p", "g", "m", "v"] + (["vmax"] if any(dict(kw, **h).get("amsbound") for h in hyper.values()) else [])
        if not isinstance(layouts, dict):
            layouts = {q: layouts for q in names}
        self.q = {q: Layout(shapes, layouts.get(q, "separate"), rng, DEV) for q in names}
        self.inputs = [R.inputs(kind, int(np.prod(s)), seed=seed * 1000 + i) for i, s in enumerate(shapes)]
        self.params = []
        for i in range(len(shapes)):
            if self.inputs[i][0].size:
                self.q["p"].set(i, self.inputs[i][0])
            self.params.append(self.q["p"].views[i].requires_grad_())
        self.opt = _cls(kind)([{"params": [self.params[i] for i in idx], **over} for idx, over in groups], lr=R.LR[kind], **kw)
        self.runs = []
        for i in range(len(shapes)):
            h = dict(kw)
            h.update({k: v for k, v in hyper[i].items() if k != "lr"})
            st = {} if state is None else state[i]
            if not h.get("amsbound"):
                st = {k: v for k, v in st.items() if k != "vmax"}
            self.runs.append(R.make_run(kind, h, self.inputs[i][0], base_lr=hyper[i].get("lr"), **st))
            if state is not None or layouts.get("m", "separate") != "separate":
                s = {"step": torch.tensor(float(st.get("step", 0)), dtype=torch.float32)}
                for q, key in STATE_KEYS:
                    if q in self.q and (q != "vmax" or h.get("amsbound")):
                        self.q[q].set(i, st.get(q, np.zeros(shapes[i])))
                        s[key] = self.q[q].views[i]
                self.opt.state[self.params[i]] = s
        self.k = 0

    def lr(self, p):
        return next(gr["lr"] for gr in self.opt.param_groups if any(p is q for q in gr["params"]))

    def step(self):
        for i, p in enumerate(self.params):
            g = None if self.k in self.none_at.get(i, ()) else self.inputs[i][1][self.k]
            if g is None:
                p.grad = None
            else:
                if g.size:
                    self.q["g"].set(i, g)
                p.grad = self.q["g"].views[i]
            self.runs[i].step(g, self.lr(p))
        self.opt.step()
        self.k += 1

    def check(self, what=""):
        torch.cuda.synchronize()
        worst = {}
        for i, (p, run) in enumerate(zip(self.params, self.runs)):
            got = [("p", p.detach(), run.p, run.Ep)]
            st = self.opt.state.get(p, {})
            if run.t == 0 and "step" not in st:
                assert len(st) == 0
            else:
                assert float(st["step"]) == run.t, (what, i, float(st["step"]), run.t)
                assert st["step"].device.type == "cpu" and st["step"].dtype == torch.float32
                got += [("m", st["exp_avg"], run.m, run.Em), ("v", st["exp_avg_sq"], run.v, run.Ev)]
                if run.vmax is not None:
                    got.append(("vmax", st["max_exp_avg_sq"], run.vmax, run.Evmax))
                else:
                    assert "max_exp_avg_sq" not in st
            for name, t, want, bound in got:
                ok, w = R.within(t.cpu().numpy().reshape(-1), want.reshape(-1), bound.reshape(-1))
                worst[name] = max(worst.get(name, 0.0), w)
                assert ok, f"{what}: tensor {i} {tuple(self.shapes[i])} {name}: |err| / bound = {w:.3f}"
        for q, lay in self.q.items():
            assert lay.guards_untouched(), f"{what}: elements outside the {q} views changed"
        print(f"{what} after {self.k} steps: worst |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))

    def run(self, what, steps=R.STEPS, check_at=CHECK_AT):
        for _ in range(steps):
            self.step()
            if self.k in check_at:
                self.check(what)
        return self


def _count_calls(monkeypatch):
    DO = _do()
    seen, real = [], DO.call
    monkeypatch.setattr(DO, "call", lambda name, *a: (seen.append((name, a)), real(name, *a))[1])
    return seen


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_every_option_on_separate_tensors(case, monkeypatch):
    """Every size (aligned: the 16-byte instantiation plus the scalar tail), every option combination, after 1, 5, 6 and 8
    steps: RAdam crosses its switch between the two middle checks.  One parameter never has a gradient (untouched, no state)
    and one misses a step: its step count stays behind, which for RAdam is an unrectified tensor beside rectified ones in one
    launch (step 6) and for AdaBound a second launch per step, the bounds being launch scalars."""
    kind, kw = R.CASES[case]
    seen = _count_calls(monkeypatch)
    h = Harness(kind, kw, SHAPES, "separate", seed=3, none_at=NONE_AT).run(case)
    assert np.array_equal(_bits(h.params[2].detach().cpu().numpy().reshape(-1)), _bits(h.inputs[2][0]))
    assert len(h.opt.state.get(h.params[2], {})) == 0
    assert [float(h.opt.state[p]["step"]) for p in (h.params[0], h.params[6])] == [8.0, 7.0]
    names = [n for n, _ in seen]
    assert set(names) == {f"dram_optim_{kind}"}
    # steps 1, 2: one step count; step 3: tensor 6 has no gradient; steps 4 .. 8: two step counts
    assert len(names) == (R.STEPS if kind == "radam" else 3 + 2 * 5)
    if kind == "radam":
        assert h.runs[0].rectified == [False] * 5 + [True] * 3 and h.runs[6].rectified == [False] * 5 + [True] * 2
    else:
        best = [max(f[k] for f in h.runs[7].regimes) for k in range(3)]
        assert min(best) >= 0.10 or "default_gamma" in case, best


@pytest.mark.parametrize("layout", ["off1", "off2", "off3"])
@pytest.mark.parametrize("case", ["radam", "radam_all", "radam_decoupled", "adabound", "adabound_all"])
def test_views_into_flat_buffers(case, layout):
    """p, g, m, v, vmax as views 1, 2 and 3 elements past a 16-byte boundary (the one-dword instantiation), guard elements
    around every view bit-unchanged."""
    kind, kw = R.CASES[case]
    Harness(kind, kw, SHAPES, layout, seed=4, none_at=NONE_AT).run(f"{case}/{layout}", check_at=(1, 6, R.STEPS))


@pytest.mark.parametrize("case", ["radam", "adabound_amsbound"])
def test_packed_gradient_bucket(case):
    """The trainer's case: parameters and state in their own allocations, gradients back to back in one flat bucket, so one
    launch holds aligned and misaligned tensors; and the same with the state guarded in aligned flat buffers."""
    kind, kw = R.CASES[case]
    Harness(kind, kw, SHAPES, {"g": "packed"}, seed=5).run(f"{case}/bucket", check_at=(1, 6, R.STEPS))
    Harness(kind, kw, SHAPES, {"g": "packed", "p": "off0", "m": "off0", "v": "off0", "vmax": "off0"}, seed=6).run(
        f"{case}/bucket+guards", check_at=(6, R.STEPS))


@pytest.mark.parametrize("case", ["radam_wd", "adabound_wd"])
def test_group_longer_than_one_table_with_an_empty_tensor(case, monkeypatch):
    """TABLE_CAPACITY + 2 tensors of 1 to 7 elements and one of none in one group: two launches per step; the empty one keeps
    its (empty) state and advances its step count, as under torch."""
    DO = _do()
    kind, kw = R.CASES[case]
    shapes = [(1 + i % 7,) for i in range(DO.TABLE_CAPACITY + 2)]
    shapes[10] = (0,)
    seen = _count_calls(monkeypatch)
    h = Harness(kind, kw, shapes, "packed", seed=7).run(case, steps=6, check_at=(1, 6))
    assert [a[1] for _, a in seen] == [DO.TABLE_CAPACITY, 1] * 6
    assert float(h.opt.state[h.params[10]]["step"]) == 6.0 and h.opt.state[h.params[10]]["exp_avg"].numel() == 0


@pytest.mark.parametrize("case", ["radam", "adabound_amsbound"])
def test_loaded_state_with_differing_step_counts(case, monkeypatch):
    """Nine tensors at nine step counts (0 .. 1000) in one group.  RAdam: rectified and unrectified tensors share a launch, and
    those loaded at 1 and 3 cross the switch during the run.  AdaBound: one launch per step count."""
    kind, kw = R.CASES[case]
    rng = np.random.default_rng(9)
    steps0 = (0, 1, 7, 100, 3, 2, 1000, 12, 5)
    state = []
    for i, s in enumerate(SHAPES):
        n = int(np.prod(s))
        scale = 1e-4 if kind == "radam" else 1e-2
        v = (scale * rng.random(n)).astype(np.float32)
        state.append({"step": steps0[i], "m": (math.sqrt(scale) * rng.standard_normal(n)).astype(np.float32), "v": v,
                      "vmax": (v * (1 + rng.random(n))).astype(np.float32)})
    seen = _count_calls(monkeypatch)
    h = Harness(kind, kw, SHAPES, "off1", seed=10, state=state).run(f"{case} loaded state", steps=5, check_at=(1, 3, 5))
    assert [float(h.opt.state[p]["step"]) for p in h.params] == [s + 5.0 for s in steps0]
    assert len(seen) == (5 if kind == "radam" else 5 * len(set(steps0)))
    if kind == "radam":
        assert h.runs[1].rectified == [False] * 4 + [True] and h.runs[4].rectified == [False, False, True, True, True]
        assert h.runs[3].rectified == [True] * 5 and h.runs[0].rectified == [False] * 5


def test_two_groups_with_their_own_hyper_parameters():
    idx = list(range(len(SHAPES)))
    groups = [(idx[::2], {}), (idx[1::2], {"lr": 1e-3, "weight_decay": 0.1, "betas": (0.8, 0.9), "decoupled_weight_decay": True})]
    Harness("radam", {}, SHAPES, "separate", seed=11, groups=groups).run("two groups radam", check_at=(1, R.STEPS))
    groups = [(idx[::2], {}), (idx[1::2], {"lr": 5e-4, "final_lr": 0.02, "gamma": 0.1, "amsbound": True, "betas": (0.8, 0.9)})]
    h = Harness("adabound", {"gamma": 0.5}, SHAPES, "separate", seed=12, groups=groups).run("two groups adabound",
                                                                                            check_at=(1, R.STEPS))
    assert h.opt.base_lrs == [R.LR["adabound"], 5e-4]
    assert "max_exp_avg_sq" in h.opt.state[h.params[1]] and "max_exp_avg_sq" not in h.opt.state[h.params[0]]


@pytest.mark.parametrize("kind", ["radam", "adabound"])
def test_exponential_lr(kind, monkeypatch):
    """ExponentialLR(gamma=0.9) rewrites param_groups[...]['lr']; AdaBound's bounds follow it: the launch scalars of epoch k are
    0.9^k times those of a constant-lr optimiser at the same step count."""
    kw = R.CASES[kind][1]
    lr0 = R.LR[kind]
    h = Harness(kind, kw, SHAPES[:6], "separate", seed=13)
    sched = torch.optim.lr_scheduler.ExponentialLR(h.opt, gamma=0.9)
    seen = _count_calls(monkeypatch)
    for epoch in range(3):
        assert h.opt.param_groups[0]["lr"] == pytest.approx(lr0 * 0.9 ** epoch, rel=1e-12)
        h.step()
        h.step()
        sched.step()
    h.check(f"{kind} ExponentialLR")
    const = R.make_run(kind, kw, h.inputs[5][0])
    for g in h.inputs[5][1][:6]:
        const.step(g, lr0)
    assert not R.within(h.params[5].detach().cpu().numpy(), const.p, const.Ep)[0]     # the schedule matters at this bound
    if kind == "adabound":
        assert h.opt.base_lrs == [lr0] and len(seen) == 6
        for k, (_, a) in enumerate(seen):
            lower, upper = a[7], a[8]
            assert (lower, upper) == h.runs[0].bounds[k]
            assert lower == pytest.approx(const.bounds[k][0] * 0.9 ** (k // 2), rel=1e-12)
            assert upper == pytest.approx(const.bounds[k][1] * 0.9 ** (k // 2), rel=1e-12)


@pytest.mark.parametrize("ours_first,capturable", [(True, False), (False, False), (False, True)])
def test_radam_state_dict_interchange_with_torch(ours_first, capturable):
    """3 steps with one optimiser, state_dict() loaded into the other (torch's, on the same device), 5 more there, across the
    switch: the result stays within the bound of 8 fp64 steps (the bound covers both orders of evaluation).  A capturable
    torch checkpoint carries `step` on the device; ours holds it on the host after loading."""
    kw = R.CASES["radam_wd"][1]
    h = Harness("radam", kw, SHAPES, "separate", seed=14)
    a = h.opt if ours_first else torch.optim.RAdam(h.params, lr=R.LR["radam"], capturable=capturable, **kw)
    b = torch.optim.RAdam(h.params, lr=0.5) if ours_first else h.opt
    h.opt = a
    for _ in range(3):
        h.step()
    sd = a.state_dict()
    assert sd["state"][0]["step"].is_cuda == capturable
    b.load_state_dict(sd)
    assert b.param_groups[0]["lr"] == R.LR["radam"]
    if not ours_first:
        assert b.param_groups[0]["capturable"] is False and b.param_groups[0]["foreach"] is None
        assert all(b.state[p]["step"].device.type == "cpu" and float(b.state[p]["step"]) == 3.0 for p in h.params)
    for k, v in sd["state"][0].items():
        w = b.state_dict()["state"][0][k]
        assert w.dtype == v.dtype and (w.device == v.device or (capturable and k == "step")), k
    h.opt = b
    for _ in range(5):
        h.step()
    h.check(f"radam {'ours->torch' if ours_first else 'torch->ours'} capturable={capturable}")


def test_adabound_takes_a_package_checkpoint():
    """A state as the package writes it (`step` a Python int): loaded, the next step takes the int over as the host fp32 scalar
    and continues from it."""
    kind, kw = R.CASES["adabound"]
    h = Harness(kind, kw, SHAPES[:5], "separate", seed=15)
    for _ in range(2):
        h.step()
    sd = h.opt.state_dict()
    for st in sd["state"].values():
        st["step"] = int(st["step"])
    fresh = _cls(kind)(h.params, lr=R.LR[kind], **kw)
    fresh.load_state_dict(sd)
    assert fresh.state[h.params[0]]["step"] == 2 and not torch.is_tensor(fresh.state[h.params[0]]["step"])
    h.opt = fresh
    h.step()
    h.check("adabound from an int step")


# ---- the scaled entry points and the clipped step

class _Ptr:
    """Stands for the one-element device tensor optim._launch takes as gscale."""

    def __init__(self, ptr):
        self.ptr = ptr

    def data_ptr(self):
        return self.ptr


SIZES = [1, 3, 4, 5, 4095, 4096, 4097, 65536 + 7]        # around the 4096 elements of a block, and 17 blocks
LRS = {"radam": (1e-2, 1e-3), "adabound": (1e-3, 5e-4)}


class Twin:
    """The tensors of SIZES under one optimiser of ours in two parameter groups (even / odd tensors, their own lr), gradients
    in a packed bucket (test_gpu_clip.Twin for the two optimisers of this file); tensor 3 has no gradient at the second
    step, so that AdaBound issues two launches for its group afterwards."""

    def __init__(self, kind, kw, seed):
        self.kind = kind
        self.inputs = [R.inputs(kind, n, seed=seed * 1000 + i, steps=7) for i, n in enumerate(SIZES)]
        self.params = [torch.from_numpy(p0).to(DEV).requires_grad_() for p0, _ in self.inputs]
        self.lay = Layout([(n,) for n in SIZES], "packed", np.random.default_rng(seed), DEV)
        self.opt = _cls(kind)([{"params": self.params[0::2], "lr": LRS[kind][0]}, {"params": self.params[1::2], "lr": LRS[kind][1]}],
                              lr=LRS[kind][0], **kw)

    def lr(self, i):
        return LRS[self.kind][i % 2]

    def live(self, k, i):
        return not (k == 1 and i == 3)

    def set_grads(self, k):
        for i, (p, (_, gs)) in enumerate(zip(self.params, self.inputs)):
            if self.live(k, i):
                self.lay.set(i, gs[k])
                p.grad = self.lay.views[i]
            else:
                p.grad = None

    def grads(self):
        return [None if p.grad is None else p.grad.cpu().numpy().reshape(-1).copy() for p in self.params]

    def tensors(self):
        out = {}
        for i, p in enumerate(self.params):
            out[f"p{i}"] = p.detach().cpu().numpy()
            for k, v in self.opt.state.get(p, {}).items():
                out[f"{k}{i}"] = v.cpu().numpy()
        return out


def _same_bits(a, b, what):
    ta, tb = a.tensors(), b.tensors()
    assert ta.keys() == tb.keys(), what
    for k in ta:
        assert ta[k].dtype == tb[k].dtype and np.array_equal(_bits(ta[k]), _bits(tb[k])), (what, k)


CLIP_CASES = ["radam_all", "radam_decoupled", "adabound_all", "adabound"]


@pytest.mark.parametrize("case", CLIP_CASES)
def test_scaled_entries_without_a_scale_are_the_unscaled_ones(case, monkeypatch):
    """dram_optim_radam_scaled / dram_optim_adabound_scaled with gscale NULL, and with a device coefficient of exactly 1.0: the
    parameters and the state of the unscaled entry bit for bit, over seven steps (across RAdam's switch)."""
    DO = _do()
    kind, kw = R.CASES[case]
    one = torch.ones(1, device=DEV)
    plain, null, unit = (Twin(kind, kw, seed=31) for _ in range(3))
    launch, entries = DO._launch, []

    def routed(gscale):
        def f(entry, rows, *scalars, **_):
            entries.append(entry)
            return launch(entry, rows, *scalars, gscale=gscale)
        return f
    for k in range(7):
        for twin, gscale in ((plain, None), (null, _Ptr(0)), (unit, one)):
            monkeypatch.setattr(DO, "_launch", launch if gscale is None else routed(gscale))
            twin.set_grads(k)
            twin.opt.step()
        monkeypatch.setattr(DO, "_launch", launch)
        _same_bits(plain, null, f"{case} step {k + 1}: gscale NULL")
        _same_bits(plain, unit, f"{case} step {k + 1}: gscale 1.0")
    assert set(entries) == {f"dram_optim_{kind}"}
    moved = sum(int((a != p0).sum()) for a, (p0, _) in zip((p.detach().cpu().numpy() for p in plain.params), plain.inputs))
    assert moved > 0


@pytest.mark.parametrize("case", CLIP_CASES)
@pytest.mark.parametrize("norm_type", [2.0, math.inf])
def test_fused_step_is_clip_then_step(case, norm_type):
    """step() after set_grad_clip(c) against clip_grad_norm_(params, c) followed by step() on a twin: parameters and state bit
    for bit over seven steps (across RAdam's switch; two launches per AdaBound group from the third), two groups with their
    own lr, once with c below the norm and once above; .grad unscaled after the fused step and scaled after the two-pass one;
    a second fused run gives the same bits again; and all of them lie inside the bound of the fp64 run that is fed
    np.float32(coefficient) * g, the coefficient read back from the device."""
    DO = _do()
    kind, kw = R.CASES[case]
    top = max(float(np.abs(g).max()) for _, gs in Twin(kind, kw, seed=32).inputs for g in gs)
    for c, active in ((1e-3 * top, True), (1e4 * top, False)):
        fused, again, two = (Twin(kind, kw, seed=32) for _ in range(3))
        fused.opt.set_grad_clip(c, norm_type)
        again.opt.set_grad_clip(c, norm_type)
        runs = [R.make_run(kind, kw, p0, base_lr=fused.lr(i)) for i, (p0, _) in enumerate(fused.inputs)]
        all_params = [p for g in two.opt.param_groups for p in g["params"]]
        for k in range(7):
            for t in (fused, again, two):
                t.set_grads(k)
            raw = fused.grads()
            fused.opt.step()
            again.opt.step()
            norm = DO.clip_grad_norm_(all_params, c, norm_type)
            two.opt.step()
            torch.cuda.synchronize()
            what = f"{case} norm_type={norm_type} max_norm={c:.3g} step {k + 1}"
            assert _bits(norm.cpu().numpy()) == _bits(fused.opt.last_grad_norm.cpu().numpy()), what
            assert fused.opt.last_grad_norm.shape == () and fused.opt.last_grad_norm.is_cuda
            coef = fused.opt.last_clip_coef.cpu().numpy()
            assert coef.dtype == np.float32 and fused.opt.last_clip_coef.is_cuda
            assert (coef < 1.0) == active, (what, float(norm), float(coef))
            _same_bits(fused, two, what)
            _same_bits(fused, again, what + ": second run")
            worst = 0.0
            for i, (g, gf, gt, run) in enumerate(zip(raw, fused.grads(), two.grads(), runs)):
                if g is None:
                    assert gf is None and gt is None
                    continue
                scaled = coef * g
                assert scaled.dtype == np.float32
                assert np.array_equal(_bits(gf), _bits(g)), f"{what}: the fused step wrote .grad of tensor {i}"
                assert np.array_equal(_bits(gt), _bits(scaled)), f"{what}: clip_grad_norm_ left .grad of tensor {i} unscaled"
                run.step(scaled, fused.lr(i))
                ok, w = R.within(fused.params[i].detach().cpu().numpy(), run.p, run.Ep)
                worst = max(worst, w)
                assert ok, f"{what}: tensor {i}: |err| / bound = {w:.3f}"
            print(f"{what}: norm {float(norm):.6g} coefficient {float(coef):.6g} worst |err| / bound of p {worst:.3f}")
        assert fused.lay.guards_untouched() and two.lay.guards_untouched()
        assert [float(fused.opt.state[p]["step"]) for p in fused.params[2:5]] == [7.0, 6.0, 7.0]


def test_clipping_off_is_the_step_as_it_was(monkeypatch):
    """Without set_grad_clip, and after set_grad_clip(None), step() issues the unscaled launches and nothing else."""
    for kind in ("radam", "adabound"):
        t = Twin(kind, R.CASES[kind][1], seed=33)
        seen = _count_calls(monkeypatch)
        t.set_grads(0)
        t.opt.step()
        t.opt.set_grad_clip(1.0)
        t.opt.set_grad_clip(None)
        t.opt.step()
        assert [n for n, _ in seen] == [f"dram_optim_{kind}"] * 4 and t.opt.last_grad_norm is None
        t.opt.set_grad_clip(1.0)
        t.opt.step()
        assert [n for n, _ in seen[4:]] == ["dram_optim_grad_norm", "dram_optim_grad_norm_finish"] + [f"dram_optim_{kind}_scaled"] * 2
        monkeypatch.undo()


def test_rejects_what_it_cannot_run():
    DO = _do()
    for cls in (DO.RAdam, DO.AdaBound):
        p = torch.zeros(8, device=DEV, dtype=torch.float64).requires_grad_()
        p.grad = torch.zeros_like(p)
        with pytest.raises(TypeError, match="float32"):
            cls([p]).step()
        q = torch.zeros(8, device=DEV).requires_grad_()
        q.grad = torch.zeros_like(q)
        opt = cls([q])
        opt.state[q] = {"step": torch.tensor(1.0, device=DEV), "exp_avg": torch.zeros_like(q), "exp_avg_sq": torch.zeros_like(q)}
        with pytest.raises(RuntimeError, match="step count is a device tensor"):
            opt.step()


@pytest.mark.parametrize("kind", ["radam", "adabound"])
def test_data_parallel_trainer_takes_it_with_max_grad_norm(kind):
    """DataParallelTrainer (world size 1) on models.DC3D(**SLIM), input 2 x 1 x 16^3, one step with max_grad_norm below the
    gradient norm: the trainer hands the clipping to the optimiser's own step() (set_grad_clip), .grad stays unscaled, and
    every parameter lies within the bound of the fp64 update of np.float32(coefficient) * gradient."""
    import models
    from dram_amd.configs import SLIM
    from dram_amd.train_step import DataParallelTrainer, synthetic_batch
    torch.manual_seed(17)
    model = models.DC3D(**SLIM)
    model.init(models.HeNorm(mode="fan_in"))
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    batch = synthetic_batch(2, 16, seed=18, device=DEV)
    assert tuple(batch.images.shape) == (2, 1, 16, 16, 16)
    mg = model.cuda().train()
    kw = {"radam": {}, "adabound": {"final_lr": 0.01}}[kind]           # the reference's settings: lr 1e-4 (final_lr 0.01)
    opt = _cls(kind)(mg.parameters(), lr=1e-4, **kw)
    tr = DataParallelTrainer(mg, opt, max_grad_norm=1e-3)
    assert tr._clip_in_opt and opt._clip == (1e-3, 2)
    tr.step(batch)
    torch.cuda.synchronize()
    norm, coef = float(tr.last_grad_norm), opt.last_clip_coef.cpu().numpy()
    assert tr.last_grad_norm is opt.last_grad_norm and norm > 1e-3 and 0.0 < float(coef) < 1.0
    total, moved = 0.0, 0
    for k, p in mg.named_parameters():
        assert p.grad is not None, k
        g = p.grad.cpu().numpy().reshape(-1)
        total += float((g.astype(np.float64) ** 2).sum())
        run = R.make_run(kind, kw, sd[k].numpy().reshape(-1), base_lr=1e-4).step(coef * g, 1e-4)
        got = p.detach().cpu().numpy().reshape(-1)
        ok, w = R.within(got, run.p, run.Ep)
        assert ok, (kind, k, w)
        moved += int((got != sd[k].numpy().reshape(-1)).sum())
    assert moved > 0
    assert math.sqrt(total) == pytest.approx(norm, rel=1e-5)         # .grad is what the norm was taken of: unscaled
