"""dram_amd.optim (csrc/optim.hip) on the device against the fp64 restatement of tests/optim_restatement.py, under the
rounding-error bound that tests/test_optim_cpu.py holds torch's own fp32 optimisers to."""
import numpy as np
import pytest
import torch

import optim_restatement as R

pytestmark = pytest.mark.gpu

SHAPES = [(1,), (3,), (4,), (5,), (1023,), (1024,), (1025,), (65536 + 7,), (8, 4, 3, 3, 3)]
GUARD = 5
QUANT = {"adam": ("p", "g", "m", "v", "vmax"), "adamw": ("p", "g", "m", "v", "vmax"), "sgd": ("p", "g")}


def _classes():
    from dram_amd import optim as DO
    return {"adam": DO.Adam, "adamw": DO.AdamW, "sgd": DO.SGD}


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


class Layout:
    """The tensors of one quantity (p, g, m, ...) on the device.  layout 'separate': one allocation each.  'off1' / 'off2' /
    'off3': views into one flat buffer, each starting that many elements past a 16-byte boundary, GUARD or more sentinel
    elements between them.  'packed': views back to back with nothing between (the trainer's gradient buckets: whatever offset
    the sizes add up to)."""

    def __init__(self, shapes, layout, rng, dev):
        self.flat = None
        sizes = [int(np.prod(s)) for s in shapes]
        if layout == "separate":
            self.views = [torch.zeros(s, device=dev) for s in shapes]
            return
        starts, cur = [], 0
        for n in sizes:
            if layout == "packed":
                starts.append(cur)
            else:
                starts.append((cur + GUARD + 3) // 4 * 4 + int(layout[3:]))
            cur = starts[-1] + n
        total = cur + (0 if layout == "packed" else GUARD)
        self.host = rng.standard_normal(total).astype(np.float32)          # sentinels everywhere
        self.flat = torch.from_numpy(self.host).to(dev)
        assert self.flat.data_ptr() % 16 == 0
        self.views = [self.flat[a:a + n].view(s) for a, n, s in zip(starts, sizes, shapes)]
        self.outside = np.ones(total, dtype=bool)
        for a, n in zip(starts, sizes):
            self.outside[a:a + n] = False

    def set(self, i, arr):
        self.views[i].copy_(torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32)).view(self.views[i].shape))

    def guards_untouched(self):
        if self.flat is None:
            return True
        return np.array_equal(_bits(self.flat.cpu().numpy())[self.outside], _bits(self.host)[self.outside])


class Harness:
    """`shapes` tensors under one optimiser of ours, every quantity laid out as `layouts` says (a name, or a dict per quantity),
    and one restatement run per tensor.  Tensor i gets no gradient at the steps listed in none_at.get(i, ())."""

    def __init__(self, kind, kw, shapes, layouts, seed, groups=None, lr=R.LR, state=None, none_at=None):
        dev = torch.device("cuda")
        rng = np.random.default_rng(seed)
        self.kind, self.kw, self.shapes, self.lr = kind, kw, shapes, lr
        self.none_at = none_at or {}
        amsgrad = bool(kw.get("amsgrad"))
        names = [q for q in QUANT[kind] if q != "vmax" or amsgrad]
        if not isinstance(layouts, dict):
            layouts = {q: layouts for q in names}
        self.q = {q: Layout(shapes, layouts.get(q, "separate"), rng, dev) for q in names}
        self.inputs = [R.make_inputs(int(np.prod(s)), seed=seed * 1000 + i) for i, s in enumerate(shapes)]
        self.params = []
        for i in range(len(shapes)):
            self.q["p"].set(i, self.inputs[i][0])
            self.params.append(self.q["p"].views[i].requires_grad_())
        # groups: list of (indices, overrides); every group's restatement takes its own hyper-parameters
        groups = groups or [(list(range(len(shapes))), {})]
        self.hyper = {}
        pg = []
        for idx, over in groups:
            pg.append({"params": [self.params[i] for i in idx], **over})
            for i in idx:
                self.hyper[i] = over
        self.opt = _classes()[kind](pg, lr=lr, **kw)
        self.runs = []
        for i in range(len(shapes)):
            h = dict(kw)
            h.update({k: v for k, v in self.hyper[i].items() if k != "lr"})
            st = {} if state is None else state[i]
            self.runs.append(R.make_run(kind, h, self.inputs[i][0], **st))
            if kind != "sgd" and (state is not None or layouts.get("m", "separate") != "separate"):
                s = {"step": torch.tensor(float(st.get("step", 0)), dtype=torch.float32)}
                for q, key in (("m", "exp_avg"), ("v", "exp_avg_sq"), ("vmax", "max_exp_avg_sq")):
                    if q in self.q:
                        self.q[q].set(i, st.get(q, np.zeros(shapes[i])))
                        s[key] = self.q[q].views[i]
                self.opt.state[self.params[i]] = s
        self.k = 0

    def step(self):
        for i, p in enumerate(self.params):
            g = None if self.k in self.none_at.get(i, ()) else self.inputs[i][1][self.k]
            if g is None:
                p.grad = None
            else:
                self.q["g"].set(i, g)
                p.grad = self.q["g"].views[i]
            lr = next(gr["lr"] for gr in self.opt.param_groups if any(p is q for q in gr["params"]))
            self.runs[i].step(g, lr)
        self.opt.step()
        self.k += 1

    def check(self, what=""):
        torch.cuda.synchronize()
        worst = {}
        for i, (p, run) in enumerate(zip(self.params, self.runs)):
            got = [("p", p.detach(), run.p, run.Ep)]
            st = self.opt.state.get(p, {})
            if self.kind == "sgd":
                if run.buf is not None:
                    got.append(("buf", st["momentum_buffer"], run.buf, run.Eb))
                else:
                    assert "momentum_buffer" not in st
            elif run.t == 0 and "step" not in st:
                assert len(st) == 0
            else:
                assert float(st["step"]) == run.t, (what, i, float(st["step"]), run.t)
                assert st["step"].device.type == "cpu" and st["step"].dtype == torch.float32
                got += [("m", st["exp_avg"], run.m, run.Em), ("v", st["exp_avg_sq"], run.v, run.Ev)]
                if run.amsgrad:
                    got.append(("vmax", st["max_exp_avg_sq"], run.vmax, run.Evmax))
            for name, t, want, bound in got:
                ok, w = R.within(t.cpu().numpy().reshape(-1), want, bound)
                worst[name] = max(worst.get(name, 0.0), w)
                assert ok, f"{what}: tensor {i} {tuple(self.shapes[i])} {name}: |err| / bound = {w:.3f}"
        for q, lay in self.q.items():
            assert lay.guards_untouched(), f"{what}: elements outside the {q} views changed"
        print(f"{what} after {self.k} steps: worst |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))

    def run(self, what, steps=5, check_at=(1, 5)):
        for _ in range(steps):
            self.step()
            if self.k in check_at:
                self.check(what)
        return self


NONE_AT = {2: (0, 1, 2, 3, 4), 6: (2,)}     # tensor 2 never has a gradient; tensor 6 misses the third step


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_every_option_on_separate_tensors(case):
    """Every size (aligned: the 16-byte instantiation plus the scalar tail), every option combination, after 1 and 5 steps; one
    parameter never has a gradient (untouched, no state) and one misses a step (its step count stays behind)."""
    kind, kw = R.CASES[case]
    h = Harness(kind, kw, SHAPES, "separate", seed=3, none_at=NONE_AT).run(case)
    assert np.array_equal(_bits(h.params[2].detach().cpu().numpy().reshape(-1)), _bits(h.inputs[2][0]))
    assert len(h.opt.state.get(h.params[2], {})) == 0
    if kind != "sgd":
        assert [float(h.opt.state[p]["step"]) for p in (h.params[0], h.params[6])] == [5.0, 4.0]


@pytest.mark.parametrize("layout", ["off1", "off2", "off3"])
@pytest.mark.parametrize("case", ["adam", "adam_all", "adamw_wd_amsgrad", "sgd_nesterov", "sgd_dampening"])
def test_views_into_flat_buffers(case, layout):
    """p, g, m, v, vmax as views 1, 2 and 3 elements past a 16-byte boundary (the scalar instantiation), guard elements around
    every view bit-unchanged."""
    kind, kw = R.CASES[case]
    Harness(kind, kw, SHAPES, layout, seed=4, none_at=NONE_AT).run(f"{case}/{layout}")


@pytest.mark.parametrize("case", ["adam", "adam_amsgrad", "sgd_momentum"])
def test_packed_gradient_bucket(case):
    """The trainer's case: parameters and state in their own allocations, gradients back to back in one flat bucket, so one
    launch holds aligned and misaligned tensors; and the same with the state guarded in aligned flat buffers."""
    kind, kw = R.CASES[case]
    Harness(kind, kw, SHAPES, {"g": "packed"}, seed=5).run(f"{case}/bucket")
    if kind != "sgd":
        Harness(kind, kw, SHAPES, {"g": "packed", "p": "off0", "m": "off0", "v": "off0", "vmax": "off0"}, seed=6).run(
            f"{case}/bucket+guards")


def test_table_longer_than_one_launch():
    from dram_amd import optim as DO
    shapes = [(1 + i % 7,) for i in range(DO.TABLE_CAPACITY + 1)]
    Harness("adam", {"weight_decay": 0.05}, shapes, "packed", seed=7).run("capacity+1")
    Harness("sgd", {"momentum": 0.9}, shapes, {"p": "packed", "g": "packed"}, seed=8).run("capacity+1 sgd")


def test_loaded_state_with_differing_step_counts():
    rng = np.random.default_rng(9)
    state = []
    for i, s in enumerate(SHAPES):
        n = int(np.prod(s))
        v = (1e-4 * rng.random(n)).astype(np.float32)
        state.append({"step": (0, 1, 7, 100, 3, 2, 1000, 12, 5)[i], "m": (0.01 * rng.standard_normal(n)).astype(np.float32),
                      "v": v, "vmax": (v * (1 + rng.random(n))).astype(np.float32)})
    h = Harness("adam", {"amsgrad": True}, SHAPES, "off1", seed=10, state=state).run("loaded state")
    assert [float(h.opt.state[p]["step"]) for p in h.params] == [s["step"] + 5.0 for s in state]


def test_two_groups_with_their_own_hyper_parameters():
    idx = list(range(len(SHAPES)))
    groups = [(idx[::2], {}), (idx[1::2], {"lr": 1e-3, "weight_decay": 0.1, "betas": (0.8, 0.9)})]
    Harness("adam", {}, SHAPES, "separate", seed=11, groups=groups).run("two groups")
    groups = [(idx[::2], {}), (idx[1::2], {"lr": 1e-3, "momentum": 0.5})]
    Harness("sgd", {"momentum": 0.9}, SHAPES, "separate", seed=12, groups=groups).run("two groups sgd")


def test_exponential_lr():
    """st_dram_ref.py's schedule: ExponentialLR(gamma=0.9) stepped once per epoch reads and writes param_groups[...]['lr']."""
    h = Harness("adam", {}, SHAPES[:6], "separate", seed=13, lr=1e-2)
    sched = torch.optim.lr_scheduler.ExponentialLR(h.opt, gamma=0.9)
    for epoch in range(3):
        assert h.opt.param_groups[0]["lr"] == pytest.approx(1e-2 * 0.9 ** epoch, rel=1e-12)
        h.step()
        if epoch == 2:
            h.step()
        sched.step()
    h.check("ExponentialLR")
    # the schedule matters at this bound: a constant-lr run is far outside it
    const = R.make_run("adam", {}, h.inputs[5][0])
    for g in h.inputs[5][1][:4]:
        const.step(g, 1e-2)
    assert not R.within(h.params[5].detach().cpu().numpy(), const.p, const.Ep)[0]


@pytest.mark.parametrize("kind,kw", [("adam", {"amsgrad": True, "weight_decay": 0.05}), ("sgd", {"momentum": 0.9})])
@pytest.mark.parametrize("ours_first", [True, False])
def test_state_dict_interchange_with_torch(kind, kw, ours_first):
    """2 steps with one optimiser, state_dict() loaded into the other (torch's, on the same device), 2 more there: the result
    stays within the bound of 4 fp64 steps (the bound covers both orders of evaluation)."""
    theirs = {"adam": torch.optim.Adam, "sgd": torch.optim.SGD}[kind]
    h = Harness(kind, kw, SHAPES, "separate", seed=14)
    a = h.opt if ours_first else theirs(h.params, lr=R.LR, **kw)
    b = theirs(h.params, lr=0.5) if ours_first else h.opt
    h.opt = a
    h.step()
    h.step()
    sd = a.state_dict()
    b.load_state_dict(sd)
    assert b.param_groups[0]["lr"] == R.LR
    for k, v in sd["state"][0].items():
        w = b.state_dict()["state"][0][k]
        assert (w.dtype, w.device) == (v.dtype, v.device), k
    h.opt = b
    h.step()
    h.step()
    h.check(f"{kind} {'ours->torch' if ours_first else 'torch->ours'}")


def test_rejects_what_it_cannot_run():
    from dram_amd import optim as DO
    p = torch.zeros(8, device="cuda", dtype=torch.float64).requires_grad_()
    p.grad = torch.zeros_like(p)
    with pytest.raises(TypeError, match="float32"):
        DO.Adam([p]).step()
    q = torch.zeros((4, 4), device="cuda").requires_grad_()
    q.grad = torch.sparse_coo_tensor(torch.tensor([[0], [1]]), torch.tensor([1.0]), (4, 4)).cuda()
    with pytest.raises(RuntimeError, match="sparse"):
        DO.SGD([q], lr=0.1).step()
    # a non-contiguous gradient is made contiguous
    p0, gs = R.make_inputs(12, seed=15, steps=1)
    r = torch.from_numpy(p0).cuda().view(3, 4).requires_grad_()
    r.grad = torch.from_numpy(gs[0]).cuda().view(4, 3).t()
    assert not r.grad.is_contiguous()
    DO.Adam([r], lr=R.LR).step()
    run = R.make_run("adam", {}, p0).step(gs[0].reshape(4, 3).T.reshape(-1), R.LR)
    assert R.within(r.detach().cpu().numpy().reshape(-1), run.p, run.Ep)[0]


def test_runs_on_the_current_stream():
    from dram_amd import optim as DO
    p0, gs = R.make_inputs(1 << 16, seed=16, steps=1)
    p = torch.from_numpy(p0).cuda().requires_grad_()
    s = torch.cuda.Stream()
    opt = DO.Adam([p], lr=R.LR)
    with torch.cuda.stream(s):
        p.grad = torch.from_numpy(gs[0]).cuda()
        opt.step()
    s.synchronize()
    run = R.make_run("adam", {}, p0).step(gs[0], R.LR)
    assert R.within(p.detach().cpu().numpy(), run.p, run.Ep)[0]


def test_data_parallel_trainer_takes_it_unchanged():
    """DataParallelTrainer (world size 1) on models.DC3D(**SLIM), input 2 x 1 x 16^3: one step with dram_amd.optim.Adam and one
    with torch.optim.Adam from the same weights; every parameter of either lies within the bound of the fp64 update of the
    gradient that run saw, so the two agree within the two bounds' sum."""
    import models
    from dram_amd import optim as DO
    from dram_amd.configs import SLIM
    from dram_amd.train_step import DataParallelTrainer, synthetic_batch
    torch.manual_seed(17)
    model = models.DC3D(**SLIM)
    model.init(models.HeNorm(mode="fan_in"))
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    batch = synthetic_batch(2, 16, seed=18, device="cuda")
    assert tuple(batch.images.shape) == (2, 1, 16, 16, 16)
    out = {}
    for name, cls in (("ours", DO.Adam), ("torch", torch.optim.Adam)):
        model.load_state_dict(sd)
        mg = model.cuda().train()
        tr = DataParallelTrainer(mg, cls(mg.parameters(), lr=1e-4))
        tr.step(batch)
        torch.cuda.synchronize()
        res = {}
        for k, p in mg.named_parameters():
            assert p.grad is not None, k
            run = R.make_run("adam", {}, sd[k].numpy().reshape(-1)).step(p.grad.cpu().numpy().reshape(-1), 1e-4)
            got = p.detach().cpu().numpy().reshape(-1)
            ok, w = R.within(got, run.p, run.Ep)
            assert ok, (name, k, w)
            res[k] = (got, run.Ep)
        out[name] = res
        model = model.cpu()
    moved = 0
    for k in out["ours"]:
        (a, ea), (b, eb) = out["ours"][k], out["torch"][k]
        assert (np.abs(a.astype(np.float64) - b) <= ea + eb).all(), k
        moved += int((a != sd[k].numpy().reshape(-1)).sum())
    assert moved > 0
