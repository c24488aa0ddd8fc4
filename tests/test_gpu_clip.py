"""Device gradient clipping (csrc/optim.hip: norm, finish, scaled update, in-place scale) against the restatement of
tests/clip_restatement.py: the norm under its rounding bound, the coefficient bit for bit, the update under the bound of
tests/optim_restatement.py, and the fused step bit for bit against clip-then-step."""
import math

import numpy as np
import pytest
import torch

import clip_restatement as C
import optim_restatement as R
from test_gpu_optim import Layout, _bits

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 4095, 4096, 4097, 65536 + 7]        # around OCHUNK = 4096, and 17 blocks
SHAPES = [(n,) for n in SIZES]
LAYOUTS = ["separate", "off1", "off2", "off3", "packed"]
NORM_TYPES = [2.0, math.inf]
DEV = "cuda"


def _do():
    from dram_amd import optim as DO
    return DO


def _params(shapes):
    return [torch.zeros(s, device=DEV).requires_grad_() for s in shapes]


def _attach(params, lay, arrays):
    """arrays[i] None: no gradient; the others go into the layout's views, which become the .grad."""
    for i, (p, a) in enumerate(zip(params, arrays)):
        if a is None:
            p.grad = None
        else:
            if a.size:
                lay.set(i, a)
            p.grad = lay.views[i]


def _device_norm(params, max_norm, norm_type):
    """[norm, coefficient] as the kernels leave them, nothing scaled (the two launches clip_grad_norm_ starts with)."""
    DO = _do()
    grads = [p.grad for p in params if p.grad is not None and p.grad.numel() > 0]
    out = DO._grad_norm(grads, DO._grad_tables(grads), C.KINDS[float(norm_type)], max_norm)
    return out.cpu().numpy()


def _check_clip(shapes, arrays, layout, max_norm, norm_type, seed=0, what=""):
    """clip_grad_norm_ over `arrays` laid out as `layout`: norm within the bound, coefficient bit-equal to the restatement's
    from the device's own norm, the gradients the fp32 product coefficient * g, everything else untouched.  Returns
    (device norm, device coefficient)."""
    DO = _do()
    params = _params(shapes)
    lay = Layout(shapes, layout, np.random.default_rng(seed), DEV)
    _attach(params, lay, arrays)
    live = [a for a in arrays if a is not None and a.size]
    sizes = [a.size for a in live]
    want = C.total_norm(live, norm_type)
    norm_dev, coef_dev = _device_norm(params, max_norm, norm_type)
    ret = DO.clip_grad_norm_(params, max_norm, norm_type)
    assert ret.shape == () and ret.dtype == torch.float32 and ret.is_cuda
    got = ret.cpu().numpy()
    torch.cuda.synchronize()
    bound = C.norm_bound(want, sizes, norm_type) if math.isfinite(want) else float("nan")
    print(f"{what} {layout} norm_type={norm_type}: device {got!r} fp64 {want!r} |err| {abs(float(got) - want):.3e} bound "
          f"{bound:.3e}; coefficient {coef_dev!r}")
    assert C.norm_within(got, want, sizes, norm_type), (what, layout, norm_type, float(got), want, bound)
    assert _same_scalar(got, norm_dev), "two runs over the same gradients differ"
    coef = C.clip_coef(got, max_norm)
    assert coef.dtype == np.float32 and _same_scalar(coef, coef_dev), (what, layout, norm_type, coef, coef_dev)
    with np.errstate(all="ignore"):
        for i, (p, a) in enumerate(zip(params, arrays)):
            if a is None:
                assert p.grad is None
            elif a.size:
                exp = coef * a.astype(np.float32)
                assert exp.dtype == np.float32
                g = p.grad.cpu().numpy().reshape(-1)
                if np.isnan(exp).any():
                    assert np.array_equal(np.isnan(g), np.isnan(exp)), (what, layout, norm_type, i)
                    ok = ~np.isnan(exp)
                    assert np.array_equal(_bits(g)[ok], _bits(exp.reshape(-1))[ok]), (what, layout, norm_type, i)
                else:
                    assert np.array_equal(_bits(g), _bits(exp.reshape(-1))), (what, layout, norm_type, i)
    assert lay.guards_untouched(), f"{what} {layout}: elements outside the gradient views changed"
    return got, coef_dev


def _same_scalar(a, b):
    """Bit-equal, or both NaN (a NaN's payload carries nothing)."""
    a, b = np.float32(a), np.float32(b)
    return bool(np.isnan(a) and np.isnan(b)) or bool((_bits(a) == _bits(b)).all())


def _random(sizes, seed, scale=0.01):
    rng = np.random.default_rng(seed)
    return [(scale * rng.standard_normal(n)).astype(np.float32) for n in sizes]


@pytest.mark.parametrize("norm_type", NORM_TYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_size_in_every_layout(layout, norm_type):
    """One table of every size: aligned tensors (16-byte groups plus the scalar tail), views 1, 2, 3 elements past a 16-byte
    boundary and back-to-back bucket views (one dword per lane), guard elements bit-unchanged; clipping active (the 2-norm is
    ~ 2.7, the inf-norm ~ 0.04) and inactive."""
    arrays = _random(SIZES, seed=21)
    for max_norm in (0.01, 100.0):
        _, coef = _check_clip(SHAPES, arrays, layout, max_norm, norm_type, seed=22, what=f"max_norm={max_norm}")
        assert (coef < 1.0) == (max_norm == 0.01)


@pytest.mark.parametrize("norm_type", NORM_TYPES)
@pytest.mark.parametrize("live", [65, 129])
def test_more_tensors_than_one_table(live, norm_type):
    """65 and 129 tensors with a gradient (two and three tables: partial_offset), 1 to 9 elements each, packed; one further
    parameter has no gradient and one has no elements."""
    DO = _do()
    assert DO.TABLE_CAPACITY == 64
    sizes = [1 + i % 9 for i in range(live)]
    sizes[3:3] = [7]                                    # no gradient
    sizes[40:40] = [0]                                  # no elements
    arrays = _random(sizes, seed=23)
    arrays[3] = None
    # the largest |g| in the last table, so that the inf-norm depends on partial_offset too
    arrays[-1][0] = np.float32(0.5)
    for max_norm in (0.05, 10.0):
        _check_clip([(n,) for n in sizes], arrays, "packed", max_norm, norm_type, seed=24, what=f"{live} tensors")


@pytest.mark.parametrize("norm_type", NORM_TYPES)
def test_zero_large_and_small_values(norm_type):
    shapes, sizes = [(5,), (4097,), (3,)], [5, 4097, 3]
    zeros = [np.zeros(n, np.float32) for n in sizes]
    norm, coef = _check_clip(shapes, zeros, "off1", 1.0, norm_type, what="zeros")
    assert float(norm) == 0.0 and _bits(coef) == _bits(np.float32(1.0))
    # squares of 1e20 overflow fp32, squares of 1e-30 vanish in it: the sum is an fp64 one
    rng = np.random.default_rng(25)
    big = [(1e20 * (1 + rng.random(n))).astype(np.float32) for n in sizes]
    norm, coef = _check_clip(shapes, big, "packed", 1.0, norm_type, what="1e20")
    assert math.isfinite(float(norm)) and float(norm) >= 1e20 and 0 < float(coef) < 1e-20
    small = [(1e-30 * (1 + rng.random(n))).astype(np.float32) for n in sizes]
    norm, coef = _check_clip(shapes, small, "separate", 1e-31, norm_type, what="1e-30")
    assert 1e-30 <= float(norm) < 1e-27 and float(coef) < 1.0
    mixed = [np.where(rng.random(n) < 0.5, 1e20, 1e-30).astype(np.float32) for n in sizes]
    _check_clip(shapes, mixed, "off3", 1e19, norm_type, what="1e20 and 1e-30")


@pytest.mark.parametrize("norm_type", NORM_TYPES)
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_gradients_poison_as_under_torch(bad, norm_type):
    """One NaN (or infinite) element: norm NaN and coefficient NaN (norm inf and coefficient 0), whichever lane, block and
    table slot holds it; after a clipped Adam step the parameters are non-finite exactly where torch's are after
    torch.nn.utils.clip_grad_norm_ + torch.optim.Adam on the same device."""
    DO = _do()
    shapes, sizes = [(5,), (4097,), (3,)], [5, 4097, 3]
    for ti, ei in ((1, 4096), (1, 77), (2, 1)):         # the scalar tail of a second block, a 16-byte group, a small tensor
        arrays = _random(sizes, seed=26)
        arrays[ti][ei] = np.float32(bad)
        norm, coef = _check_clip(shapes, arrays, "separate", 1.0, norm_type, what=f"{bad} at {ti}/{ei}")
        if math.isnan(bad):
            assert math.isnan(float(norm)) and math.isnan(float(coef))
        else:
            assert float(norm) == math.inf and _bits(coef) == _bits(np.float32(0.0))
    arrays = _random(sizes, seed=26)
    arrays[1][4096] = np.float32(bad)
    p0 = [R.make_inputs(n, seed=27 + i, steps=1)[0] for i, n in enumerate(sizes)]
    masks = {}
    for who in ("ours", "torch"):
        ps = [torch.from_numpy(a).to(DEV).requires_grad_() for a in p0]
        for p, g in zip(ps, arrays):
            p.grad = torch.from_numpy(g).to(DEV)
        if who == "ours":
            opt = DO.Adam(ps, lr=R.LR)
            opt.set_grad_clip(1.0, norm_type)
        else:
            opt = torch.optim.Adam(ps, lr=R.LR)
            torch.nn.utils.clip_grad_norm_(ps, 1.0, norm_type)
        opt.step()
        masks[who] = [torch.isfinite(p.detach()).cpu().numpy() for p in ps]
    for a, b in zip(masks["ours"], masks["torch"]):
        assert np.array_equal(a, b)
    assert not masks["ours"][1][4096]
    assert masks["ours"][0].all() == (not math.isnan(bad))          # inf: coefficient 0, only inf * 0 is lost


# ---- the scaled entry points

class _Ptr:
    """Stands for the one-element device tensor optim._launch takes as gscale."""

    def __init__(self, ptr):
        self.ptr = ptr

    def data_ptr(self):
        return self.ptr


class Twin:
    """The tensors of SIZES under one optimiser of ours in two parameter groups (even / odd tensors, their own lr), gradients
    in a packed bucket, and the inputs of optim_restatement.make_inputs for three steps."""

    LRS = (R.LR, 1e-3)

    def __init__(self, kind, kw, seed):
        DO = _do()
        self.kind, self.kw = kind, kw
        self.inputs = [R.make_inputs(n, seed=seed * 1000 + i, steps=3) for i, n in enumerate(SIZES)]
        self.params = [torch.from_numpy(p0).to(DEV).requires_grad_() for p0, _ in self.inputs]
        self.lay = Layout(SHAPES, "packed", np.random.default_rng(seed), DEV)
        cls = {"adam": DO.Adam, "adamw": DO.AdamW, "sgd": DO.SGD}[kind]
        self.opt = cls([{"params": self.params[0::2], "lr": self.LRS[0]}, {"params": self.params[1::2], "lr": self.LRS[1]}],
                       lr=R.LR, **kw)

    def lr(self, i):
        return self.LRS[i % 2]

    def set_grads(self, k):
        _attach(self.params, self.lay, [gs[k] for _, gs in self.inputs])

    def grads(self):
        return [p.grad.cpu().numpy().reshape(-1).copy() for p in self.params]

    def tensors(self):
        """Every parameter and state tensor, by name, on the host."""
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


IDENTITY_CASES = ["adam", "adam_amsgrad", "adam_wd", "adamw", "sgd_momentum", "sgd_nesterov"]


@pytest.mark.parametrize("case", IDENTITY_CASES)
def test_scaled_entries_without_a_scale_are_the_unscaled_ones(case, monkeypatch):
    """dram_optim_adam_scaled / dram_optim_sgd_scaled with gscale NULL, and with a device coefficient of exactly 1.0: the
    parameters and the state of dram_optim_adam / dram_optim_sgd bit for bit, over three steps."""
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
    for k in range(3):
        for twin, gscale in ((plain, None), (null, _Ptr(0)), (unit, one)):
            monkeypatch.setattr(DO, "_launch", launch if gscale is None else routed(gscale))
            twin.set_grads(k)
            twin.opt.step()
        monkeypatch.setattr(DO, "_launch", launch)
        _same_bits(plain, null, f"{case} step {k + 1}: gscale NULL")
        _same_bits(plain, unit, f"{case} step {k + 1}: gscale 1.0")
    assert len(entries) == 3 * 2 * 2                     # every group of both routed twins went through the scaled entry
    moved = sum(int((a != p0).sum()) for a, (p0, _) in zip((p.detach().cpu().numpy() for p in plain.params), plain.inputs))
    assert moved > 0


@pytest.mark.parametrize("case", ["adam", "adam_all", "adamw_wd_amsgrad", "sgd_momentum", "sgd_maximize"])
@pytest.mark.parametrize("norm_type", NORM_TYPES)
def test_fused_step_is_clip_then_step(case, norm_type):
    """step() after set_grad_clip(m) against clip_grad_norm_(params, m) followed by step() on a twin: parameters and state
    bit for bit over three steps, two groups with their own lr, once with m below the norm (~ 2.7 / ~ 0.05) and once above;
    .grad unscaled after the fused step and scaled after the two-pass one; and both inside optim_restatement's bound of the
    fp64 run that is fed np.float32(c) * g, c read back from the device."""
    DO = _do()
    kind, kw = R.CASES[case]
    for m, active in ((0.02, True), (50.0, False)):
        fused, two = Twin(kind, kw, seed=32), Twin(kind, kw, seed=32)
        fused.opt.set_grad_clip(m, norm_type)
        runs = [R.make_run(kind, kw, p0) for p0, _ in fused.inputs]
        all_params = [p for g in two.opt.param_groups for p in g["params"]]
        for k in range(3):
            fused.set_grads(k)
            two.set_grads(k)
            raw = fused.grads()
            fused.opt.step()
            norm = DO.clip_grad_norm_(all_params, m, norm_type)
            two.opt.step()
            torch.cuda.synchronize()
            what = f"{case} norm_type={norm_type} m={m} step {k + 1}"
            assert _bits(norm.cpu().numpy()) == _bits(fused.opt.last_grad_norm.cpu().numpy()), what
            assert fused.opt.last_grad_norm.shape == () and fused.opt.last_grad_norm.is_cuda
            c = fused.opt.last_clip_coef.cpu().numpy()
            assert c.dtype == np.float32 and _bits(c) == _bits(C.clip_coef(norm.cpu().numpy(), m)), what
            assert (c < 1.0) == active, (what, float(norm), float(c))
            _same_bits(fused, two, what)
            worst = 0.0
            for i, (g, gf, gt, run) in enumerate(zip(raw, fused.grads(), two.grads(), runs)):
                scaled = c * g
                assert scaled.dtype == np.float32
                assert np.array_equal(_bits(gf), _bits(g)), f"{what}: the fused step wrote .grad of tensor {i}"
                assert np.array_equal(_bits(gt), _bits(scaled)), f"{what}: clip_grad_norm_ left .grad of tensor {i} unscaled"
                run.step(scaled, fused.lr(i))
                for t in (fused, two):
                    ok, w = R.within(t.params[i].detach().cpu().numpy(), run.p, run.Ep)
                    worst = max(worst, w)
                    assert ok, f"{what}: tensor {i}: |err| / bound = {w:.3f}"
            print(f"{what}: norm {float(norm):.6g} coefficient {float(c):.6g} worst |err| / bound of p {worst:.3f}")
        assert fused.lay.guards_untouched() and two.lay.guards_untouched()


def test_clipping_off_is_the_step_as_it_was(monkeypatch):
    """Without set_grad_clip, and after set_grad_clip(None), step() issues the unscaled launches and nothing else."""
    DO = _do()
    seen = []
    real = DO.call
    monkeypatch.setattr(DO, "call", lambda name, *a: (seen.append(name), real(name, *a))[1])
    t = Twin("adam", {}, seed=33)
    t.set_grads(0)
    t.opt.step()
    t.opt.set_grad_clip(1.0)
    t.opt.set_grad_clip(None)
    t.opt.step()
    assert seen == ["dram_optim_adam"] * 4 and t.opt.last_grad_norm is None
    t.opt.set_grad_clip(1.0)
    t.opt.step()
    assert seen[4:] == ["dram_optim_grad_norm", "dram_optim_grad_norm_finish", "dram_optim_adam_scaled", "dram_optim_adam_scaled"]


@pytest.mark.parametrize("norm_type", NORM_TYPES)
def test_error_if_nonfinite_raises_before_scaling(norm_type):
    DO = _do()
    arrays = _random(SIZES, seed=34)
    arrays[5][17] = np.float32("nan")
    params = _params(SHAPES)
    lay = Layout(SHAPES, "off2", np.random.default_rng(35), DEV)
    _attach(params, lay, arrays)
    with pytest.raises(RuntimeError, match=f"The total norm of order {float(norm_type)} for gradients from `parameters` is "
                                           f"non-finite, so it cannot be clipped"):
        DO.clip_grad_norm_(params, 1e-3, norm_type, error_if_nonfinite=True)
    for p, a in zip(params, arrays):
        g = p.grad.cpu().numpy()
        assert np.array_equal(np.isnan(g), np.isnan(a)) and np.array_equal(_bits(g)[~np.isnan(a)], _bits(a)[~np.isnan(a)])
    assert lay.guards_untouched()
    # finite gradients: the flag changes nothing
    arrays[5][17] = np.float32(0.25)
    _attach(params, lay, arrays)
    a = DO.clip_grad_norm_(params, 1e-3, norm_type, error_if_nonfinite=True)
    _attach(params, lay, arrays)
    b = DO.clip_grad_norm_(params, 1e-3, norm_type)
    assert _bits(a.cpu().numpy()) == _bits(b.cpu().numpy())


@pytest.mark.parametrize("norm_type", NORM_TYPES)
def test_norm_agrees_with_torch_on_the_device(norm_type):
    """torch.nn.utils.clip_grad_norm_ on the same device tensors: the two norms differ by no more than the kernel's bound
    plus torch's fp32 one (clip_restatement.torch_fp32_norm_bound), and the clipped gradients by the roundings of the
    coefficient (ours: one quotient; torch: a reciprocal and a product) and of the product."""
    DO = _do()
    arrays = _random(SIZES, seed=36)
    ours, theirs = _params(SHAPES), _params(SHAPES)
    for ps in (ours, theirs):
        for p, a in zip(ps, arrays):
            p.grad = torch.from_numpy(a).to(DEV)
    a = float(DO.clip_grad_norm_(ours, 0.01, norm_type))
    b = float(torch.nn.utils.clip_grad_norm_(theirs, 0.01, norm_type))
    want = C.total_norm(arrays, norm_type)
    bound = C.norm_bound(want, SIZES, norm_type) + (0.0 if norm_type == math.inf else C.torch_fp32_norm_bound(want, SIZES))
    print(f"norm_type={norm_type}: ours {a!r} torch {b!r} fp64 {want!r} bound {bound:.3e}")
    assert abs(a - b) <= bound
    for p, q, g in zip(ours, theirs, arrays):
        # ours: norm, sum, quotient, product (3u beside the norm's bound); torch: norm, sum, reciprocal, product, product (4u)
        tol = (bound / want + 8 * C.UE) * (0.01 / want) * np.abs(g.astype(np.float64)) + 2.0 ** -149
        assert (np.abs(p.grad.cpu().numpy().astype(np.float64) - q.grad.cpu().numpy()) <= tol).all()


def test_rejects_what_it_cannot_run():
    DO = _do()
    p = torch.zeros(8, device=DEV, dtype=torch.float64).requires_grad_()
    p.grad = torch.ones_like(p)
    with pytest.raises(TypeError, match="float32"):
        DO.clip_grad_norm_([p], 1.0)
    # a non-contiguous gradient is clipped where it lies
    g = (0.5 + np.arange(12, dtype=np.float32)).reshape(4, 3)
    r = torch.zeros(3, 4, device=DEV).requires_grad_()
    r.grad = torch.from_numpy(g).to(DEV).t()
    assert not r.grad.is_contiguous()
    norm = DO.clip_grad_norm_(r, 1.0).cpu().numpy()
    assert C.norm_within(norm, C.total_norm([g], 2.0), [12], 2.0)
    assert np.array_equal(_bits(r.grad.cpu().numpy()), _bits((C.clip_coef(norm, 1.0) * g).T))
    # nothing with a gradient: zero, and no launch
    q = torch.zeros(4, device=DEV).requires_grad_()
    assert float(DO.clip_grad_norm_([q], 1.0)) == 0.0
    e = torch.zeros(0, device=DEV).requires_grad_()
    e.grad = torch.zeros(0, device=DEV)
    assert float(DO.clip_grad_norm_([e, q], 1.0, math.inf)) == 0.0


def test_runs_on_the_current_stream():
    DO = _do()
    (a,) = _random([1 << 16], seed=37)
    p = torch.zeros(1 << 16, device=DEV).requires_grad_()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        p.grad = torch.from_numpy(a).to(DEV)
        norm = DO.clip_grad_norm_([p], 0.5)
    s.synchronize()
    got = norm.cpu().numpy()
    assert C.norm_within(got, C.total_norm([a], 2.0), [a.size], 2.0)
    assert np.array_equal(_bits(p.grad.cpu().numpy()), _bits(C.clip_coef(got, 0.5) * a))
