"""tests/norm_stat_cases.py on the CPU: its float64 reference is BatchNorm / GroupNorm (+ReLU) as torch's autograd has them, and
its inputs are such that a finalizer of csrc/norm.hip which loses, doubles or mis-weights one (row, chunk) work item -- or a lap
of 256, or a block -- lands at least ten tolerances away from that reference.  Host code only."""
import pytest
import torch
import torch.nn.functional as F

import norm_stat_cases as K
from norm_stat_cases import BATCH, BATCH_IDS, BWD_MUTATIONS, CASE, CASES, EPS, FWD_MUTATIONS, MOMENTUM, U

IDS = [c.id for c in CASES]


def rel(got, ref):
    """max |got - ref| / max |ref|: the first figure of test_gpu_parity.rel_err."""
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def torch_norm(c, x, gamma, beta, rm, rv, training):
    if c.kind == BATCH:
        return F.batch_norm(x, rm, rv, gamma, beta, training, MOMENTUM, EPS)
    return F.group_norm(x, c.G, gamma, beta, EPS)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("case_id", [i for i in IDS if i != "bn_one_value"])
def test_reference_is_torch_autograd_in_float64(case_id, relu):
    c, L, I = CASE[case_id], K.layout(case_id), K.inputs(case_id)
    x = I["x"].double().requires_grad_(True)
    gamma, beta = I["gamma"].double().requires_grad_(True), I["beta"].double().requires_grad_(True)
    rm, rv = I["running_mean"].double(), I["running_var"].double()
    y = torch_norm(c, x, gamma, beta, rm, rv, True)
    y = F.relu(y) if relu else y
    y.backward(I["dy"].double())
    f, b = K.forward_ref(case_id), K.backward_ref(case_id, relu)
    assert rel(K.y_of(f["pre"], relu), y.detach().view(L.rows, c.S)) <= 1e-12
    assert rel(b["dx"], x.grad.view(L.rows, c.S)) <= 1e-12
    assert rel(b["dgamma"], gamma.grad) <= 1e-12 and rel(b["dbeta"], beta.grad) <= 1e-12
    # the statistics by another route: torch.var_mean over the members of each statistic
    xs = I["x"].double().transpose(0, 1).reshape(c.C, -1) if c.kind == BATCH else I["x"].double().reshape(c.N * c.G, -1)
    var, mean = torch.var_mean(xs, 1, unbiased=False)
    assert rel(f["save_mean"], mean) <= 1e-12 and rel(f["save_rstd"], (var + EPS).rsqrt()) <= 1e-12
    assert rel(f["m2"], var * L.count) <= 1e-12
    # {a, b} reproduce y
    coef = f["rowcoef"]
    assert rel(coef[:, :1] * I["x"].double().view(L.rows, c.S) + coef[:, 1:], f["pre"]) <= 1e-12
    if c.kind == BATCH:      # F.batch_norm updated rm / rv in place
        assert rel(f["running_mean"], rm) <= 1e-12 and rel(f["running_var"], rv) <= 1e-12


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("case_id", BATCH_IDS)
def test_eval_reference_is_torch_autograd_in_float64(case_id, relu):
    c, L, I = CASE[case_id], K.layout(case_id), K.inputs(case_id)
    x = I["x"].double().requires_grad_(True)
    gamma, beta = I["gamma"].double().requires_grad_(True), I["beta"].double().requires_grad_(True)
    y = torch_norm(c, x, gamma, beta, I["running_mean"].double(), I["running_var"].double(), False)
    y = F.relu(y) if relu else y
    y.backward(I["dy"].double())
    e = K.eval_ref(case_id, relu)
    assert rel(K.y_of(e["pre"], relu), y.detach().view(L.rows, c.S)) <= 1e-12
    assert rel(e["dx"], x.grad.view(L.rows, c.S)) <= 1e-12
    assert rel(e["dgamma"], gamma.grad) <= 1e-12 and rel(e["dbeta"], beta.grad) <= 1e-12
    assert torch.equal(e["save_mean"], I["running_mean"].double())
    assert rel(e["save_rstd"], (I["running_var"].double() + EPS).rsqrt()) <= 1e-12


def test_one_value_reference_by_formula():
    """torch refuses one value per channel in training.  With one value: mean = x, var = 0, xhat = 0, so y = beta,
    rstd = 1/sqrt(eps), the running variance takes var itself (there is no N - 1), dx = 0, dgamma = 0, dbeta = dy'."""
    I, f = K.inputs("bn_one_value"), K.forward_ref("bn_one_value")
    x, dy = I["x"].double().view(2), I["dy"].double().view(2)
    gamma, beta = I["gamma"].double(), I["beta"].double()
    assert torch.equal(f["save_mean"], x) and torch.equal(f["m2"], torch.zeros(2, dtype=torch.float64))
    assert rel(f["save_rstd"], torch.full((2,), EPS ** -0.5, dtype=torch.float64)) <= 1e-15
    assert torch.equal(f["pre"].view(2), beta)
    assert rel(f["rowcoef"][:, 0], gamma * EPS ** -0.5) <= 1e-15
    assert rel(f["rowcoef"][:, 1], beta - x * gamma * EPS ** -0.5) <= 1e-15
    assert rel(f["running_mean"], (1 - MOMENTUM) * I["running_mean"].double() + MOMENTUM * x) <= 1e-15
    assert rel(f["running_var"], (1 - MOMENTUM) * I["running_var"].double()) <= 1e-15
    for relu in (0, 1):
        b = K.backward_ref("bn_one_value", relu)
        keep = (beta > 0).double() if relu else torch.ones(2, dtype=torch.float64)
        assert torch.equal(b["dx"].view(2), torch.zeros(2, dtype=torch.float64))
        assert torch.equal(b["dgamma"], torch.zeros(2, dtype=torch.float64)) and torch.equal(b["dbeta"], dy * keep)
    assert bool((beta > 0).any()) and bool((beta < 0).any())          # the mask keeps one channel and drops the other


@pytest.mark.parametrize("case_id", IDS)
def test_inputs_are_what_the_table_says(case_id):
    c, L, I, T = CASE[case_id], K.layout(case_id), K.inputs(case_id), K.item_tables(case_id)
    assert I["x"].dtype == torch.float32 and I["x"].shape == (c.N, c.C, c.S) == I["dy"].shape
    g = I["gamma"]
    assert bool((g != 0).all()) and bool((g > 0).any()) and bool((g < 0).any()) and len(set(g.tolist())) == c.C
    for name in ("beta", "running_mean", "running_var"):
        assert len(set(I[name].tolist())) == c.C
    assert bool((I["running_var"] > 0).all())
    # every (row, chunk) has a mean of its own, none near 0, in x and in dy
    off = K.item_offsets(c, 0).abs()
    assert off.min() >= K.OFF_LO and off.max() <= K.OFF_HI and len(set(off.reshape(-1).tolist())) == off.numel()
    if c.S > 1:
        for means in (T["mean"].reshape(-1), T["s1"].reshape(-1) / T["len"].repeat(L.rows)):
            assert len(set(means.tolist())) == means.numel() and means.abs().min() > 1.0


@pytest.mark.parametrize("case_id", IDS)
def test_item_model_without_mutation_is_the_reference(case_id):
    """The per-item combination that the mutated references are written in gives the reference when nothing is mutated."""
    f, b = K.forward_ref(case_id), K.backward_ref(case_id, 0)
    small = K.forward_small(case_id)
    for name, got in small.items():
        ref = f[{"stats_mean": "save_mean", "stats_m2": "m2"}.get(name, name)]
        assert rel(got, ref) <= 1e-12 or (got - ref).abs().max() <= 1e-12, name
    for name, got in K.backward_small(case_id).items():
        assert rel(got, b[name]) <= 1e-12 or (got - b[name]).abs().max() <= 1e-9, name


@pytest.mark.parametrize("case_id", IDS)
def test_no_preactivation_is_within_rounding_of_the_relu_threshold(case_id):
    """The kernels take the ReLU mask from fmaf(a, x, b) in fp32, the reference from float64.  a and b carry a few roundings of
    2^-24 relative to |a|, |beta| and |mean * a|, the fmaf one more: an element can change sides only if its pre-activation is
    within some 4 * 2^-24 of those magnitudes.  The inputs keep 16 * 2^-24, so the two masks are the same set."""
    c, L, f = CASE[case_id], K.layout(case_id), K.forward_ref(case_id)
    if c.S > 1:     # (one value: pre == beta exactly; the fp32 path's rounding there is the GPU test's matter)
        assert K.mask_margin(case_id, f["pre"], f["save_mean"][L.stat], f["rowcoef"][:, 0]) >= 16 * U
    if c.kind == BATCH:
        e = K.eval_ref(case_id, 1)
        assert K.mask_margin(case_id, e["pre"], e["save_mean"][L.chan], e["rowcoef"][:, 0]) >= 16 * U


PAIRS = [(c.id, side, m) for c in CASES for side, names in (("fwd", FWD_MUTATIONS), ("bwd", BWD_MUTATIONS)) for m in names]


@pytest.mark.parametrize("case_id,side,mutation", [q for q in PAIRS if K.applies(*q)], ids=lambda v: str(v))
def test_inputs_can_tell(case_id, side, mutation):
    """For every case and every mutation that changes anything for it, at least one checked output moves from the true
    reference by 10 tolerances or more; the dropped or doubled item is the one that moves the outputs least."""
    L = K.layout(case_id)
    small = K.forward_small if side == "fwd" else K.backward_small
    true = small(case_id)
    if mutation in ("drop_item", "double_item"):
        moved = min(K.movement(case_id, small(case_id, mutation, (r, k)), true) for r in range(L.rows) for k in range(L.nch))
    else:
        moved = K.movement(case_id, small(case_id, mutation), true)
    print(f"norm-stats-sensitivity: {case_id} {side} {mutation}: {moved:.1f} tolerances")
    assert moved >= 10.0


def test_mutations_that_do_not_apply_are_the_identity_and_each_applies_somewhere():
    for side, names, small in (("fwd", FWD_MUTATIONS, K.forward_small), ("bwd", BWD_MUTATIONS, K.backward_small)):
        for m in names:
            assert any(K.applies(c.id, side, m) for c in CASES), m
            for c in CASES:
                if not K.applies(c.id, side, m) and c.N * c.C * c.S < 100000:
                    assert K.movement(c.id, small(c.id, m), small(c.id)) == 0.0, (c.id, side, m)


def test_mean_bound_counts_the_kernel():
    assert K.K_MEAN == 16 + 6 + 3 + 1
    one = torch.ones(1, dtype=torch.float64)
    assert K.mean_bound(one, one).item() == (K.K_MEAN + 1) * U + U
