"""tests/row_kernel_cases.py against torch on the CPU: the exact-arithmetic condition of every table row, every numpy
reference against the torch op it restates (bit for bit where the GPU test claims bit equality), the derived bound of the
real-valued cases against torch's own fp32 evaluation, and ATen's two-NaN rule as torch has it.  Host code only."""
import pytest
import torch
import torch.nn.functional as F

import row_kernel_cases as K


# ------------------------------------------------------------------------------------------------ exactness
def test_every_exact_case_sums_below_2_to_24():
    """Derived from the builders' ranges and S, not from a run: |partial| <= largest |term| * number of terms, per chunk (the
    fp32 part of every kernel) and per row.  What one result collects from several rows or chunks is added in fp64, where
    integers are exact up to 2^53."""
    seen = 0
    for _, N, C, S in K.MASKED_MEAN_CASES + [("ones", 3, 23, K.S_MULTI), ("per_channel", 3, 4, K.S_MULTI), ("bwd", 1, 1, K.S_MEAN_BWD)]:
        for kind in ("masked_mean", "mask_count"):
            chunk, row = K.worst_case(kind, S)
            assert chunk < K.EXACT_LIMIT and row < K.EXACT_LIMIT, (kind, S)
            seen += 1
    for _, N, C, S in K.CHANNEL_SUM_CASES:
        chunk, channel = K.worst_case("channel_sum", S, rows_per_sum=N)
        assert chunk < K.EXACT_LIMIT and K.worst_case("channel_sum", S)[1] < K.EXACT_LIMIT and channel < K.EXACT_LIMIT
        seen += 1
    for _, N, C, nparam, S in K.PRELU_CHUNK_CASES + K.PRELU_DA_CASES:
        chunk, row = K.worst_case("prelu_da", S)
        assert chunk < K.EXACT_LIMIT and row < K.EXACT_LIMIT, S
        assert K.worst_case("prelu_da", S, rows_per_sum=N * C)[1] < 2 ** 53
        seen += 1
    assert seen == 14 + 4 + 11
    assert K.worst_case("prelu_da", 52 * K.CHUNK - 3) == (32 * 8192, 32 * (52 * 8192 - 3))


def test_builders_keep_their_ranges():
    x = K.ints((3, 5, 1000), K.DATA_MAX, 1)
    assert x.dtype == torch.float32 and torch.equal(x, x.round())
    assert sorted(x.abs().unique().tolist()) == [float(v) for v in range(1, K.DATA_MAX + 1)]
    assert bool((x > 0).any()) and bool((x < 0).any())
    g = K.ints((4000,), K.COT_MAX, 2)
    assert sorted(g.abs().unique().tolist()) == [1.0, 2.0, 3.0, 4.0]
    m = K.masks(3, 3 * K.CHUNK + 77, 3)
    assert sorted(m.unique().tolist()) == [0.0, 1.0]
    assert m[1].sum() == 1 and m[1, -1] == 1                       # the only voxel of sample 1: the last chunk's last element
    assert not torch.equal(m[0], m[2]) and m[0].sum() > m[2].sum() > 1
    for s in K.SLOPES:                                             # powers of two: slope * integer is exact
        assert torch.frexp(torch.tensor(abs(s)))[0].item() == 0.5
    xr, gr = K.relu_input(1000, 4)
    assert int((xr == 0).sum()) >= 143 and bool(torch.isfinite(xr).all()) and bool(torch.isfinite(gr).all())
    assert bool((xr > 0).any()) and bool((xr < 0).any())


def test_shapes_reach_the_paths_they_are_meant_for():
    """The kernel constants the tables are built around (csrc/act.hip, csrc/head.hip, csrc/norm.hip)."""
    cdiv = lambda a, b: -(-a // b)
    assert [cdiv(S, K.CHUNK) for S in K.S_CHUNKED] == [1, 1, 2, 4] and K.S_CHUNKED[3] % K.CHUNK == 77
    assert all(N * C > 64 for _, N, C, _ in K.MASKED_MEAN_CASES)                   # a second finalise block of 64 rows
    assert all(C > 64 for _, N, C, _ in K.CHANNEL_SUM_CASES)                       # ... of 64 channels
    (_, N1, C1, k1, S1), (_, N2, C2, k2, S2), (_, N3, C3, k3, S3) = K.PRELU_DA_CASES
    assert k1 == 1 and N1 * C1 * cdiv(S1, K.CHUNK) > K.THREADS and N1 * C1 == 40
    assert k2 == C2 and N2 * cdiv(S2, K.CHUNK) > K.THREADS
    assert k3 == C3 == 5 and N3 == 3 and cdiv(S3, K.CHUNK) == 3
    assert cdiv(K.S_STREAM, 256 * 8) > 1024 and cdiv(K.S_MEAN_BWD, 256) > 1024 and cdiv(K.RELU_SIZES[-1], 256) > 8192
    d, h, w = K.DHW_MULTI
    assert d * h * w == K.S_MULTI
    assert len(K.GMAX_CASES) == 5 + 5 + 2 + 1 + 5 + 5 + 5 + 4


# ------------------------------------------------------------------------------------------------ references vs torch
def reference_pool(x, lungs):
    """The masked-mean branch of the reference's pooling_dense_features (models.py:45-47), as written."""
    B, C = x.shape[0], x.shape[1]
    e = lungs.expand_as(x)
    return (x * e).view(B, C, -1).sum(dim=-1) / e.view(B, C, -1).sum(dim=-1)


@pytest.mark.parametrize("case", K.MASKED_MEAN_CASES + [("per_channel", 3, 4, K.S_MULTI)], ids=lambda c: c[0])
def test_masked_mean_reference_is_the_formula_in_fp64(case):
    name, N, C, S = case
    x, dout = K.ints((N, C, S), K.DATA_MAX, 11), K.ints((N, C), K.COT_MAX, 12)
    m = K.masks(N * C, S, 13).view(N, C, S) if name == "per_channel" else K.masks(N, S, 13)
    ref = K.masked_mean_ref(x, m, dout)
    x64 = x.double().view(N, C, 1, 1, S).requires_grad_(True)
    l64 = m.double().view(N, -1, 1, 1, S)
    out = reference_pool(x64, l64)
    out.backward(dout.double())
    assert ref["out"].dtype == torch.float32 and torch.equal(ref["out"], out.detach().float())
    assert torch.equal(ref["msum"].double().view(N, -1), l64.view(N, -1, S).sum(-1))
    # dout / count of two fp32 numbers: rounding the fp64 quotient to fp32 IS the correctly rounded fp32 quotient (53 >= 2 * 24 + 2)
    assert ref["dx"].dtype == torch.float32 and torch.equal(ref["dx"], x64.grad.float().view(N, C, S))


def test_all_ones_mask_is_adaptive_avg_pool():
    x = K.ints((3, 23) + K.DHW_MULTI, K.DATA_MAX, 14)
    ref = K.masked_mean_ref(x.view(3, 23, -1), torch.ones(3, K.S_MULTI))
    assert torch.equal(ref["out"], F.adaptive_avg_pool3d(x.double(), 1).view(3, 23).float())
    assert ref["msum"].tolist() == [float(K.S_MULTI)] * 3


@pytest.mark.parametrize("case", K.CHANNEL_SUM_CASES, ids=lambda c: c[0])
def test_channel_sum_reference(case):
    _, N, C, S = case
    x = K.ints((N, C, S), K.DATA_MAX, 15)
    ref = K.channel_sum_ref(x)
    assert ref.dtype == torch.float32 and torch.equal(ref.double(), x.double().sum((0, 2)))


@pytest.mark.parametrize("case", K.PRELU_CHUNK_CASES + K.PRELU_DA_CASES, ids=lambda c: c[0])
def test_prelu_reference_is_F_prelu(case):
    _, N, C, nparam, S = case
    x, dy, a = K.ints((N, C, S), K.DATA_MAX, 16), K.ints((N, C, S), K.COT_MAX, 17), K.slopes(nparam)
    ref = K.prelu_ref(x, a, dy)
    xg, ag = x.clone().requires_grad_(True), a.clone().requires_grad_(True)
    y = F.prelu(xg, ag)
    y.backward(dy)
    assert torch.equal(ref["y"], y.detach()) and torch.equal(ref["dx"], xg.grad)
    a64 = a.double().requires_grad_(True)
    F.prelu(x.double(), a64).backward(dy.double())                 # integers in fp64: the exact sum
    assert torch.equal(torch.from_numpy(ref["da_exact"]).double(), a64.grad)
    assert ref["da"].dtype == torch.float32 and torch.equal(ref["da"], a64.grad.float())


@pytest.mark.parametrize("case", K.GMAX_CASES, ids=lambda c: f"{c[0]}-S{c[1]}")
def test_global_max_patterns_and_their_indices(case):
    """The index each planted row is built to return is the one F.adaptive_max_pool3d returns."""
    pattern, S = case
    x, want = K.gmax_input(pattern, S)
    assert x.shape == (1, K.GMAX_ROWS, 1, 1, S)
    val, idx = F.adaptive_max_pool3d(x, 1, return_indices=True)
    assert torch.equal(idx.view(1, K.GMAX_ROWS), want)
    rows = x.view(K.GMAX_ROWS, S)
    assert K.same_values(val.view(-1), rows[torch.arange(K.GMAX_ROWS), want.view(-1)])
    if pattern == "two_nans":
        assert bool(torch.isnan(val).all()) and bool((torch.isnan(rows).sum(1) == 2).all())
        assert bool((rows.nan_to_num(nan=0.0).max(1).values > K.DATA_MAX).all())      # the larger finite value is there
    elif pattern == "all_neg_inf":
        assert bool((val == float("-inf")).all())
    elif pattern.startswith("tie"):
        assert bool(((rows == val.view(-1, 1)).sum(1) == 2).all())
    elif pattern in ("first", "last", "pos_inf"):
        assert len(set(val.view(-1).tolist())) == (1 if pattern == "pos_inf" else K.GMAX_ROWS)


def test_two_nans_torch_keeps_the_last():
    """Recorded as what torch does: a 2 x 3 x 4 volume with NaN at flat indices 5 and 9 and a larger finite value between
    them returns index 9, and the gradient goes to 9."""
    x = torch.arange(24, dtype=torch.float32).view(1, 1, 2, 3, 4).clone()
    x.view(-1)[5] = x.view(-1)[9] = float("nan")
    x.view(-1)[7] = 100.0
    x.requires_grad_(True)
    val, idx = F.adaptive_max_pool3d(x, 1, return_indices=True)
    assert bool(torch.isnan(val).all()) and idx.item() == 9
    val.backward(torch.full_like(val, 3.0))
    want = torch.zeros(24)
    want[9] = 3.0
    assert torch.equal(x.grad.view(-1), want)


def test_same_values_is_strict():
    a = torch.tensor([1.0, float("nan"), float("inf"), 0.0])
    assert K.same_values(a, a.clone())
    assert not K.same_values(a, torch.tensor([1.0, float("nan"), 3.4028234663852886e38, 0.0]))
    assert not K.same_values(a, torch.tensor([1.0, 2.0, float("inf"), 0.0]))
    assert not K.same_values(a, torch.tensor([1.0, float("nan"), float("inf"), 1e-45]))


# ------------------------------------------------------------------------------------------------ the derived bound
@pytest.mark.parametrize("kind", ["masked_mean", "channel_sum", "prelu_da"])
def test_torch_fp32_meets_the_derived_bound(kind):
    """A bound that the reference's own fp32 arithmetic cannot meet is wrong: torch's fp32 evaluation of the same op on the
    same inputs must lie inside it (and the bound must still be tight enough to see one term: it is below the mean |term|)."""
    t, ref, sum_abs = K.real_case(kind)
    if kind == "masked_mean":
        got = reference_pool(t["x"], t["m"])
    elif kind == "channel_sum":
        got = t["x"].sum((0, 2))
    else:
        a = t["a"].clone().requires_grad_(True)
        F.prelu(t["x"], a).backward(t["dy"])
        got = a.grad
    assert got.dtype == torch.float32 and got.shape == ref.shape
    err, bound = (got.double() - ref).abs(), K.sum_bound(sum_abs, ref)
    print(f"row-kernel-accuracy: torch-CPU-fp32 {kind}: worst err / bound {(err / bound).max().item():.3f}")
    assert bool((err <= bound).all())
    terms = {"masked_mean": 0.4 * K.S_MULTI, "channel_sum": 2 * K.S_MULTI, "prelu_da": 1.5 * K.S_MULTI}[kind]
    assert bool((bound < sum_abs / terms).all())
