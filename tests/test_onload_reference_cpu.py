"""tests/onload_reference.py against torch: Chan's combine of the float32-rounded synthetic partials reproduces the mean
and the variance of the tensor they were cut from, for every shape tests/test_gpu_onload.py hands to the device, and empty
pieces change nothing.  Host code only."""
import pytest
import torch

from onload_reference import (BATCH, GROUP, STAT_CASES, act64, coef_table, combine, make_parts, moments_of, random_cuts,
                              stat_case_data, stat_of_row)


def rel(got, ref):
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


@pytest.mark.parametrize("case", STAT_CASES, ids=[c[0] for c in STAT_CASES])
def test_combine_of_parts_reproduces_mean_and_var(case):
    """The partials carry float32 roundings of piece means and M2 (6e-8 relative each, averaged over the pieces), so the
    combined moments must agree with torch's fp64 ones to 1e-6 of the largest value."""
    name, kind, G, N, C, S, nparts, offset = case
    y, cuts = stat_case_data(case)
    parts = make_parts(y, cuts)
    assert parts.dtype == torch.float32 and parts.shape == (N * C, nparts, 3)
    if nparts >= 4:
        assert int((parts[0, :, 2] == 0).sum()) >= 3          # first, one inner and the last piece are empty
        assert bool((parts[:, parts[0, :, 2] == 0] == 0).all())
    st = combine(parts, kind, G, N, C)
    mean, var, var_u = moments_of(y, kind, G)
    assert bool((st["count"] == (N if kind == BATCH else C // G) * S).all())
    assert rel(st["mean"], mean) <= 1e-6
    assert rel(st["var"], var) <= 1e-6
    assert rel(st["var_unbiased"], var_u) <= 1e-6
    assert rel(st["m2"], var * st["count"]) <= 1e-6


def test_empty_pieces_change_nothing():
    gen = torch.Generator().manual_seed(7)
    y = torch.randn(2, 4, 501, generator=gen, dtype=torch.float64) * 1.3 + 0.7
    cuts = [40, 100, 333]
    base = make_parts(y, cuts)
    padded = make_parts(y, [0, 0, 40, 100, 100, 100, 333, 501, 501])
    assert padded.shape[1] == 10 and int((padded[0, :, 2] == 0).sum()) == 6
    assert torch.equal(padded[:, padded[0, :, 2] > 0], base)              # the non-empty pieces are the same triples
    for kind, G in ((BATCH, 1), (GROUP, 1), (GROUP, 2), (GROUP, 4)):
        a, b = combine(base, kind, G, 2, 4), combine(padded, kind, G, 2, 4)
        for k in a:
            assert rel(b[k], a[k]) <= 1e-14, (kind, G, k)
    # and a zero-filled tail appended to the buffer itself
    tail = torch.cat([base, torch.zeros(8, 5, 3)], 1)
    for k, v in combine(tail, BATCH, 1, 2, 4).items():
        assert rel(v, combine(base, BATCH, 1, 2, 4)[k]) <= 1e-14, k


def test_random_cuts_and_statistic_of_row():
    gen = torch.Generator().manual_seed(3)
    for nparts in (1, 2, 7, 2049):
        cuts = random_cuts(6007, nparts, gen)
        assert len(cuts) == nparts - 1 and cuts == sorted(cuts) and all(0 <= c <= 6007 for c in cuts)
    assert stat_of_row(BATCH, 1, 2, 3).tolist() == [0, 1, 2, 0, 1, 2]
    assert stat_of_row(GROUP, 2, 2, 4).tolist() == [0, 0, 1, 1, 2, 2, 3, 3]
    assert stat_of_row(GROUP, 1, 2, 3).tolist() == [0, 0, 0, 1, 1, 1]


def test_coefficient_table_has_the_rows_that_matter():
    gen = torch.Generator().manual_seed(5)
    coef, sp = coef_table(9, gen)
    assert coef.dtype == torch.float32 and coef.shape == (9, 2)
    assert len({tuple(r) for r in coef.tolist()}) == 9                     # every row different
    assert coef[sp["neg"], 0] < 0 and coef[sp["zero"], 0] == 0 and coef[sp["zero"], 1] > 0
    assert bool((coef[:, 1] > 0).any()) and bool((coef[:, 1] < 0).any())
    raw = torch.randn(9, 4000, generator=gen)
    pre, post = act64(raw, coef, 0), act64(raw, coef, 1)
    assert bool((pre[sp["dead"]] < 0).all()) and bool((post[sp["dead"]] == 0).all())
    assert bool((pre[sp["mixed"]] > 0).any()) and bool((pre[sp["mixed"]] < 0).any())
    assert bool((pre[sp["zero"]] == coef[sp["zero"], 1].double()).all())
    assert torch.equal(post, pre.clamp_min(0.0))
    assert coef_table(1, gen)[1] == {"neg": 0}
