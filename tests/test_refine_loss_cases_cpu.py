"""Host-side checks of tests/refine_loss_cases.py, the reference tests/test_gpu_refine_loss_kernels.py holds the fused
IntRegRefineLoss kernels of csrc/loss.hip to:
  * the float64 restatement equals oracle.dram_oracle.fused_loss_math in value and gradient, and the hinge of
    reg_loss_with_probs plus boot_bce on the same pseudo label (the form that decides the tie at p = 0.5);
  * every case satisfies the input conditions, by their margins, and lies in the regime its name claims;
  * every count is below 2^24, so the kernels' fp32 counters are exact;
  * sensitivity: a reference with c_out or c_boot scaled by 1.01, alpha shifted by 1e-3, sample 256 dropped or the last
    element of the ragged chunk dropped fails the comparators of the GPU test."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import refine_loss_cases as R
from oracle import dram_oracle as O

SMALL = [c for c in R.CASES if c != "cap"]


# ------------------------------------------------------------------------------------------------ against the oracle
def _oracle(inp, with_boot_bce):
    """(reg, seg, dreg, dseg) from oracle.dram_oracle on 5-D tensors."""
    N, S = inp.dense.shape
    t5 = lambda a: torch.from_numpy(a).double().view(N, 1, 1, 1, S)
    d = t5(inp.dense).requires_grad_(True)
    x = d if inp.refined is None else t5(inp.refined).requires_grad_(True)
    lobes, lesions = t5(inp.lobes), t5(inp.lesions)
    keep = torch.from_numpy(inp.keep).double().view(N, 1, 1, 1, 1)
    batch = SimpleNamespace(lobes=lobes, lesions=lesions, keep=keep, targets=torch.from_numpy(inp.targets).double(),
                            weight=torch.from_numpy(inp.weight).double())
    reg, seg = O.fused_loss_math(d, batch, refined=None if x is d else x, smoothing=R.SMOOTHING)
    if with_boot_bce:
        with torch.no_grad():
            pseudo = ((torch.sigmoid(d) > 0.5) & (lobes > 0) & (lesions > 0)).double() * keep
        seg = O.boot_bce(torch.sigmoid(x), pseudo, lobes > 0, R.SMOOTHING)
    dreg, = torch.autograd.grad(reg, d, retain_graph=True)
    dseg, = torch.autograd.grad(seg, x)
    return float(reg.detach()), float(seg.detach()), dreg.view(N, S).numpy(), dseg.view(N, S).numpy()


@pytest.mark.parametrize("cid", ["s257", "s8193", "alpha_clamped_25", "keep_mixed", "refined", "saturation", "n257"])
@pytest.mark.parametrize("with_boot_bce", [False, True])
def test_restatement_equals_oracle(cid, with_boot_bce):
    """Values to 1e-12.  Gradients element for element: the oracle forms 1 - p from a rounded p (relative error up to
    1.1e-16 / 1.86e-7 = 6e-10 at |d| = 15.5) and sigmoid's derivative as p (1 - p), which is 0 from |d| = 37 on where the
    restatement has e^-|d|: hence 1e-6 relative and 1e-30 absolute.  fused_loss_math spells the boot term with
    torch.maximum, whose gradient at the tie p = 0.5 is the mean of both sides; the reference's [p > 0.5] (boot_bce) takes
    the 1 - p side, as the kernel and the restatement do, so the exact zeros are left out of the first comparison only."""
    inp, ref = R.build(cid), R.reference(cid)
    reg, seg, dreg, dseg = _oracle(inp, with_boot_bce)
    assert abs(reg - ref["reg"]) <= 1e-12 * max(1.0, abs(reg)) and abs(seg - ref["seg"]) <= 1e-9 * max(1.0, abs(seg))
    sel = np.ones(inp.dense.shape, bool) if with_boot_bce else (inp.dense if inp.refined is None else inp.refined) != 0
    np.testing.assert_allclose(ref["dreg"], dreg, rtol=1e-6, atol=1e-30)
    np.testing.assert_allclose(ref["dseg"][sel], dseg[sel], rtol=1e-6, atol=1e-30)
    if not with_boot_bce and inp.refined is None:
        assert (~sel).any() and float(np.abs(ref["dseg"][~sel]).min()) > 0.0      # the tie carries the 1 - p side's gradient


# ------------------------------------------------------------------------------------------------ conditions and regimes
@pytest.mark.parametrize("cid", list(R.CASES))
def test_input_conditions(cid):
    c, inp = R.CASES[cid], R.build(cid)
    cond = R.conditions(cid, inp)
    assert cond["min_nonzero"] >= R.ZERO_MARGIN and cond["in_gap"] == 0 and cond["finite"], cond
    assert cond["hinge_margin"] >= R.HINGE_MARGIN, cond
    assert cond["binary_masks"] and cond["lesion_outside_lobe"] == 0 and cond["zeros_elsewhere"] == 0, cond
    assert cond["zeros_on_lesion_in_lobe"] > 0 or c.S == 1, cond
    assert cond["max_count"] < 2 ** 24, cond
    assert cond["samples_without_inside"] == sorted(list(c.empty) + ([1] if c.S == 1 else [])), cond
    assert cond["samples_without_outside"] == (list(range(c.N)) if cid == "no_outside" else [0, 2] if c.S == 1 else []), cond
    m = inp.lobes > 0
    assert m.any() and ((~m).any() or cid == "no_outside")          # the batch as a whole has both
    for t in inp:
        assert t is None or t.dtype == np.float32
    assert np.all((inp.weight >= 0.2) & (inp.weight <= 0.8)) and (c.N == 1 or len(set(inp.weight[:3].tolist())) == min(c.N, 3))
    sat = np.abs(inp.dense) >= R.SAT_MIN
    if cid == "saturation":     # samples 0, 1 mostly saturated on both sides, 2 mixed, every magnitude present
        share = sat.mean(1)
        assert share[0] > 0.8 and share[1] > 0.8 and 0.2 < share[2] < 0.4, share
        for v in R.SAT_VALUES:
            assert (inp.dense == np.float32(v)).any() and (inp.dense == -np.float32(v)).any()
        assert (sat & m).any() and (sat & ~m).any()
    else:
        assert not sat.any()


def test_refined_absent_is_refined_without_the_tensor():
    a, b = R.build("refined"), R.build("refined_absent")
    assert a.refined is not None and b.refined is None and not np.array_equal(a.refined, a.dense)
    for name in ("dense", "lobes", "lesions", "keep", "targets", "weight"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name


def _hinge_kinds(inp, ref):
    lo, hi = inp.targets[:, 0].astype(np.float64), inp.targets[:, 1].astype(np.float64)
    return ["none" if np.isnan(r) else "below" if r < l else "above" if r > h else "inside" for r, l, h in zip(ref["r"], lo, hi)]


@pytest.mark.parametrize("cid", SMALL)
def test_regime_claims(cid):
    c, inp, ref = R.CASES[cid], R.build(cid), R.reference(cid)
    assert max(ref["n_in"], ref["n_out"], ref["T"]) < 2 ** 24 and float(ref["nm"].max()) < 2 ** 24
    assert np.isfinite([ref["reg"], ref["seg"], ref["alpha"], ref["wsum"]]).all()
    assert np.isfinite(ref["dreg"]).all() and np.isfinite(ref["dseg"]).all()
    share = ref["T"] / ref["n_in"]
    want = R.ALPHA_REGIME.get(cid)
    if want == "interior":
        assert 0.3 <= share <= 0.7 and ref["alpha"] == 1.0 - share
    elif want == 0.75:
        assert share < 0.2 and ref["alpha"] == 0.75
    elif want == 0.25:
        assert share > 0.8 and ref["alpha"] == 0.25
    kinds = _hinge_kinds(inp, ref)
    if c.N >= 3 and cid not in ("s1", "empty_lobe"):
        assert {"below", "inside", "above"} <= set(kinds), kinds
    for n, kind in enumerate(kinds):                  # zero reg gradient exactly where the hinge is off
        assert bool((ref["dreg"][n] == 0).all()) == (kind in ("inside", "none")), (n, kind)
        assert bool((ref["dreg"][n][inp.lobes[n] == 0] == 0).all())
    if cid == "keep_mixed":
        assert sorted(set(inp.keep.tolist())) == [0.0, 1.0]
        assert not ref["t"][inp.keep == 0].any() and ref["t"][inp.keep > 0].any()
    if cid == "keep_none":
        assert ref["T"] == 0 and not ref["t"].any() and ref["wsum"] == 0.25 * ref["n_in"]
    if cid == "n257":
        r = ref["r"]
        assert kinds[256] == "above" and r[256] > r[:256].max() + 0.1                  # a distinctive r, an active hinge
        lo, hi, w = (float(v) for v in (*inp.targets[256], inp.weight[256]))
        assert ((r[256] - 0.5 * (lo + hi)) ** 2 - 0.25 * (hi - lo) ** 2) / w > 1e3 * R.VALUE_TOL * max(1.0, ref["reg"])
    if cid == "few_inside":
        assert ref["n_in"] * 100 < ref["n_out"]
    if cid == "few_outside":
        assert 0 < ref["n_out"] * 100 < ref["n_in"]
    if cid == "no_outside":
        assert ref["n_out"] == 0
    if cid in ("empty_lobe", "s1"):
        assert kinds[1] == "none" and ref["nm"][1] == 0 and ref["nm"][0] > 0 and ref["nm"][2] > 0
    if cid == "saturation":     # with gout = (0, 1) the saturated class owes exactly 0, inside and outside the lobe
        sat = R.voxel_classes(inp, ref, inp.dense)["saturated"]
        assert bool((ref["dseg"][sat] == 0).all()) and float(np.abs(ref["dreg"][sat]).max()) > 0.0


def test_shapes_reach_what_they_name():
    S = {cid: R.CASES[cid].S for cid in R.SHAPE_CASES}
    assert sorted(S.values()) == [1, 255, 257, 8191, 8192, 8193, 3 * 8192 + 5] and all(R.CASES[c].N == 3 for c in S)
    chunks = lambda s: -(-s // R.LCHUNK)
    assert [chunks(s) for s in sorted(S.values())] == [1, 1, 1, 1, 1, 2, 4] and 8193 - R.LCHUNK == 1
    for cid in R.REGIME_CASES + R.EDGE_CASES + ["refined"]:
        assert R.CASES[cid].S % R.LCHUNK not in (0,) and chunks(R.CASES[cid].S) > 1       # a ragged chunk after a full one
    assert R.CASES["n257"].N == 257 > 256
    cap = R.CASES["cap"]
    assert cap.N == 1 and -(-cap.S // R.BWD_PER_BLOCK) == R.BWD_CAP + 1 and cap.S < 2 ** 24 and cap.gouts == ((2.0, 1.0),)
    assert sorted(set(R.CASES["unaligned"].shifts.values())) == [1, 2, 3]
    assert set(R.CASES["hinge"].gouts) == {(2.0, 1.0), (1.0, 0.0), (0.0, 1.0), (-0.37, 3.0)}


# ------------------------------------------------------------------------------------------------ sensitivity
def _verdicts(cid, perturb, gout):
    """(old whole-tensor bound passes, per-class comparator passes, |value error| / value bound of (reg, seg)) for the
    perturbed restatement taken as the kernel's result."""
    inp, ref = R.build(cid), R.reference(cid)
    bad = R.restate(inp, perturb=perturb)
    want = R.expected_grads(ref, gout, False)["ddense"]
    got = R.expected_grads(bad, gout, False)["ddense"].astype(np.float32)
    classes = R.voxel_classes(inp, ref, inp.dense)
    return (R.old_bound_ok(got, want), R.grad_ok(got, want, classes),
            (R.value_ratio(bad["reg"], ref["reg"]), R.value_ratio(bad["seg"], ref["seg"])))


def test_unperturbed_reference_passes_its_own_comparators():
    for cid in R.REGIME_CASES:
        inp, ref = R.build(cid), R.reference(cid)
        for gout in R.CASES[cid].gouts:
            want = R.expected_grads(ref, gout, False)["ddense"]
            assert R.grad_ok(want.astype(np.float32), want, R.voxel_classes(inp, ref, inp.dense)), (cid, gout)


def test_coefficient_errors_pass_the_old_bound_and_fail_the_new_one():
    """The gap these tests close.  c_out scaled by 1.01 on `few_inside` (94 lobe voxels among 24579: an outside
    gradient is g1 p / n_out, hundreds of times below the lobe's) and c_boot scaled by 1.01 on `few_outside` with
    gout = (0, 1) (12 outside voxels: the tensor's maximum is an outside gradient g1 p / n_out, thousands of times above
    the lobe's) both satisfy max |got - ref| <= 1e-4 max |ref| over the whole tensor, the only gradient bound of
    tests/test_gpu_train_step.py, and both fail the per-class comparator."""
    old, new, _ = _verdicts("few_inside", "c_out", (2.0, 1.0))
    assert old and not new
    old, new, _ = _verdicts("few_outside", "c_boot", (0.0, 1.0))
    assert old and not new


@pytest.mark.parametrize("perturb", ["c_out", "c_boot", "alpha"])
def test_coefficient_errors_fail_on_regime_cases(perturb):
    failed = [cid for cid in R.REGIME_CASES if not all(_verdicts(cid, perturb, g)[1] for g in R.CASES[cid].gouts)]
    assert failed, perturb
    if perturb != "alpha":      # a coefficient of every voxel of a class: no regime case lets it through
        assert failed == R.REGIME_CASES, failed


def test_dropped_sample_256_shows_in_reg_state_and_gradient():
    inp, ref = R.build("n257"), R.reference("n257")
    old, new, (reg_ratio, _) = _verdicts("n257", "drop_sample_256", (2.0, 1.0))
    assert not new and reg_ratio > 100.0
    bad = R.restate(inp, perturb="drop_sample_256")
    assert bad["nm"][256] == 0 and ref["nm"][256] > 0 and bad["n_in"] < ref["n_in"]
    assert float(np.abs(ref["dreg"][256]).max()) > 0.0 and float(np.abs(bad["dreg"][256]).max()) == 0.0


@pytest.mark.parametrize("cid", ["s8193", "hinge", "s24581"])
def test_dropped_last_element_of_a_ragged_chunk_fails(cid):
    """The last element of every sample is outside the lobe: n_out, the outside sum and that voxel's gradient move."""
    ref, bad = R.reference(cid), R.restate(R.build(cid), perturb="drop_last_element")
    assert bad["n_out"] == ref["n_out"] - R.CASES[cid].N
    _, new, _ = _verdicts(cid, "drop_last_element", (2.0, 1.0))
    assert not new
    assert np.float32(bad["n_out"]) != np.float32(ref["n_out"])           # the exact state comparison sees it too
