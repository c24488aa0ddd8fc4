"""The three fused IntRegRefineLoss kernels of csrc/loss.hip (loss_partial_kernel, loss_finalize_kernel, loss_bwd_kernel)
through dram_intreg_loss_fwd / dram_intreg_loss_bwd on raw pointers, per regime and past one chunk; a few cases again through
functional.intreg_refine_loss, which must return the same bits.

Cases, inputs, the float64 reference and the comparators: tests/refine_loss_cases.py, checked on the host by
tests/test_refine_loss_cases_cpu.py (input conditions and regime claims of every case; a reference with c_out or c_boot
scaled by 1.01, alpha shifted by 1e-3, sample 256 or the last element of a ragged chunk dropped fails the comparators used
here, the first two while passing the single whole-tensor bound of tests/test_gpu_train_step.py).

Per call: out, state, ddense and drefined are filled with a finite sentinel and every element must have been overwritten;
the workspace (exactly dram_intreg_loss_ws_bytes) is NaN; all of them lie between guard words that must come back
bit-identical.  out[0], out[1] and r_n: |err| <= 2e-5 max(1, |ref|).  n_in, n_out, nm_n: the reference's integers.  alpha and
wsum: float32(fp64 value) bit for bit (functions of the exact counts alone).  Gradients: per voxel class (outside the lobe,
inside with t = 1, inside with t = 0, saturated) |err| <= 1e-4 of that class's own max |ref|; a class whose reference is
identically 0 must be exactly 0.0f.  A second run gives the same bits.  Every case prints `refine-loss-accuracy:` lines,
|err| / bound per quantity, before it asserts (profiles/refine_loss_accuracy.txt is that output of one run)."""
import numpy as np
import pytest
import torch

import refine_loss_cases as R
from test_gpu_onload import DEV, Placed, call, p

pytestmark = pytest.mark.gpu
FILL = -777.25            # what every output holds before the call; no result equals it
NAN = float("nan")


def placed(a, shift):
    return Placed(a.shape, shift=4 * shift, src=torch.from_numpy(np.ascontiguousarray(a)))


def bits(t):
    return t.contiguous().view(torch.int32)


def run(cid, gout, variant):
    """One forward and one backward call.  variant: "absent" (refined and drefined NULL), "distinct" (the case's refined
    tensor), "same" (refined is the pointer of dense, with a drefined buffer that must come back untouched).  Returns the
    outputs as device tensors; guards and coverage are asserted here."""
    from dram_amd import _lib
    c, inp = R.CASES[cid], R.build(cid)
    N, S = c.N, c.S
    sh = lambda name: (c.shifts or {}).get(name, 0)
    dense, lobes, lesions = placed(inp.dense, sh("dense")), placed(inp.lobes, sh("lobes")), placed(inp.lesions, sh("lesions"))
    keep, targets, weight = placed(inp.keep, sh("keep")), placed(inp.targets, sh("targets")), placed(inp.weight, sh("weight"))
    g = placed(np.asarray(gout, dtype=np.float32), sh("gout"))
    refined = placed(inp.refined, sh("refined")) if variant == "distinct" else None
    refined_ptr = p(dense.t) if variant == "same" else p(refined.t) if refined is not None else None
    nstate = _lib.lib.dram_intreg_loss_state_floats(N)
    assert nstate == 4 + 2 * N
    ws_bytes = _lib.lib.dram_intreg_loss_ws_bytes(N, S)
    assert ws_bytes % 8 == 0
    ws = Placed((ws_bytes // 4,), fill=NAN)
    out, state = Placed((2,), shift=4 * sh("out"), fill=FILL), Placed((nstate,), shift=4 * sh("state"), fill=FILL)
    ddense = Placed((N, S), shift=4 * sh("ddense"), fill=FILL)
    drefined = Placed((N, S), shift=4 * sh("drefined"), fill=FILL) if variant != "absent" else None
    call("dram_intreg_loss_fwd", p(dense.t), refined_ptr, p(lobes.t), p(lesions.t), p(keep.t), p(targets.t), p(weight.t),
         R.SMOOTHING, p(out.t), p(state.t), p(ws.t), ws_bytes, N, S)
    call("dram_intreg_loss_bwd", p(dense.t), refined_ptr, p(lobes.t), p(lesions.t), p(keep.t), p(targets.t), p(weight.t),
         p(state.t), p(g.t), R.SMOOTHING, p(ddense.t), None if drefined is None else p(drefined.t), N, S)
    torch.cuda.synchronize()
    for name, o in (("ws", ws), ("out", out), ("state", state), ("ddense", ddense), ("drefined", drefined), ("dense", dense),
                    ("refined", refined), ("lobes", lobes), ("lesions", lesions)):
        assert o is None or o.intact(), f"{cid}: a write outside {name}"
    res = {"out": out.t, "state": state.t, "ddense": ddense.t}
    for name, t in res.items():
        assert bool((t != FILL).all()), f"{cid}: an element of {name} was not written"
    if variant == "distinct":
        assert bool((drefined.t != FILL).all()), f"{cid}: an element of drefined was not written"
        res["drefined"] = drefined.t
    elif variant == "same":
        assert bool((drefined.t == FILL).all()), f"{cid}: drefined was written although refined is dense"
    return res


def same_bits(a, b):
    return a.keys() == b.keys() and all(torch.equal(bits(a[k]), bits(b[k])) for k in a)


def line(cid, tag, name, ratio):
    print(f"refine-loss-accuracy: {cid:18s} {tag:22s} {name:22s} |err|/bound {ratio:.3f}")


def check(cid, gout, variant, res):
    """Every value and gradient of one run against the fp64 reference; prints before it asserts."""
    inp, ref = R.build(cid), R.reference(cid)
    tag = f"{variant} g=({gout[0]:g},{gout[1]:g})"
    N = R.CASES[cid].N
    out, state = res["out"].cpu().numpy(), res["state"].cpu().numpy()
    exp = R.expected_state(ref)
    live = ref["nm"] > 0
    r_got, nm_got = state[4::2], state[5::2]
    ratios = {"reg": R.value_ratio(out[0], ref["reg"]), "seg": R.value_ratio(out[1], ref["seg"]),
              "r_n": max(R.value_ratio(a, b) for a, b in zip(r_got[live], ref["r"][live]))}
    for name, ratio in ratios.items():
        line(cid, tag, name, ratio)
    distinct = variant == "distinct"
    want = R.expected_grads(ref, gout, distinct)
    reports = {}
    for name, w in want.items():
        got = res[name].cpu().numpy()
        classes = R.voxel_classes(inp, ref, inp.refined if name == "drefined" else inp.dense)
        reports[name] = (got, w, classes, R.grad_report(got, w, classes))
        for cls, count, top, err, ratio, _ in reports[name][3]:
            line(cid, tag, f"{name}/{cls}", ratio)
    assert np.isfinite(out).all(), (cid, out)
    assert all(r <= 1.0 for r in ratios.values()), (cid, tag, ratios)
    assert state.size == exp["floats"]
    assert state[2] == exp["n_in"] and state[3] == exp["n_out"] and np.array_equal(nm_got, exp["nm"]), (cid, state[:4])
    assert state[0:1].view(np.int32)[0] == exp["alpha"].view(np.int32), (cid, state[0], exp["alpha"])
    assert state[1:2].view(np.int32)[0] == exp["wsum"].view(np.int32), (cid, state[1], exp["wsum"])
    assert np.isfinite(r_got[live]).all() and np.isnan(r_got[~live]).all() and r_got.size == N
    for name, (got, w, classes, rows) in reports.items():
        assert np.isfinite(got).all(), (cid, name)
        assert all(row[-1] for row in rows), (cid, tag, name, rows)
        m = inp.lobes > 0
        if name == "drefined" or not distinct:      # the seg classes: zero gradient beyond the eps clamp, outside the lobe ...
            assert bool((got[classes["saturated"] & ~m] == 0).all()), (cid, name)
            if gout[0] == 0.0:                      # ... and inside it where no reg term is added
                assert bool((got[classes["saturated"]] == 0).all()), (cid, name)
        if name == "ddense" and (distinct or gout[1] == 0.0):    # reg alone: 0 outside the lobes and where the hinge is off
            off = np.asarray([bool((ref["dreg"][n] == 0).all()) for n in range(N)])
            assert bool((got[~m] == 0).all()) and bool((got[off] == 0).all()), (cid, name)
    return reports


def run_checked(cid, gout, variant="absent"):
    res = run(cid, gout, variant)
    check(cid, gout, variant, res)
    assert same_bits(res, run(cid, gout, variant)), f"{cid}: a second run gives other bits"
    return res


# ------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("cid", R.SHAPE_CASES)
def test_shapes(cid):
    """S = 1, 255, 257, 8191, 8192, 8193 and 3 * 8192 + 5 with N = 3: below, at and one past a forward chunk, a ragged chunk
    after full ones.  At S = 1 sample 1 is its batch's only outside voxel and has no lobe."""
    run_checked(cid, R.GOUTS[0])


# ------------------------------------------------------------------------------------------------ regimes
@pytest.mark.parametrize("cid,gout", [(cid, g) for cid in R.REGIME_CASES for g in R.CASES[cid].gouts],
                         ids=lambda v: v if isinstance(v, str) else f"g{v[0]:g}_{v[1]:g}")
def test_regimes(cid, gout):
    """alpha interior and at both clamps; the hinge below / inside / above its band under every upstream gradient; keep mixed
    and all zero; saturated samples; lobes of a few voxels and lobes that leave a few."""
    res = run_checked(cid, gout)
    ref = R.reference(cid)
    state = res["state"].cpu().numpy()
    want = R.ALPHA_REGIME.get(cid)
    if isinstance(want, float):
        assert state[0] == np.float32(want)
    elif want == "interior":
        assert 0.3 <= state[0] <= 0.7
    if cid == "keep_none":
        assert state[1] == np.float32(0.25 * ref["n_in"])


def test_refined_variants():
    """refined absent, a distinct tensor (ddense carries reg alone, drefined seg alone, each compared on its own) and the
    pointer of dense (bit-identical to absent, the drefined buffer handed in comes back untouched)."""
    absent = run_checked("refined_absent", R.GOUTS[0])
    distinct = run_checked("refined", R.GOUTS[0], "distinct")
    same = run("refined", R.GOUTS[0], "same")
    assert same_bits(absent, same)
    inp = R.build("refined")
    m = torch.from_numpy(inp.lobes > 0)
    assert bool((distinct["ddense"].cpu()[~m] == 0).all())
    assert not torch.equal(bits(distinct["ddense"]), bits(absent["ddense"]))


# ------------------------------------------------------------------------------------------------ laps, cap, alignment
def test_second_lap_of_the_finalise_loop():
    """N = 257: thread 0 of loss_finalize_kernel takes sample 256 in its second lap; that sample's hinge is active and its
    r is above every other's (host test), so losing it moves reg by 1e3 bounds, state[4 + 512], state[5 + 512] and row 256."""
    res = run_checked("n257", R.GOUTS[0])
    ref = R.reference("n257")
    state = res["state"].cpu().numpy()
    assert state[5 + 512] == ref["nm"][256] > 0 and abs(state[4 + 512] - ref["r"][256]) <= R.VALUE_TOL
    assert float(res["ddense"][256].abs().max()) > 0.0


def test_one_past_the_backward_grid_cap():
    """N = 1, S = 4096 * 2048 + 300: the backward grid stops at 4096 blocks and the first 300 threads of the grid take a second
    element; 1025 forward chunks, the last of 300."""
    run_checked("cap", R.GOUTS[0])


def test_unaligned_bases():
    """Every tensor, inputs and outputs, starts 1, 2 or 3 floats past a 16-byte boundary; refined is a distinct tensor."""
    run_checked("unaligned", R.GOUTS[0], "distinct")


# ------------------------------------------------------------------------------------------------ edges
@pytest.mark.parametrize("cid", R.EDGE_CASES)
def test_an_empty_sum_contributes_zero(cid):
    """no_outside: no voxel outside any lobe -- the outside mean is 0 (torch: NaN) and everything is finite.  empty_lobe:
    sample 1 has no lobe while the others do -- it adds nothing to reg, nm_1 = 0, r_1 is NaN (check()), its gradient is the
    outside term's alone and finite."""
    res = run_checked(cid, R.GOUTS[0])
    ref = R.reference(cid)
    if cid == "no_outside":
        assert ref["n_out"] == 0 and float(res["state"][3]) == 0.0
    else:
        assert float(res["state"][5 + 2]) == 0.0 and bool(torch.isfinite(res["ddense"][1]).all())
        assert float(res["ddense"][1].abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------ the autograd wrapper
@pytest.mark.parametrize("cid,variant", [("hinge", "absent"), ("refined", "distinct"), ("refined", "same")])
def test_autograd_wrapper_returns_the_entry_points_bits(cid, variant):
    """functional.intreg_refine_loss on [N, 1, 1, 1, S] tensors: IntRegRefineLossFn allocates, saves and hands over what the
    raw calls above were given, so values and gradients are bit-identical to them (and `refined is dense` takes the
    one-tensor path)."""
    from dram_amd import functional as HF
    c, inp = R.CASES[cid], R.build(cid)
    gout = R.GOUTS[3]
    raw = run(cid, gout, variant)
    if variant == "distinct":
        check(cid, gout, variant, raw)
    t5 = lambda a: torch.from_numpy(a).to(DEV).view(c.N, 1, 1, 1, c.S)
    dense = t5(inp.dense).requires_grad_(True)
    refined = t5(inp.refined).requires_grad_(True) if variant == "distinct" else dense if variant == "same" else None
    out = HF.intreg_refine_loss(dense, t5(inp.lobes), t5(inp.lesions), torch.from_numpy(inp.keep).to(DEV),
                                torch.from_numpy(inp.targets).to(DEV), torch.from_numpy(inp.weight).to(DEV), R.SMOOTHING,
                                refined=refined)
    (gout[0] * out[0] + gout[1] * out[1]).backward()
    torch.cuda.synchronize()
    assert torch.equal(bits(out.detach()), bits(raw["out"]))
    assert torch.equal(bits(dense.grad.view(c.N, c.S)), bits(raw["ddense"]))
    if variant == "distinct":
        assert torch.equal(bits(refined.grad.view(c.N, c.S)), bits(raw["drefined"]))
