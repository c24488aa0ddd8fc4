"""Test-time augmentation of LobeInference end to end on the device against tests/tta_cases.py run_tta_ref (the oracle's
evaluate_scan with the ensemble in the middle; equal to evaluate_scan for the identity view, tests/test_tta_cpu.py).

Heat map: the tolerance of tests/test_gpu_inference.py::test_lobe_inference_matches_oracle (1e-4, the device model against the
oracle's) plus the ensemble's and the resize's derived shares (tta_cases.htp_tol).  Spread: point by point within the bound that
follows from the bound on s^2 (tta_cases.spread_bound_map: var_tol / s where s is not small, sqrt(var_tol) where it is --
the square root of an error near zero is not small), with every probability allowed the same 1e-4."""
import functools
import os

import numpy as np
import pytest
import torch

import tta_cases as T
from oracle import dram_oracle as O
from dram_amd.configs import SLIM, SLIM_ATT

pytestmark = pytest.mark.gpu
R = T.SCAN_R
THREE_VIEWS = (T.IDENTITY, T.CYCLE_VIEW, ((2, 0, 1), (0, 1, 1)))


@functools.lru_cache(maxsize=None)
def slim():
    """(model on the device, params, buffers): shared, never modified."""
    m = T.slim_model()
    params, buffers = O.split_state_dict({k: v.clone() for k, v in m.state_dict().items()})
    return m.cuda().eval(), params, buffers


@functools.lru_cache(maxsize=None)
def reference(views):
    _, params, buffers = slim()
    scan, lobe, spacing = T.scan_inputs()
    return T.run_tta_ref(SLIM, params, buffers, scan, lobe, spacing, views, R)


def check_against(res, ref, lobe, V, tag):
    htp, spread = res["htp"].cpu().numpy(), res["spread"].cpu().numpy()
    assert htp.dtype == np.float32 and spread.dtype == np.float32 and spread.shape == lobe.shape
    e_h = np.abs(htp - ref["htp"]).max() / (T.htp_tol(V) * max(1.0, np.abs(ref["htp"]).max()))
    bound = T.spread_bound_map(ref, lobe, T.e2e_var_tol(V))
    inside = lobe > 0
    e_s = (np.abs(spread.astype(np.float64) - ref["spread"])[inside] / bound[inside]).max()
    big = inside & (ref["spread"] >= T.S_MIN)
    e_big = np.abs(spread - ref["spread"])[big].max() if big.any() else 0.0
    print(f"\ntta-accuracy: end to end {tag} V={V}: htp {e_h:.3f} of htp_tol, spread {e_s:.3f} of its point-wise bound; "
          f"spread range 0..{ref['spread'].max():.4f}, largest error where the reference spread >= 2^-8 ({int(big.sum())} voxels): {e_big:.2e}")
    assert e_h <= 1 and e_s <= 1
    assert (htp[~inside] == 0).all() and (spread[~inside] == 0).all()
    assert abs(res["threshold"] - ref["threshold"]) <= 1.0 / 255.0 + 1e-9


def test_flip_ensemble_matches_the_reference():
    from dram_amd.inference import LobeInference
    model, _, _ = slim()
    scan, lobe, spacing = T.scan_inputs()
    res = LobeInference(model, resample_size=R, tta="flip").run(scan, lobe, spacing)
    assert {"spread", "views", "input", "htp", "mask", "threshold", "lesion_ratio", "ctss", "chunks"} <= set(res)
    assert res["views"] == T.FLIP_VIEWS
    L = len(res["chunks"])
    assert L >= 2 and tuple(res["input"].shape) == (L, 1, R, R, R)
    plain = LobeInference(model, resample_size=R).run(scan, lobe, spacing)
    assert torch.equal(res["input"], plain["input"]) and "spread" not in plain and "views" not in plain
    ref = reference(T.FLIP_VIEWS)
    assert float(ref["spread"].max()) > 1e-3                                 # the views do disagree
    check_against(res, ref, lobe, 8, "flip")
    assert abs(res["lesion_ratio"] - ref["ratio"]) <= T.htp_tol(8) * max(1.0, abs(ref["ratio"]))


def test_identity_view_is_the_plain_run():
    from dram_amd.inference import LobeInference
    model, _, _ = slim()
    scan, lobe, spacing = T.scan_inputs()
    plain = LobeInference(model, resample_size=R).run(scan, lobe, spacing)
    res = LobeInference(model, resample_size=R, tta=[T.IDENTITY]).run(scan, lobe, spacing)
    a, b = res["htp"].cpu().numpy(), plain["htp"].cpu().numpy()
    print(f"\ntta-accuracy: tta=[identity] against tta=None: htp differs by {np.abs(a.astype(np.float64) - b).max() / T.U:.3f} U "
          f"(asked: 2), bit-identical: {np.array_equal(a, b)}")
    assert np.abs(a.astype(np.float64) - b).max() <= 2 * T.U
    assert not bool(res["spread"].any())
    assert abs(res["threshold"] - plain["threshold"]) <= 1.0 / 255.0 + 1e-9


@pytest.mark.parametrize("tta_batch", [5, 4, 1, 64])
def test_three_views_with_a_cycle_in_ragged_batches(tta_batch):
    """Three views, one a 3-cycle with a flip.  The scan has five lobes, so 15 viewed chunks: tta_batch = 5 is one view per
    model call; 4 gives 4 + 4 + 4 + 3 -- the second and third calls straddle two views and the last is ragged --; 1 and 64
    are the two ends."""
    from dram_amd.inference import LobeInference
    model, _, _ = slim()
    scan, lobe, spacing = T.scan_inputs()
    res = LobeInference(model, resample_size=R, tta=THREE_VIEWS, tta_batch=tta_batch).run(scan, lobe, spacing)
    assert len(res["chunks"]) == 5
    check_against(res, reference(THREE_VIEWS), lobe, 3, f"cycle, tta_batch={tta_batch}")


def test_attention_model_flip_ensemble(golden_dir):
    """DC3DATGeneric, built as tests/test_gpu_inference.py::test_lobe_inference_with_attention_model builds it; the golden
    weights allow the oracle's forward, so the reference is run_tta_ref with it."""
    import models
    from dram_amd.inference import LobeInference
    z = np.load(os.path.join(golden_dir, "dc3dat_slim.npz"))
    sd = {k[len("slim_att/sd/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("slim_att/sd/")}
    m = models.DC3DATGeneric(**SLIM_ATT)
    m.load_state_dict(sd)
    params, buffers = O.split_state_dict(sd)
    scan, lobe, spacing = T.scan_inputs()
    res = LobeInference(m.cuda().eval(), resample_size=R, tta="flip").run(scan, lobe, spacing)
    assert bool(torch.isfinite(res["htp"]).all()) and bool(torch.isfinite(res["spread"]).all())
    fwd = lambda t: O.dc3dat_forward(SLIM_ATT, params, buffers, t, training=False, attention=True)[1]
    ref = T.run_tta_ref(SLIM_ATT, params, buffers, scan, lobe, spacing, T.FLIP_VIEWS, R, forward=fwd)
    check_against(res, ref, lobe, 8, "attention model, flip")


def test_cam_head_is_refused():
    from dram_amd.inference import LobeInference
    model, _, _ = slim()
    with pytest.raises(NotImplementedError, match="cam"):
        LobeInference(model, resample_size=R, head="cam", tta="flip")


def test_empty_lobe_map():
    from dram_amd.inference import LobeInference
    model, _, _ = slim()
    scan, lobe, spacing = T.scan_inputs()
    res = LobeInference(model, resample_size=R, tta="flip").run(scan, np.zeros_like(lobe), spacing)
    assert res["chunks"] == [] and res["views"] == T.FLIP_VIEWS
    assert res["spread"].shape == scan.shape and res["spread"].dtype == torch.float32 and not bool(res["spread"].any())
    assert not bool(res["htp"].any()) and not bool(res["mask"].any())
