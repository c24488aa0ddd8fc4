"""LobeInference(refine=...): the guided-filter refinement of the finished heat map inside the inference entry point.  The slim
model and the small synthetic scan of tests/test_gpu_tta.py.  The filter itself is held to its definition by
tests/test_gpu_guided.py; here: refine=None is the path as it was, refine=True adds keys and changes none, and every new key is
what its definition says, from the pieces it is defined by."""
import functools

import numpy as np
import pytest
import torch

import tta_cases as T

pytestmark = pytest.mark.gpu
R = T.SCAN_R

PLAIN_KEYS = {"htp", "mask", "threshold", "lesion_ratio", "ctss", "chunks", "input"}
POST_KEYS = {"mask_post", "threshold_scan", "iou", "dice", "iou_post", "dice_post", "curves", "curves_post"}
REFINE_KEYS = {"htp_refined", "threshold_refined", "mask_refined"}
REFINE_POST_KEYS = {"mask_refined_post", "iou_refined", "dice_refined", "iou_refined_post", "dice_refined_post", "curves_refined",
                    "curves_refined_post"}


@functools.lru_cache(maxsize=None)
def slim():
    return T.slim_model().cuda().eval()                          # shared, never modified


@functools.lru_cache(maxsize=None)
def labels():
    """(lesion, vessel) uint8: the bright voxels of the lobes as the reference mask, a sparse pattern as the vessel mask."""
    scan, lobe, _ = T.scan_inputs()
    lesion = ((scan > -600) & (lobe > 0)).astype(np.uint8)
    vessel = (np.random.default_rng(9).integers(0, 7, size=scan.shape) == 0).astype(np.uint8)
    assert lesion.sum() > 100
    return lesion, vessel


def same(a, b):
    if isinstance(a, torch.Tensor):
        return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8) if a.dtype != torch.uint8 else a,
                                                                         b.view(torch.uint8) if b.dtype != torch.uint8 else b)
    if isinstance(a, dict):
        return set(a) == set(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b, equal_nan=True)
    return a == b or (isinstance(a, float) and np.isnan(a) and np.isnan(b))


def host_overlap(mask, lesion):
    m, l = mask.cpu().numpy() > 0, lesion > 0
    s = 1e-5
    inter = float((m & l).sum())
    return (inter + s) / (float((m | l).sum()) + s), (2.0 * inter + s) / (float(m.sum()) + float(l.sum()) + s)


def test_refine_none_is_the_path_as_it_was_and_refine_adds_only_keys():
    from dram_amd.inference import LobeInference
    scan, lobe, spacing = T.scan_inputs()
    lesion, vessel = labels()
    kw = dict(vessel=vessel, lesion=lesion, curves=64)
    plain = LobeInference(slim(), resample_size=R).run(scan, lobe, spacing)
    assert set(plain) == PLAIN_KEYS
    none = LobeInference(slim(), resample_size=R, refine=None).run(scan, lobe, spacing, **kw)
    assert set(none) == PLAIN_KEYS | POST_KEYS
    res = LobeInference(slim(), resample_size=R, refine=True).run(scan, lobe, spacing, **kw)
    assert set(res) == PLAIN_KEYS | POST_KEYS | REFINE_KEYS | REFINE_POST_KEYS
    for k in none:
        assert same(none[k], res[k]), k
    short = LobeInference(slim(), resample_size=R, refine=True).run(scan, lobe, spacing)
    assert set(short) == PLAIN_KEYS | REFINE_KEYS and same(short["htp_refined"], res["htp_refined"])


def test_values_of_the_new_keys():
    from dram_amd import heatmap_curves, refine_heatmap
    from dram_amd.inference import LobeInference, binary_cam_threshold
    scan, lobe, spacing = T.scan_inputs()
    lesion, vessel = labels()
    opts = dict(radius_mm=2.5, eps=2e-3, window=(-1100, 300), iterations=2)
    res = LobeInference(slim(), resample_size=R, refine=opts).run(scan, lobe, spacing, vessel=vessel, lesion=lesion, curves=64)
    dev = res["htp"].device
    s, l = torch.from_numpy(scan).to(dev), torch.from_numpy(lobe).to(dev)
    want = refine_heatmap(res["htp"], s, l, spacing, **opts)
    assert torch.equal(res["htp_refined"].view(torch.int32), want.view(torch.int32))
    plain = refine_heatmap(res["htp"], s, l, spacing)
    assert not torch.equal(plain, want)                          # the options did arrive
    q = res["htp_refined"].cpu().numpy()
    inside = lobe > 0
    assert not q[~inside].any() and np.isfinite(q).all() and np.abs(q - res["htp"].cpu().numpy())[inside].max() > 1e-4
    hist = np.bincount((np.clip(q[inside], 0.0, 1.0) * 255.0).astype(np.uint8), minlength=256)
    assert res["threshold_refined"] == binary_cam_threshold(hist)
    assert np.array_equal(res["mask_refined"].cpu().numpy() > 0, q > np.float32(res["threshold_refined"]))
    # the gate of mask_post, applied to the refined mask
    gate = (res["mask_post"].cpu().numpy() > 0) | ~(res["mask"].cpu().numpy() > 0)        # where mask is set, mask_post is the gate
    post = res["mask_refined_post"].cpu().numpy() > 0
    m_r = res["mask_refined"].cpu().numpy() > 0
    assert not (post & ~m_r).any()
    both = m_r & (res["mask"].cpu().numpy() > 0)
    assert np.array_equal(post[both], gate[both]) and post.any() and (m_r & ~post).any()
    for tag, mask in (("refined", res["mask_refined"]), ("refined_post", res["mask_refined_post"])):
        iou, dice = host_overlap(mask, lesion)
        assert res["iou_" + tag] == pytest.approx(iou, rel=1e-12) and res["dice_" + tag] == pytest.approx(dice, rel=1e-12)
    n_regions = int(lobe.max())
    cur = heatmap_curves(res["htp_refined"], torch.from_numpy(lesion).to(dev), l, n_regions, None, 64, 16)
    assert same(cur, res["curves_refined"])
    assert not same(res["curves"], res["curves_refined"]) and not same(res["curves_refined"], res["curves_refined_post"])


def test_original_grid():
    from dram_amd.inference import LobeInference, resample_volume
    scan, lobe, spacing = T.scan_inputs()
    lesion, vessel = labels()
    osp, osz = (1.25, 0.8, 0.8), (82, 71, 83)
    res = LobeInference(slim(), resample_size=R, refine=True).run(scan, lobe, spacing, vessel=vessel, lesion=lesion,
                                                                   original_spacing=osp, original_size=osz, curves=32)
    orig = res["original"]
    assert {"htp_refined", "mask_refined", "mask_refined_post"} <= set(orig)
    assert set(orig) == {"mask", "mask_post", "scan", "htp", "lesion", "htp_refined", "mask_refined", "mask_refined_post"}
    assert tuple(orig["htp_refined"].shape) == osz and orig["htp_refined"].dtype == torch.float32
    assert torch.equal(orig["htp_refined"], resample_volume(res["htp_refined"], spacing, osp, osz, "linear"))
    for k in ("mask_refined", "mask_refined_post"):
        assert torch.equal(orig[k], resample_volume(res[k], spacing, osp, osz, "nearest"))
    iou, dice = host_overlap(orig["mask_refined"], orig["lesion"].cpu().numpy())
    assert res["iou_refined"] == pytest.approx(iou, rel=1e-12) and res["dice_refined"] == pytest.approx(dice, rel=1e-12)
    none = LobeInference(slim(), resample_size=R).run(scan, lobe, spacing, vessel=vessel, lesion=lesion, original_spacing=osp,
                                                       original_size=osz, curves=32)
    assert set(none["original"]) == {"mask", "mask_post", "scan", "htp", "lesion"}
    for k in none:
        if k == "original":                                      # the one nested result: its old keys unchanged, three added
            assert all(same(none[k][j], res[k][j]) for j in none[k]), k
        else:
            assert same(none[k], res[k]), k


def test_with_test_time_augmentation():
    from dram_amd import refine_heatmap
    from dram_amd.inference import LobeInference
    scan, lobe, spacing = T.scan_inputs()
    res = LobeInference(slim(), resample_size=R, tta="flip", refine=True).run(scan, lobe, spacing)
    assert REFINE_KEYS | {"spread", "views"} <= set(res)
    dev = res["htp"].device
    want = refine_heatmap(res["htp"], torch.from_numpy(scan).to(dev), torch.from_numpy(lobe).to(dev), spacing)
    assert torch.equal(res["htp_refined"].view(torch.int32), want.view(torch.int32))
    none = LobeInference(slim(), resample_size=R, tta="flip").run(scan, lobe, spacing)
    for k in none:
        assert same(none[k], res[k]), k


def test_with_the_cam_head():
    """The class head on a 6-channel slim model (the recipe of tests/test_gpu_cam_inference.py)."""
    import models
    from dram_amd import refine_heatmap
    from dram_amd.configs import SLIM
    from dram_amd.inference import LobeInference
    torch.manual_seed(3)
    m = models.DC3D(**dict(SLIM, out_ch=6))
    m.init(models.HeNorm(mode="fan_in"))
    with torch.no_grad():
        m.top_layer.weight.mul_(16.0)
        m.top_layer.bias.copy_(torch.tensor([3.186, -2.59, 0.779, -4.838, 0.002, -3.118]))
    m = m.cuda().eval()
    scan, lobe, spacing = T.scan_inputs()
    none = LobeInference(m, resample_size=24, head="cam").run(scan, lobe, spacing)
    res = LobeInference(m, resample_size=24, head="cam", refine=True).run(scan, lobe, spacing)
    assert set(res) == set(none) | REFINE_KEYS
    for k in none:
        assert same(none[k], res[k]), k
    dev = res["htp"].device
    want = refine_heatmap(res["htp"], torch.from_numpy(scan).to(dev), torch.from_numpy(lobe).to(dev), spacing)
    assert torch.equal(res["htp_refined"].view(torch.int32), want.view(torch.int32))


def test_empty_lobe_map():
    from dram_amd.inference import LobeInference
    scan, lobe, spacing = T.scan_inputs()
    res = LobeInference(slim(), resample_size=R, refine=True).run(scan, np.zeros_like(lobe), spacing)
    assert res["chunks"] == [] and res["threshold_refined"] == 0.0
    assert not bool(res["htp_refined"].any()) and not bool(res["mask_refined"].any())
    assert res["htp_refined"].dtype == torch.float32 and res["mask_refined"].dtype == torch.uint8
