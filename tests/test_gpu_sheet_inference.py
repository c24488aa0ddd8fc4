"""LobeInference.sheet: the screenshot sheet of archive_results from a result of run().  The slim model and the small synthetic
scan of tests/test_gpu_tta.py.  The kernels are held to their definition by tests/test_gpu_sheet.py; here: the rows and the
coordinate mask are archive_results', the sheet is the restatement's fed from `res`, an empty mask gives None, and run() is the
path it was."""
import functools

import numpy as np
import pytest
import torch

import sheet_restatement as S
import tta_cases as T
from test_gpu_refine_inference import labels, same, slim

pytestmark = pytest.mark.gpu
R = T.SCAN_R
OSP, OSZ = (1.25, 0.8, 0.8), (82, 71, 83)


@functools.lru_cache(maxsize=None)
def result():
    """One run with everything archive_results draws, on both grids.  Shared, never modified."""
    from dram_amd.inference import LobeInference
    scan, lobe, spacing = T.scan_inputs()
    lesion, vessel = labels()
    inf = LobeInference(slim(), resample_size=R)
    return inf, inf.run(scan, lobe, spacing, vessel=vessel, lesion=lesion, original_spacing=OSP, original_size=OSZ)


def expected(scan, mask, post, lesion, htp, **kw):
    rows = [[(mask, S.MASK)]] + ([[(post, S.MASK)]] if post is not None else []) + ([[(lesion, S.MASK)]] if lesion is not None else [])
    rows.append([(htp, S.UNIT)])
    coord = (mask > 0) | (lesion > 0) if lesion is not None else mask > 0
    geometry = dict(flip_axis=kw.get("flip_axis", 0), zoom_size=kw.get("zoom_size", 360), coord_axis=kw.get("coord_axis", 1))
    ids = S.pick_slices(S.occupancy(coord, **geometry), kw.get("num_slices", 5))
    return ids, S.sheet(scan, rows, ids, alpha=kw.get("alpha", 0.5), colormap=kw.get("colormap", "jet"),
                        sheet_width=kw.get("sheet_width", 1920), **geometry)


def host(t):
    return t.cpu().numpy()


def test_sheet_is_archive_results_sheet():
    inf, res = result()
    scan, _, _ = T.scan_inputs()
    lesion, _ = labels()
    keys = set(res)
    out = inf.sheet(res, scan, lesion)
    ids, ref = expected(scan, host(res["mask"]), host(res["mask_post"]), lesion, host(res["htp"]))
    assert out["slice_ids"] == ids and out["titles"] == ["pred_lesion", "pred_lesion_post", "lesion", "pred_cam"]
    assert out["sheet"].is_cuda and tuple(out["sheet"].shape) == (5 * 360, 1920, 3)
    assert np.array_equal(host(out["sheet"]), ref)
    assert len(out["tiles"]) == 5 and out["tiles"][4][4] == (4 * 360, 60 + 4 * 360, 360, 360)
    assert set(res) == keys
    # options reach result_sheet; without a reference there are three rows and the mask alone chooses the slices
    kw = dict(zoom_size=70, sheet_width=None, coord_axis=0, flip_axis=None, alpha=0.3, colormap="summer", num_slices=4)
    out = inf.sheet(res, scan, **kw)
    ids, ref = expected(scan, host(res["mask"]), host(res["mask_post"]), None, host(res["htp"]), **kw)
    assert out["slice_ids"] == ids and out["titles"] == ["pred_lesion", "pred_lesion_post", "pred_cam"]
    assert np.array_equal(host(out["sheet"]), ref)


def test_sheet_on_the_original_grid():
    inf, res = result()
    orig = res["original"]
    kw = dict(zoom_size=128, sheet_width=700)
    out = inf.sheet(res, None, original=True, **kw)
    ids, ref = expected(host(orig["scan"]), host(orig["mask"]), host(orig["mask_post"]), host(orig["lesion"]), host(orig["htp"]), **kw)
    assert out["slice_ids"] == ids and np.array_equal(host(out["sheet"]), ref)
    assert tuple(out["sheet"].shape) == (5 * 128, 700, 3) and tuple(orig["scan"].shape) == OSZ


def test_plain_run_and_empty_mask():
    from dram_amd.inference import LobeInference
    scan, lobe, spacing = T.scan_inputs()
    inf = LobeInference(slim(), resample_size=R)
    res = inf.run(scan, lobe, spacing)                           # no mask_post, no reference: two rows
    out = inf.sheet(res, scan, zoom_size=64, sheet_width=None)
    ids, ref = expected(scan, host(res["mask"]), None, None, host(res["htp"]), zoom_size=64, sheet_width=None)
    assert out["titles"] == ["pred_lesion", "pred_cam"] and out["slice_ids"] == ids and np.array_equal(host(out["sheet"]), ref)
    empty = inf.run(scan, np.zeros_like(lobe), spacing)
    assert not bool(empty["mask"].any()) and inf.sheet(empty, scan) is None
    with pytest.raises(ValueError, match="original"):
        inf.sheet(res, scan, original=True)


def test_run_is_the_path_it_was():
    """The same keys and bits from run() before and after a sheet was drawn from its result, and `res` itself untouched."""
    from dram_amd.inference import LobeInference
    scan, lobe, spacing = T.scan_inputs()
    lesion, vessel = labels()
    inf = LobeInference(slim(), resample_size=R)
    before = inf.run(scan, lobe, spacing, vessel=vessel, lesion=lesion)
    kept = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in before.items()}
    assert inf.sheet(before, scan, lesion, zoom_size=64, sheet_width=None) is not None
    after = inf.run(scan, lobe, spacing, vessel=vessel, lesion=lesion)
    assert set(before) == set(after) == set(kept)
    for k in kept:
        assert same(kept[k], before[k]) and same(before[k], after[k]), k
    assert "sheet" not in after
