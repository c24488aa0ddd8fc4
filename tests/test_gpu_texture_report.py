"""dram_amd/texture.py on the device: `label_glcm` and `lesion_texture` against the restatement (equal integers, and the
restatement's own feature arithmetic to 1e-12: both are fp64 on the same integers), and the `texture=` keyword of
`lesion_report`."""
import numpy as np
import pytest
import torch

import texture_restatement as TR

pytestmark = pytest.mark.gpu


def _planted():
    """24 x 40 x 48: three lesions of different texture -- flat, noisy, striped -- and a speck below the volume filter, over two
    lobes; the parenchyma mildly noisy."""
    shape = (24, 40, 48)
    rng = np.random.default_rng(11)
    z, y, x = np.meshgrid(*(np.arange(s, dtype=np.float64) for s in shape), indexing="ij")
    scan = rng.integers(-900, -800, size=shape)
    mask = np.zeros(shape, dtype=np.uint8)
    bodies = (((7, 10, 11), (4, 6, 7)), ((15, 26, 34), (5, 7, 8)), ((8, 30, 12), (4, 5, 6)), ((21, 5, 40), (1, 1, 1)))
    fill = (np.full(shape, -500), rng.integers(-750, 50, size=shape), np.where(x.astype(np.int64) % 4 < 2, -650, -100), np.full(shape, -300))
    for ((cz, cy, cx), (rz, ry, rx)), values in zip(bodies, fill):
        inside = ((z - cz) / rz) ** 2 + ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0
        mask[inside] = 1
        scan = np.where(inside, values, scan)
    lobe = np.where(x < 24, 1, 2).astype(np.uint8)
    lobe[:, :2, :] = 0
    return scan.astype(np.int16), mask, lobe, (2.0, 0.8, 0.8)


def _assert_features_close(got, ref, where):
    assert np.array_equal(got["pairs"], ref["pairs"]), where
    for key in TR.FEATURES:
        a, b = np.asarray(got[key], dtype=np.float64), np.asarray(ref[key], dtype=np.float64)
        assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)), (where, key)
        assert np.allclose(a, b, rtol=1e-12, atol=0, equal_nan=True), (where, key, a, b)


def test_label_glcm_and_lesion_texture_match_the_restatement():
    from dram_amd import label_glcm, lesion_report, lesion_texture
    scan, mask, lobe, spacing = _planted()
    labels = lesion_report(mask, lobe, spacing, min_volume_mm3=20.0)["labels"]
    lab_h = labels.cpu().numpy()
    assert lab_h.max() == 3
    for kw in (dict(), dict(levels=32, lo=-1024, width=40, distance=2), dict(levels=2, lo=-400, width=1)):
        got = label_glcm(torch.from_numpy(scan).cuda(), labels, 3, **kw)
        ref = TR.glcm(scan, lab_h, 3, **kw)
        assert got.dtype == np.int64 and got.shape == ref.shape and np.array_equal(got, ref), kw
        _assert_features_close(lesion_texture(scan, lab_h, 3, **kw), TR.features(ref), kw)      # host arrays go in as they are
    f = lesion_texture(scan, lab_h, 3)
    flat, noisy, striped = (int(lab_h[p]) - 1 for p in ((7, 10, 11), (15, 26, 34), (8, 30, 12)))
    assert sorted((flat, noisy, striped)) == [0, 1, 2]
    assert f["asm"][flat] == 1.0 and f["entropy"][flat] == 0.0 and np.isnan(f["correlation"][flat])
    assert f["entropy"][noisy] > f["entropy"][striped] > 0.0 and f["contrast"][striped] > f["contrast"][flat]
    per = lesion_texture(scan, lab_h, 3, per_direction=True)["per_direction"]
    assert per["contrast"][striped, 2] == 0.0 and per["contrast"][striped, 8] == 0.0 and per["contrast"][striped, 0] > 0.0   # stripes run along y and z
    # a uint8 label volume with a mask, and the empty call
    got = label_glcm(scan, lobe, 2, mask=mask)
    assert np.array_equal(got, TR.glcm(scan, lobe, 2, mask))
    assert label_glcm(scan, lab_h, 0).shape == (0, 13, 16, 16) and lesion_texture(scan, lab_h, 0)["asm"].shape == (0,)
    with pytest.raises(ValueError, match="uint8 or int32"):
        label_glcm(scan, lab_h.astype(np.int64), 3)
    with pytest.raises(ValueError, match="int16"):
        label_glcm(scan.astype(np.int32), lab_h, 3)
    with pytest.raises(ValueError, match="same shape"):
        label_glcm(scan[1:], lab_h, 3)


def test_lesion_report_with_texture():
    from dram_amd import label_glcm, lesion_report
    from dram_amd.texture import glcm_features
    scan, mask, lobe, spacing = _planted()
    kw = dict(connectivity=1, min_volume_mm3=20.0)
    plain = lesion_report(mask, lobe, spacing, scan=scan, **kw)
    assert "texture" not in plain and plain["n_lesions"] == 3
    rep = lesion_report(mask, lobe, spacing, scan=scan, texture=True, **kw)
    assert sorted(rep) == sorted(list(plain) + ["texture"])
    for key in plain:                                                                  # every other key as without the keyword
        if key == "density":
            continue
        if isinstance(plain[key], torch.Tensor):
            assert torch.equal(rep[key], plain[key]), key
        elif isinstance(plain[key], np.ndarray):
            assert np.array_equal(rep[key], plain[key]), key
        else:
            assert rep[key] == plain[key], key
    for key, v in plain["density"]["lesions"].items():
        assert np.array_equal(rep["density"]["lesions"][key], v, equal_nan=True), key
    labels = rep["labels"].cpu().numpy()
    kept = rep["mask"].cpu().numpy()
    tex = rep["texture"]
    ref = TR.features(TR.glcm(scan, labels, 3))
    _assert_features_close(tex["lesions"], ref, "lesions")
    for i in range(3):                                                                 # the order of volumes_ml
        voxels = np.count_nonzero(labels == i + 1)
        assert abs(voxels * float(np.prod(spacing)) / 1000.0 - rep["volumes_ml"][i]) <= 1e-12 * rep["volumes_ml"][i]
        assert tex["lesions"]["pairs"][i] == TR.glcm(scan, labels == i + 1, 1).sum()
    assert sorted(tex["lobes"]) == sorted(rep["lobes"]) == [1, 2]
    whole, inside = glcm_features(label_glcm(scan, lobe, 2)), glcm_features(label_glcm(scan, lobe, 2, mask=kept))
    whole_ref, inside_ref = TR.features(TR.glcm(scan, lobe, 2)), TR.features(TR.glcm(scan, lobe, 2, kept))
    for v in (1, 2):
        for part, got, ref_ in (("parenchyma", whole, whole_ref), ("lesion", inside, inside_ref)):
            row = tex["lobes"][v][part]
            assert sorted(row) == sorted(("pairs",) + TR.FEATURES)
            for key in row:
                assert np.array_equal(row[key], got[key][v - 1], equal_nan=True), (v, part, key)
                assert np.isclose(row[key], ref_[key][v - 1], rtol=1e-12, atol=0, equal_nan=True), (v, part, key)
    # the settings reach every table
    custom = lesion_report(mask, lobe, spacing, scan=scan, texture=dict(levels=8, lo=-900, width=100, distance=2), **kw)["texture"]
    _assert_features_close(custom["lesions"], TR.features(TR.glcm(scan, labels, 3, None, 8, -900, 100, 2)), "custom")
    assert np.isclose(custom["lobes"][2]["lesion"]["contrast"], TR.features(TR.glcm(scan, lobe, 2, kept, 8, -900, 100, 2))["contrast"][1], rtol=1e-12)
    with pytest.raises(ValueError, match="scan"):
        lesion_report(mask, lobe, spacing, texture=True, **kw)
    with pytest.raises(ValueError, match="levels, lo, width and distance"):
        lesion_report(mask, lobe, spacing, scan=scan, texture=dict(bins=4), **kw)
    empty = lesion_report(np.zeros_like(mask), lobe, spacing, scan=scan, texture=True)["texture"]
    assert empty["lesions"]["pairs"].shape == (0,) and empty["lobes"][1]["lesion"]["pairs"] == 0 and np.isnan(empty["lobes"][1]["lesion"]["asm"])
