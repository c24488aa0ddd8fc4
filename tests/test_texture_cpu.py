"""CPU-side checks of the lesion texture report: the C ABI surface of csrc/texture.hip and its plan function (no kernel runs), the
numpy restatement (tests/texture_restatement.py) against a textbook table and direct pair counts, and the host arithmetic of
dram_amd/texture.py on hand-made tables."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import texture_cases as TC
import texture_restatement as TR

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ENTRY_ARGS = {"dram_label_glcm_plan": 4, "dram_label_glcm": 14}


def _header_functions():
    src = open(os.path.join(ROOT, "include", "dram_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(?:int|size_t|const char\*)\s+(dram_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        args = m.group(2).strip()
        out[m.group(1)] = 0 if args in ("", "void") else len(args.split(","))
    return out


def test_entry_points_are_exported_with_the_declared_argument_counts():
    from dram_amd import _lib
    decl = _header_functions()
    lib = ctypes.CDLL(os.path.join(ROOT, "bodyct-dram_amd", "libdram_hip.so"))
    for name, nargs in ENTRY_ARGS.items():
        assert hasattr(lib, name), f"libdram_hip.so does not export {name}"
        assert decl[name] == nargs and len(_lib.SIGNATURES[name][1]) == nargs, name
    import dram_amd
    for name in ("label_glcm", "glcm_features", "lesion_texture"):
        assert callable(getattr(dram_amd, name)) and name in dram_amd.__all__
    import inspect
    params = inspect.signature(dram_amd.lesion_report).parameters
    assert "texture" in params and params["texture"].default is False
    from dram_amd import texture as T
    assert T.OFFSETS == TR.OFFSETS and len(T.OFFSETS) == 13
    assert list(T.OFFSETS) == sorted((dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) > (0, 0, 0))


def test_plan_needs_no_gpu_and_refuses_what_the_entry_refuses():
    plan = TC.plan
    assert plan(0, 5, 16) == 0 and plan(1, 5, 16) == 0                       # the lobe map at 16 levels: 16640 words
    assert plan(0, 5, 32) == 1 and plan(1, 32, 16) == 1 and plan(1, 32, 32) == 1
    assert plan(1, 7, 16) == 0 and plan(1, 8, 16) == 1                       # the seam: 24576 words
    assert plan(1, 1, 32) == 0 and plan(1, 2, 32) == 1 and plan(0, 255, 2) == 0
    for d in (1, 2, 3, 4):
        assert plan(1, 5, 16, d) == 0 and plan(1, 8, 16, d) == 1             # the distance does not move it
    top = ((1 << 31) - 1) // (13 * 4)
    assert plan(1, top, 2) == 1 and plan(1, top + 1, 2) < 0
    for args in ((0, 0, 16, 1), (1, -1, 16, 1), (0, 256, 16, 1), (2, 5, 16, 1), (-1, 5, 16, 1), (1, 5, 1, 1), (1, 5, 33, 1), (1, 5, 0, 1),
                 (1, 5, 16, 0), (1, 5, 16, 5), (1, 5, 16, -1), (1, 1 << 21, 32, 1)):
        assert plan(*args) < 0, args


def test_argument_errors_are_reported_without_a_gpu():
    """Every check comes before the first launch, so the refusals answer on a machine without a GPU (dummy non-null pointers)."""
    from dram_amd import _lib
    q = 16

    def glcm(scan=q, labels=q, kind=0, mask=None, n=5, lo=-1000, width=75, levels=16, distance=1, out=q, D=3, H=4, W=5):
        return _lib.lib.dram_label_glcm(scan, labels, kind, mask, n, lo, width, levels, distance, out, D, H, W, None)

    err = lambda: _lib.lib.dram_last_error()
    for null in ("scan", "labels", "out"):
        assert glcm(**{null: None}) == -1 and b"null" in err(), null
    for kw in (dict(n=0), dict(n=-2), dict(kind=0, n=256), dict(kind=2), dict(kind=-1), dict(levels=1), dict(levels=33), dict(levels=0),
               dict(distance=0), dict(distance=5), dict(distance=-1), dict(kind=1, n=1 << 21, levels=32)):
        assert glcm(**kw) == -1 and b"levels in 2..32" in err(), kw
    assert glcm(width=0) == -1 and b"width" in err() and glcm(width=-75) == -1
    for axis in ("D", "H", "W"):
        assert glcm(**{axis: 0}) == -1 and glcm(**{axis: -1}) == -1 and glcm(**{axis: 32769}) == -1 and b"32768" in err(), axis
    assert glcm(D=2048, H=1024, W=1024) == -1 and b"2^31" in err()
    assert glcm(scan=17) == -1 and b"misaligned" in err()
    assert glcm(kind=1, labels=18) == -1 and b"misaligned" in err()
    assert glcm(kind=1, labels=17) == -1


def test_restatement_on_haralicks_example():
    """Haralick, Shanmugam and Dinstein (1973), figure 3: the horizontal table of a 4 x 4 image with four grey levels."""
    image = np.array([[[0, 0, 1, 1], [0, 0, 1, 1], [0, 2, 2, 2], [2, 2, 3, 3]]], dtype=np.int16)
    t = TR.glcm(image, np.ones(image.shape, np.uint8), 1, None, levels=4, lo=0, width=1, distance=1)
    assert t.shape == (1, 13, 4, 4) and t.dtype == np.int64
    c = t[0, 0]
    assert (c + c.T).tolist() == [[4, 2, 1, 0], [2, 4, 0, 0], [1, 0, 6, 1], [0, 0, 1, 2]]
    assert np.all(t[0, 4:] == 0)                                             # one plane: nothing along z
    assert (t[0, 2] + t[0, 2].T).tolist() == [[6, 0, 2, 0], [0, 4, 2, 0], [2, 2, 2, 2], [0, 0, 2, 0]]      # the vertical table of the paper
    f = TR.features_of(c)
    assert f["pairs"] == 12 and math.isclose(f["asm"], 84 / 576, rel_tol=1e-15) and math.isclose(f["contrast"], 14 / 24, rel_tol=1e-15)
    from dram_amd.texture import glcm_features
    g = glcm_features(t, per_direction=True)["per_direction"]
    assert g["pairs"][0, 0] == 12 and math.isclose(g["asm"][0, 0], 84 / 576, rel_tol=1e-15) and math.isclose(g["contrast"][0, 0], 14 / 24, rel_tol=1e-15)


def test_restatement_grey_levels_clamp():
    v = np.array([-32768, -1001, -1000, -926, -925, 124, 125, 199, 200, 32767], dtype=np.int16)
    assert TR.grey_levels(v, -1000, 75, 16).tolist() == [0, 0, 0, 0, 1, 14, 15, 15, 15, 15]
    assert TR.grey_levels(v, -1000, 75, 2).tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 1, 1]


@pytest.mark.parametrize("shape,distance", [((3, 4, 5), 1), ((5, 17, 66), 1), ((5, 17, 66), 2), ((5, 17, 66), 4), ((4, 4, 9), 4), ((1, 1, 7), 2)])
def test_restatement_pair_counts_of_a_full_box(shape, distance):
    rng = np.random.default_rng(3)
    scan = rng.integers(-1200, 400, size=shape).astype(np.int16)
    t = TR.glcm(scan, np.ones(shape, np.int32), 1, None, 16, -1000, 75, distance)
    D, H, W = shape
    pairs = t.sum(axis=(2, 3))[0].tolist()
    assert pairs == TC.box_pairs(shape, distance)
    assert pairs[0] == D * H * max(0, W - distance) and pairs[2] == D * max(0, H - distance) * W and pairs[8] == max(0, D - distance) * H * W
    assert pairs[12] == max(0, D - distance) * max(0, H - distance) * max(0, W - distance) == pairs[4]
    # the marginal of direction 0 is the level histogram of the voxels that have a neighbour at +x
    g = TR.grey_levels(scan, -1000, 75, 16)
    assert t[0, 0].sum(axis=1).tolist() == np.bincount(g[:, :, :max(0, W - distance)].reshape(-1), minlength=16).tolist()


def test_restatement_respects_labels_and_mask():
    c = TC.case("odd")
    lab, scan, mask = c["labels"], c["scan"], c["mask"]
    whole, masked = TC.expected("odd", 3, 16, 1, False), TC.expected("odd", 3, 16, 1, True)
    assert np.all(masked <= whole) and masked.sum() < whole.sum()
    # direction 8, (1,0,0), by a direct loop
    direct = np.zeros((3, 16, 16), np.int64)
    g = TR.grey_levels(scan, -1000, 75, 16)
    for z, y, x in np.ndindex(lab.shape[0] - 1, lab.shape[1], lab.shape[2]):
        k = int(lab[z, y, x])
        if 1 <= k <= 3 and lab[z + 1, y, x] == k and mask[z, y, x] and mask[z + 1, y, x]:
            direct[k - 1, g[z, y, x], g[z + 1, y, x]] += 1
    assert np.array_equal(masked[:, 8], direct)
    assert np.array_equal(TC.expected("odd", 8, 16, 1, False)[:3], whole)    # raising n adds rows and changes none


def test_features_of_hand_made_tables():
    from dram_amd.texture import FEATURES, glcm_features
    levels = 8
    t = np.zeros((3, 13, levels, levels), np.int64)
    t[0, :, 5, 5] = 1000                                                     # a constant region
    # a 3-D checkerboard of levels 2 and 6 in one label: axis directions pair 2 with 6, face diagonals pair equal levels
    axis, face = (0, 2, 8), (1, 3, 5, 7, 9, 11)
    for d in axis:
        t[1, d, 2, 6] = t[1, d, 6, 2] = 50
    for d in face:
        t[1, d, 2, 2] = t[1, d, 6, 6] = 40
    f = glcm_features(t, per_direction=True)
    per = f["per_direction"]
    assert f["pairs"].tolist() == [13000, 3 * 100 + 6 * 80, 0] and f["pairs"].dtype == np.int64
    assert f["asm"][0] == 1.0 and f["entropy"][0] == 0.0 and math.isnan(f["correlation"][0]) and f["contrast"][0] == 0.0
    assert f["homogeneity"][0] == 1.0 and f["max_probability"][0] == 1.0 and f["mean_level"][0] == 5.0 and f["dissimilarity"][0] == 0.0
    assert np.all(np.isnan(per["correlation"][0]))
    for d in axis:
        assert per["contrast"][1, d] == 16.0 and per["dissimilarity"][1, d] == 4.0 and per["correlation"][1, d] == -1.0
        assert per["asm"][1, d] == 0.5 and per["entropy"][1, d] == 1.0 and per["mean_level"][1, d] == 4.0
    for d in face:
        assert per["contrast"][1, d] == 0.0 and per["correlation"][1, d] == 1.0 and per["homogeneity"][1, d] == 1.0
    for d in (4, 6, 10, 12):                                                 # no pairs along the space diagonals
        assert per["pairs"][1, d] == 0 and all(math.isnan(per[k][1, d]) for k in FEATURES)
    assert math.isclose(f["contrast"][1], 3 * 16.0 / 9, rel_tol=1e-15)       # the mean over the nine directions with pairs
    assert f["pairs"][2] == 0 and all(math.isnan(f[k][2]) for k in FEATURES)
    assert sorted(f) == sorted(("pairs", "per_direction") + FEATURES) and sorted(per) == sorted(("pairs",) + FEATURES)
    empty = glcm_features(np.zeros((0, 13, 16, 16), np.int64))
    assert all(v.shape == (0,) for v in empty.values())
    with pytest.raises(ValueError):
        glcm_features(np.zeros((2, 13, 4, 5), np.int64))


def test_features_match_the_independent_arithmetic():
    from dram_amd.texture import FEATURES, glcm_features
    t = TC.expected("tiles", 5, 16, 1, True)
    got, ref = glcm_features(t), TR.features(t)
    assert np.array_equal(got["pairs"], ref["pairs"])
    for k in FEATURES:
        assert np.allclose(got[k], ref[k], rtol=1e-12, atol=0, equal_nan=True), k


def test_python_entry_checks_its_arguments_before_any_launch():
    from dram_amd.texture import label_glcm
    scan, lab = np.zeros((2, 3, 4), np.int16), np.ones((2, 3, 4), np.uint8)
    assert label_glcm(scan, lab, 0).shape == (0, 13, 16, 16) and label_glcm(scan, lab, 0, levels=4).dtype == np.int64
    for kw in (dict(levels=1), dict(levels=33), dict(distance=0), dict(distance=5), dict(width=0), dict(lo=1 << 31)):
        with pytest.raises(ValueError):
            label_glcm(scan, lab, 3, **kw)
