"""CPU-side checks of the lesion distribution report: the C ABI surface of csrc/distribution.hip and its plan function (no kernel
runs), the numpy restatement (tests/distribution_restatement.py) against a brute-force loop and scipy, and the report arithmetic
of dram_amd/distribution.py on hand-made tables."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import distribution_cases as XC
import distribution_restatement as XR

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ENTRY_ARGS = {"dram_label_depth_plan": 4, "dram_label_depth": 22}


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
    for name in ("lung_depth", "label_depth", "lesion_distribution"):
        assert callable(getattr(dram_amd, name)) and name in dram_amd.__all__
    import inspect
    params = inspect.signature(dram_amd.lesion_report).parameters
    assert {"distribution", "depth", "shells_mm", "zones", "box", "subpleural_mm", "percentiles_permille"} <= set(params)
    assert params["distribution"].default is False


def test_plan_is_monotone_refuses_what_the_entry_refuses_and_needs_no_gpu():
    plan = XC.plan
    for args in ((0, 5, 4096, 6), (0, 5, 0, 0), (1, 3000, 0, 6), (1, 3000, 4096, 0), (0, 255, 4096, 512), (1, 1, 0, 0)):
        assert plan(*args) in (0, 1) and plan(*args) == plan(*args)
    assert plan(0, 5, 4096, 6) == 0 and plan(0, 5, 1024, 6) == 0 and plan(0, 5, 0, 0) == 0        # the lobe map
    assert plan(1, 3000, 0, 6) == 1 and plan(0, 255, 4096, 0) == 1                                # component labels; many labels with a histogram
    for args in ((0, 0, 0, 0), (1, -1, 0, 0), (0, 256, 0, 0), (2, 5, 0, 0), (-1, 5, 0, 0), (1, 5, -1, 0), (1, 5, 4097, 0), (1, 5, 0, -1),
                 (1, 5, 0, 513), (1, (1 << 31) // 4098 + 1, 4096, 0), (1, (1 << 31) // 512 + 1, 0, 512), (1, (1 << 31) // 3 + 1, 0, 0)):
        assert plan(*args) < 0, args
    assert plan(1, (1 << 31) // 4098, 4096, 0) == 1 and plan(1, (1 << 31) // 3, 0, 0) == 1        # the last sizes in range
    # monotone in n, nbins and nzones: once past the LDS regime a larger call never returns to it
    for kind, nbins, nz in ((1, 0, 0), (1, 0, 6), (1, 4096, 0), (0, 4096, 6), (1, 64, 512)):
        n0 = XC.last_n_in_lds(kind, nbins, nz)
        seen = [plan(kind, n, nbins, nz) for n in sorted({1, 2, n0 // 2 + 1, n0, n0 + 1, 2 * n0, 255 if kind == 0 else 100 * n0})
                if not (kind == 0 and n > 255)]
        assert seen == sorted(seen) and seen[0] == 0 and seen[-1] == 1, (kind, nbins, nz)
    for n in (1, 7, 8, 200, 2978, 2979):
        by_bins = [plan(1, n, b, 6) for b in (0, 1, 2, 63, 64, 1000, 4095, 4096)]
        by_zones = [plan(1, n, 64, z) for z in (0, 1, 6, 64, 511, 512)]
        assert by_bins == sorted(by_bins) and by_zones == sorted(by_zones), n
    for name, want in XC.SEAM_REGIMES.items():
        assert XC.regime(name) == want, name
    assert all(XC.regime(name) == 1 for name in XC.names() if name.endswith("/wave") or name in XC.WAVE_ONLY)
    assert all(XC.regime(name) == 0 for name in XC.NAMES_WITHOUT_LIBRARY)


def test_argument_errors_are_reported_without_a_gpu():
    """Every check comes before the first launch, so the error paths answer on a machine without a GPU (dummy non-null
    pointers)."""
    from dram_amd import _lib
    q = 16
    good_box = np.array([0, 3, 0, 4, 0, 5], dtype=np.int32)

    def depth(d=q, labels=q, kind=0, mask=None, n=5, count=q, qsum=q, dmin=q, dmax=q, possum=q, hist=q, bpm=4, nbins=64, zones=q,
              box=good_box, nz=3, ny=2, nx=1, D=3, H=4, W=5):
        return _lib.lib.dram_label_depth(d, labels, kind, mask, n, count, qsum, dmin, dmax, possum, hist, bpm, nbins, zones,
                                         None if box is None else np.ascontiguousarray(box, dtype=np.int32).ctypes.data, nz, ny, nx, D, H, W, None)

    err = lambda: _lib.lib.dram_last_error()
    for null in ("d", "labels", "count", "qsum", "dmin", "dmax", "possum"):
        assert depth(**{null: None}) == -1 and b"null" in err(), null
    assert depth(n=0) == -1 and depth(n=-2) == -1
    assert depth(kind=0, n=256) == -1 and depth(kind=2) == -1 and depth(kind=-1) == -1
    assert depth(nbins=-1) == -1 and depth(nbins=4097) == -1
    for bpm in (0, 3, 5, 32, -4):
        assert depth(bpm=bpm) == -1 and b"bins_per_mm" in err(), bpm
    assert depth(hist=None) == -1 and b"together" in err()
    assert depth(nbins=0) == -1 and b"together" in err()
    for axis in ("nz", "ny", "nx"):
        assert depth(**{axis: 0}) == -1 and depth(**{axis: 9}) == -1 and b"1..8" in err(), axis
    assert depth(zones=None) == -1 and b"zones" in err()                              # zones asked for, no table
    assert depth(zones=None, box=None) == -1                                          # ... nor without a box
    assert depth(zones=q, box=None, nz=1, ny=1, nx=1) == -1                           # one zone and no box: no table to give
    assert depth(zones=None, nz=1, ny=1, nx=1) == -1                                  # a box without a table
    for k in range(3):
        b = good_box.copy()
        b[2 * k] = b[2 * k + 1]
        assert depth(box=b) == -1 and b"box" in err()
        b[2 * k] += 1
        assert depth(box=b) == -1
    assert depth(kind=1, n=(1 << 31) // 66 + 1) == -1                                 # n * (nbins + 2) >= 2^31
    assert depth(kind=1, n=(1 << 31) // 512 + 1, hist=None, nbins=0, nz=8, ny=8, nx=8) == -1
    assert depth(kind=1, n=(1 << 31) // 3 + 1, hist=None, nbins=0) == -1
    assert depth(D=0) == -1 and depth(H=0) == -1 and depth(W=-1) == -1 and depth(D=2048, H=1024, W=1024) == -1 and b"2^31" in err()
    assert depth(d=18) == -1 and b"misaligned" in err()
    assert depth(kind=1, labels=18) == -1 and b"misaligned" in err()


def test_restatement_against_a_brute_force_loop_on_3x4x5():
    rng = np.random.default_rng(7)
    depth = (rng.random((3, 4, 5)) * 6).astype(np.float32)
    depth[0, 0, :5] = (np.inf, np.nan, -1.0, -0.0, 3.0e6)
    depth[1, 1, :3] = (0.25, np.nextafter(np.float32(0.25), np.float32(0)), 4.0)
    labels = rng.integers(-1, 5, size=(3, 4, 5)).astype(np.int32)
    labels[0, 0, :5] = 2
    mask = (rng.random((3, 4, 5)) < 0.8).astype(np.uint8) * np.uint8(200)
    mask[0, 0, :5] = 1
    for m in (None, mask):
        for kw in (dict(bins_per_mm=4, nbins=16, zones=(2, 3, 2), box=(1, 3, 0, 4, 1, 4)), dict(bins_per_mm=1, nbins=0, zones=None),
                   dict(bins_per_mm=16, nbins=4096, zones=(8, 1, 8), box=None)):
            fast, slow = XR.tables(depth, labels, 3, m, **kw), XR.tables_brute(depth, labels, 3, m, **kw)
            for key in XR.KEYS:
                assert (fast[key] is None) == (slow[key] is None), key
                if fast[key] is not None:
                    assert np.array_equal(fast[key], np.asarray(slow[key], dtype=fast[key].dtype)), (key, kw)
    t = XR.tables(depth, labels, 3, None, 4, 16, (1, 1, 1), None)
    assert np.array_equal(t["hist"].sum(axis=1), t["count"]) and np.array_equal(t["zones"][:, 0], t["count"]) and np.all(t["hist"][:, 0] == 0)
    assert t["dmax"][1] == 0x80000000 and t["dmin"][1] < 0x7f800000                  # -0.0 keeps its own pattern, above +inf's
    with np.errstate(invalid="ignore"):
        assert t["count"][1] == np.count_nonzero((labels == 2) & (depth >= 0))       # of inf, NaN, -1, -0.0, 3e6: three count


def test_values_cases_are_what_they_are_meant_to_be():
    for b in XC.BPMS:
        c, t = XC.case(f"values_bpm{b}"), XC.expected(f"values_bpm{b}")
        # label 1: 7 edges and the 6 floats below them, then 3.0e6, 2^21 and the float below it
        assert t["count"].tolist() == [16, 3, 2, 0]                                   # label 3: +inf and -0.0 pass, NaN and -1.0 do not
        h = t["hist"][0]
        assert h[0] == 0 and h[c["nbins"] + 1] == 4                                   # nbins / b itself and the three large values
        assert h[1] == 2 and h[2] == 2 and h[3] == 2 and h[4] == 1 and h[7] == 1 and h[8] == 1 and h[c["nbins"] - 1] == 1 and h[c["nbins"]] == 2
        assert t["hist"][2].tolist() == [0, 1] + [0] * (c["nbins"] - 1) + [1]
        assert t["dmin"][1] == np.float32(0.3).view(np.uint32) and t["dmax"][1] == np.float32(0.7).view(np.uint32)
        assert t["dmax"][2] == 0x80000000 and t["dmin"][2] == 0x7f800000
        assert t["dmin"][3] == 0x7f800000 and t["dmax"][3] == 0 and t["qsum"][3] == 0
        assert t["qsum"][2] == 2 ** 31                                                # +inf clamps to 2^21 mm; -0.0 adds 0
        assert t["qsum"][0] >= 2 * 2 ** 31 + (2 ** 31 - 128)                          # 3.0e6 and 2^21 clamp, the float below 2^21 does not
    assert XC.expected("values_no_hist")["hist"] is None
    assert XC.expected("values_one_bin")["hist"].shape == (4, 3) and XC.expected("values_4096_bins")["hist"].shape == (4, 4098)


def test_zone_cases_are_what_they_are_meant_to_be():
    t = XC.expected("zones_more_than_voxels")
    assert np.count_nonzero(t["zones"].sum(axis=0) == 0) > 0 and np.array_equal(t["zones"].sum(axis=1), t["count"])
    assert XR.axis_zone(np.arange(-2, 8), 1, 4, 8).tolist() == [0, 0, 0, 0, 2, 5, 5, 5, 5, 5]
    assert XR.axis_zone(np.arange(0, 9), 0, 9, 2).tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1]
    assert XR.axis_zone(np.arange(0, 5), 2, 3, 2).tolist() == [0] * 5                 # a box one voxel wide
    one = XC.expected("zones_box_one_voxel")
    assert np.array_equal(one["zones"][:, 0], one["count"]) and np.all(one["zones"][:, 1:] == 0)
    assert np.array_equal(XC.expected("zones_one_with_box")["zones"][:, 0], XC.expected("zones_one_with_box")["count"])
    inside = XC.expected("zones_box_inside")["zones"].sum(axis=0)
    assert np.all(inside > 0) and inside.size == 12
    assert XC.expected("one_voxel")["zones"] is None and XC.expected("zones_8x8x1")["zones"].shape == (3, 64)


def test_restatement_depth_map_like_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(3)
    lobe = np.zeros((6, 9, 11), dtype=np.uint8)
    lobe[1:5, 1:8, 1:5], lobe[1:6, 2:9, 6:10] = 1, 2
    lobe[rng.random(lobe.shape) < 0.05] = 0
    spacing = (2.0, 0.8, 0.8)
    mine = XR.lung_depth(lobe, spacing)
    ref = ndimage.distance_transform_edt(lobe > 0, sampling=spacing)
    assert mine.dtype == np.float32 and np.all(mine[lobe == 0] == 0) and np.all(mine[lobe > 0] >= np.float32(0.8))
    assert np.all(np.abs(mine.astype(np.float64) - ref) <= np.spacing(ref.astype(np.float32)).astype(np.float64))   # to fp32 rounding
    # and the per-label reductions like scipy's, in fp64 on its side
    labels = lobe.astype(np.int32)
    t = XR.tables(mine, labels, 2, None, 4, 64, None, None)
    index = np.arange(1, 3)
    assert np.array_equal(t["count"], ndimage.sum_labels(np.ones_like(mine), labels, index).astype(np.int64))
    assert np.array_equal(t["dmin"].view(np.float32), np.asarray(ndimage.minimum(mine, labels, index), dtype=np.float32))
    assert np.array_equal(t["dmax"].view(np.float32), np.asarray(ndimage.maximum(mine, labels, index), dtype=np.float32))
    com = np.asarray(ndimage.center_of_mass(np.ones_like(mine), labels, index))
    assert np.allclose(t["possum"] / t["count"][:, None], com, rtol=1e-12, atol=0)
    mean = np.asarray(ndimage.mean(mine.astype(np.float64), labels, index))
    assert np.all(np.abs(t["qsum"] / 1024.0 / t["count"] - mean) <= 1.0 / 1024.0)   # every q truncates by less than 1/1024 mm


def _hand_tables():
    """A 6 x 6 x 6 box lobe with unit spacing, depth = the layer (1, 2, 3 mm) by hand: 152 voxels in the outer shell, 56 in the
    second layer, 8 in the core; bins of 1/4 mm."""
    nbins = 64
    hist = np.zeros((1, nbins + 2), np.int64)
    hist[0, 1 + 4], hist[0, 1 + 8], hist[0, 1 + 12] = 152, 56, 8
    shell, core = np.zeros_like(hist), np.zeros_like(hist)
    shell[0, 1 + 4], core[0, 1 + 12] = 152, 8
    return nbins, hist, shell, core


def test_peripheral_share_on_hand_made_histograms():
    from dram_amd import distribution as X
    nbins, hist, shell, core = _hand_tables()
    for f in (X.peripheral_share, XR.peripheral_share):
        assert f(hist[0], shell[0]) == 1.0 and f(hist[0], core[0]) == 0.0
        assert math.isnan(f(hist[0], np.zeros(nbins + 2, np.int64))) and math.isnan(f(np.zeros(nbins + 2, np.int64), core[0]))
        # equal histograms: 1/3 within the share of the bin that holds the end of the outer third
        rng = np.random.default_rng(12)
        for _ in range(20):
            h = rng.integers(0, 40, size=nbins + 2).astype(np.int64)
            h[0] = 0
            share = f(h, h)
            run = np.cumsum(h)
            e = int(np.nonzero(3 * run >= run[-1])[0][0])
            assert 1.0 / 3.0 <= share + 1e-15 and share - 1.0 / 3.0 <= h[e] / run[-1]
            assert share == run[e] / run[-1]
            assert f(h, 7 * h) == share                                                # a lesion load spread like the lobe itself


def test_report_rows_on_hand_made_tables():
    from dram_amd import distribution as X
    nbins = 8
    t = {"count": np.array([4, 0, 2], np.int64), "qsum": np.array([4 * 1536 + 2, 0, 1024 * 3], np.int64),
         "dmin": np.array([np.float32(0.5).view(np.uint32), 0x7f800000, np.float32(1.5).view(np.uint32)], np.uint32),
         "dmax": np.array([np.float32(2.75).view(np.uint32), 0, np.float32(1.5).view(np.uint32)], np.uint32),
         "possum": np.array([[6, 9, 2], [0, 0, 0], [3, 3, 3]], np.int64),
         "hist": np.array([[0, 0, 0, 1, 0, 0, 2, 0, 0, 1], [0] * 10, [0, 0, 0, 0, 0, 0, 0, 2, 0, 0]], np.int64),
         "zones": np.array([[1, 3], [0, 0], [2, 0]], np.int64)}
    spacing = (2.0, 0.5, 0.25)
    pct = np.array([[2, 5], [X.INT32_MAX] * 2, [6, X.INT32_MAX]], np.int32)
    shells = np.array([[1, 3], [0, 0], [0, 2]], np.int64)
    rows = X.rows_from_tables(t, spacing, 4, pct, shells)
    assert rows["voxels"].tolist() == [4, 0, 2]
    assert rows["depth_mean_mm"][0] == (4 * 1536 + 2) / 1024.0 / 4.0 and rows["depth_mean_mm"][2] == 1.5 and math.isnan(rows["depth_mean_mm"][1])
    assert rows["depth_min_mm"].dtype == np.float32 and rows["depth_min_mm"].tolist() == [0.5, math.inf, 1.5]
    assert rows["depth_max_mm"].tolist() == [2.75, 0.0, 1.5]
    assert rows["centroid"][0].tolist() == [1.5, 2.25, 0.5] and rows["centroid_mm"][0].tolist() == [3.0, 1.125, 0.125]
    assert np.isnan(rows["centroid"][1]).all() and np.isnan(rows["centroid_mm"][1]).all()                # no division by zero
    assert rows["percentiles_mm"][0].tolist() == [0.5, 1.25] and np.isnan(rows["percentiles_mm"][1]).all()
    assert rows["percentiles_mm"][2].tolist() == [1.5, math.inf]
    assert rows["shell_fraction"][0].tolist() == [0.25, 0.75] and np.isnan(rows["shell_fraction"][1]).all()
    assert rows["zone_fraction"][0].tolist() == [0.25, 0.75] and np.isnan(rows["zone_fraction"][1]).all() and rows["zone_voxels"][2].tolist() == [2, 0]
    # the same rows from the restatement
    for k in range(3):
        ref = XR.row(t, k, spacing, 4, nbins, (), ())
        for key in ("voxels", "depth_mean_mm", "depth_min_mm", "depth_max_mm", "centroid", "centroid_mm", "zone_voxels", "zone_fraction"):
            assert np.array_equal(np.asarray(X.row_of(rows, k)[key]), np.asarray(ref[key]), equal_nan=True), (k, key)
    # centroid and zone of an empty row
    box, zones = (0, 4, 0, 6, 0, 2), (2, 3, 1)
    assert X.centroid_zone(t["possum"][1], t["count"][1], box, zones) is None and XR.centroid_zone(t["possum"][1], 0, box, zones) is None
    # label 0: centroid (1.5, 2.25, 0.5) -> nearest indices (2, 2, 1) (halves upwards) -> zones (1, 1, 0)
    assert X.centroid_zone(t["possum"][0], 4, box, zones) == XR.centroid_zone(t["possum"][0], 4, box, zones) == (1 * 3 + 1) * 1 + 0
    assert X.axis_zone(-5, 1, 4, 8) == 0 and X.axis_zone(9, 1, 4, 8) == 5 and X.axis_zone(2, 1, 4, 8) == 2
    # both lungs: the sums of the lobes' tables, the least minimum and the greatest maximum
    lungs = X.sum_tables(t)
    ref = XR.total(t)
    for key in XR.KEYS:
        assert np.array_equal(lungs[key], ref[key]) and lungs[key].shape[0] == 1, key
    assert lungs["count"][0] == 6 and lungs["qsum"][0] == t["qsum"].sum() and lungs["possum"][0].tolist() == [9, 12, 5]
    assert lungs["dmin"].view(np.float32)[0] == 0.5 and lungs["dmax"].view(np.float32)[0] == 2.75
    assert np.array_equal(lungs["hist"][0], t["hist"].sum(axis=0)) and lungs["zones"][0].tolist() == [3, 3]
    row = X.row_of(X.rows_from_tables(lungs, spacing), 0)
    assert row["voxels"] == 6 and row["depth_mean_mm"] == float(t["qsum"].sum()) / 1024.0 / 6.0
    entry = X.lobe_entry(X.row_of(rows, 0), X.row_of(rows, 2), t["hist"][0], t["hist"][2])
    assert entry["depth_ratio"] == 1.5 / ((4 * 1536 + 2) / 1024.0 / 4.0) and entry["peripheral_share"] == 0.0
    assert math.isnan(X.lobe_entry(X.row_of(rows, 0), X.row_of(rows, 1), t["hist"][0], t["hist"][1])["depth_ratio"])


def test_shell_edges_off_the_bin_grid_are_refused():
    from dram_amd import distribution as X
    assert X.shell_bins((5.0, 10.0, 20.0)) == [20, 40, 80] and X.shell_bins((0.25, 256.0)) == [1, 1024] and X.shell_bins(()) == []
    for bad in ((5.1,), (0.125,), (-1.0,), (256.25,), (10.0, 5.0), (5.0, 5.0), (float("nan"),), tuple(range(1, 17))):
        with pytest.raises(ValueError):
            X.shell_bins(bad)
    assert X.shell_bins((0.125,), bins_per_mm=8) == [1]
    with pytest.raises(ValueError):
        XR.shell_bins((5.1,), 4, 1024)
    # and by the report before anything touches a device
    with pytest.raises(ValueError):
        X.lesion_distribution(np.zeros((2, 2, 2), np.uint8), np.ones((2, 2, 2), np.uint8), (1.0, 1.0, 1.0), shells_mm=(5.1,))
