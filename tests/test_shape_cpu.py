"""CPU-side checks of the lesion shape report: the C ABI surface of csrc/shape.hip and its plan function (no kernel runs), the
numpy restatement (tests/shape_restatement.py) against direct counts, and the host arithmetic of dram_amd/shape.py on analytic
bodies (tables from the restatement)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import shape_cases as SC
import shape_restatement as SR

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ENTRY_ARGS = {"dram_label_shape_plan": 2, "dram_label_shape": 9}
POPCOUNT = np.array([bin(c).count("1") for c in range(256)], dtype=np.int64)


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
    for name in ("label_shape", "crossings", "euler_number", "crofton_weights", "lesion_shape"):
        assert callable(getattr(dram_amd, name)) and name in dram_amd.__all__
    import inspect
    params = inspect.signature(dram_amd.lesion_report).parameters
    assert "shape" in params and params["shape"].default is False


def test_plan_needs_no_gpu_and_refuses_what_the_entry_refuses():
    plan = SC.plan
    assert plan(0, 5) == 0 and plan(1, 5) == 0 and plan(1, 3000) == 1 and plan(0, 255) == 1
    past = SC.first_n_past_lds()
    seen = [plan(1, n) for n in (1, 2, past - 1, past, past + 1, 1000, (1 << 23) - 1)]
    assert seen == sorted(seen) and seen[0] == 0 and seen[-1] == 1
    assert [plan(0, n) for n in (1, past - 1, past, 255)] == [0, 0, 1, 1]                      # the label kind does not move the seam
    for args in ((0, 0), (1, 0), (1, -1), (0, 256), (2, 5), (-1, 5), (1, 1 << 23), (1, (1 << 31) - 1)):
        assert plan(*args) < 0, args


def test_argument_errors_are_reported_without_a_gpu():
    from dram_amd import _lib
    q = 16

    def shape(labels=q, kind=0, n=5, cfg=q, mom=q, D=3, H=4, W=5):
        return _lib.lib.dram_label_shape(labels, kind, n, cfg, mom, D, H, W, None)

    err = lambda: _lib.lib.dram_last_error()
    for null in ("labels", "cfg", "mom"):
        assert shape(**{null: None}) == -1 and b"null" in err(), null
    assert shape(n=0) == -1 and shape(n=-2) == -1 and shape(kind=0, n=256) == -1 and shape(kind=2) == -1 and shape(kind=-1) == -1
    assert shape(kind=1, n=1 << 23) == -1
    for axis in ("D", "H", "W"):
        assert shape(**{axis: 0}) == -1 and shape(**{axis: -1}) == -1 and shape(**{axis: 32769}) == -1 and b"32768" in err(), axis
    assert shape(D=2048, H=1024, W=1024) == -1 and b"2^31" in err()
    assert shape(kind=1, labels=18) == -1 and b"misaligned" in err()


@pytest.mark.parametrize("name", [n for n in SC.names() if n != "grid_stride_i32"])
def test_restatement_counts_every_voxel_eight_times_and_crossings_directly(name):
    from dram_amd import shape as S
    c, t = SC.case(name), SC.expected(name)
    assert np.array_equal((t["cfg"] * POPCOUNT[None, :]).sum(axis=1), 8 * t["mom"][:, 0]) and np.all(t["cfg"][:, 0] == 0)
    lab = np.where((c["labels"] >= 0) & (c["labels"] <= c["n"]), c["labels"], 0)
    assert np.array_equal(t["mom"][:, 0], np.bincount(lab.reshape(-1), minlength=c["n"] + 1)[1:])
    for k in range(min(c["n"], 4)):
        assert S.crossings(t["cfg"][k]) == SR.crossings_direct(lab, k + 1), (name, k)


def _euler(lab):
    from dram_amd import shape as S
    return S.euler_number(SR.tables(lab, 1)["cfg"][0])


def test_euler_number_of_known_bodies():
    solid = np.zeros((6, 6, 6), np.uint8)
    solid[1:4, 1:5, 2:5] = 1
    pair = np.zeros((3, 3, 3), np.uint8)
    pair[0, 0, 0] = pair[1, 1, 1] = 1
    assert _euler(solid) == 1
    assert _euler(SC.case("cavity")["labels"]) == 2
    assert _euler(SC.case("ring")["labels"]) == 0
    assert _euler(pair) == 1                                                                   # 26-adjacency: one component
    assert _euler(SC.case("full_box")["labels"]) == 1
    assert _euler(np.zeros((2, 2, 2), np.uint8)) == 0


def test_crofton_weights():
    from dram_amd import shape as S
    w = S.crofton_weights((1.0, 1.0, 1.0))
    assert w.shape == (13,)
    assert np.all(np.abs(w[:3] - 0.0915558) < 1e-6) and np.all(np.abs(w[3:9] - 0.0739613) < 1e-6) and np.all(np.abs(w[9:] - 0.0703913) < 1e-6)
    for sp in ((1.0, 1.0, 1.0), (2.5, 0.7, 0.7), (5.0, 0.6, 0.6), (1.5, 0.8, 0.9)):
        w = S.crofton_weights(sp)
        assert abs(w.sum() - 1.0) < 1e-12 and np.all(w > 0)
    with pytest.raises(ValueError):
        S.crofton_weights((1.0, 0.0, 1.0))


@pytest.mark.parametrize("spacing,r", [((1.0, 1.0, 1.0), 12.0), ((1.0, 1.0, 1.0), 5.0), ((2.5, 0.7, 0.7), 14.0), ((1.5, 0.8, 0.8), 6.0),
                                       ((5.0, 0.6, 0.6), 15.0)])
def test_surface_estimate_on_digitised_balls(spacing, r):
    """The Crofton estimate against 4 pi r^2; the bound is the analytic value with 1 % (a numpy prototype of the formulas measured
    -0.37 % .. +0.35 % on these five)."""
    from dram_amd import shape as S
    half = [int(math.ceil(r / s)) + 2 for s in spacing]
    shape = tuple(2 * h + 1 for h in half)
    centre = (half[0] + 0.3, half[1] + 0.1, half[2] + 0.45)
    row = S.rows_from_tables(SR.tables(SR.ball(shape, centre, r, spacing), 1), spacing)[0]
    true = 4.0 * math.pi * r * r
    print(f"ball r={r} spacing={spacing}: area {row['area_mm2'] / true - 1:+.4%}, faces {row['area_faces_mm2'] / (1.5 * true) - 1:+.4%}, "
          f"sphericity {row['sphericity']:.4f}, euler {row['euler']}")
    assert abs(row["area_mm2"] / true - 1.0) < 0.01
    assert abs(row["area_faces_mm2"] / (1.5 * true) - 1.0) < 0.01
    assert 0.98 < row["sphericity"] < 1.02
    assert row["euler"] == 1


def test_moments_of_a_box():
    from dram_amd import shape as S
    sp = (2.5, 0.7, 0.9)
    a, b, c = 3, 7, 12
    lab = np.zeros((6, 10, 15), np.uint8)
    lab[2:2 + a, 1:1 + b, 3:3 + c] = 1
    row = S.rows_from_tables(SR.tables(lab, 1), sp)[0]
    want = np.diag([(a * sp[0]) ** 2, (b * sp[1]) ** 2, (c * sp[2]) ** 2]) / 12.0
    assert np.allclose(row["covariance_mm2"], want, rtol=1e-12, atol=0)
    order = np.argsort(-np.diag(want))
    assert np.allclose(row["axes_mm"], 2.0 * np.sqrt(5.0 * np.diag(want)[order]), rtol=1e-12)
    assert np.allclose(np.abs(row["axis_directions"]), np.eye(3)[order], atol=1e-12) and np.all(row["axis_directions"].max(axis=1) > 0.99)
    assert np.allclose(row["centroid"], [2 + (a - 1) / 2, 1 + (b - 1) / 2, 3 + (c - 1) / 2]) and np.allclose(row["centroid_mm"], row["centroid"] * sp)
    lam = np.sort(np.diag(want))[::-1]
    assert math.isclose(row["elongation"], math.sqrt(lam[1] / lam[0]), rel_tol=1e-12) and math.isclose(row["flatness"], math.sqrt(lam[2] / lam[0]), rel_tol=1e-12)
    assert row["voxels"] == a * b * c and row["faces"] == (2 * b * c, 2 * a * c, 2 * a * b)
    assert math.isclose(row["area_faces_mm2"], 2 * (b * sp[1] * c * sp[2] + a * sp[0] * c * sp[2] + a * sp[0] * b * sp[1]), rel_tol=1e-12)
    # the known bias of the Crofton estimate on axis-aligned faces: 74.9 for the 3 x 4 x 5 box of area 94
    box = S.rows_from_tables(SC.expected("full_box"), (1.0, 1.0, 1.0))[0]
    assert box["area_faces_mm2"] == 94.0 and abs(box["area_mm2"] - 74.9) < 0.05


def test_axes_of_a_rotated_ellipsoid():
    """Semi-axes (20, 10, 5) mm, rotated 30 degrees about z, digitised at 0.5 mm: axes within 2 % of (40, 20, 10), the first
    direction within 1 degree of the rotated axis (measured with the restatement's tables: 0.23 % at most, on the shortest axis, and 0.017 degrees)."""
    from dram_amd import shape as S
    h = 0.5
    g = np.meshgrid(np.arange(-6, 6.01, h), np.arange(-19, 19.01, h), np.arange(-19, 19.01, h), indexing="ij")
    z, y, x = (v + 0.1 for v in g)
    th = math.radians(30.0)
    u, v = x * math.cos(th) + y * math.sin(th), -x * math.sin(th) + y * math.cos(th)
    lab = ((u / 20.0) ** 2 + (v / 10.0) ** 2 + (z / 5.0) ** 2 <= 1.0).astype(np.uint8)
    row = S.rows_from_tables(SR.tables(lab, 1), (h, h, h))[0]
    rel = np.abs(row["axes_mm"] / np.array([40.0, 20.0, 10.0]) - 1.0)
    d = row["axis_directions"][0]
    angle = math.degrees(math.acos(min(1.0, abs(d[1] * math.sin(th) + d[2] * math.cos(th)))))
    print(f"ellipsoid: axes {row['axes_mm']}, worst relative error {rel.max():.3%}, first direction off by {angle:.3f} degrees")
    assert np.all(rel < 0.02) and angle < 1.0 and abs(d[0]) < 0.02
    assert d[np.argmax(np.abs(d))] > 0


def test_rows_handle_empty_labels_and_no_labels():
    from dram_amd import shape as S
    lab = np.zeros((3, 3, 3), np.uint8)
    lab[1, 1, 1] = 2
    rows = S.rows_from_tables(SR.tables(lab, 3), (1.0, 2.0, 3.0))
    assert len(rows) == 3 and [r["voxels"] for r in rows] == [0, 1, 0]
    for r in (rows[0], rows[2]):
        assert r["volume_mm3"] == 0.0 and r["euler"] == 0 and r["faces"] == (0, 0, 0) and r["area_mm2"] == 0.0
        assert math.isnan(r["sphericity"]) and math.isnan(r["elongation"]) and math.isnan(r["flatness"])
        assert np.isnan(r["centroid"]).all() and np.isnan(r["covariance_mm2"]).all() and np.isnan(r["axes_mm"]).all()
    one = rows[1]
    assert one["volume_mm3"] == 6.0 and one["faces"] == (2, 2, 2) and one["area_faces_mm2"] == 2 * (6.0 + 3.0 + 2.0) and one["euler"] == 1
    assert np.allclose(one["covariance_mm2"], np.diag([1.0, 4.0, 9.0]) / 12.0) and one["centroid"].tolist() == [1.0, 1.0, 1.0]
    assert S.rows_from_tables({"cfg": np.zeros((0, 256), np.int64), "mom": np.zeros((0, 10), np.int64)}, (1.0, 1.0, 1.0)) == []
    assert S.lesion_shape(lab, 0, (1.0, 1.0, 1.0)) == []
    assert sorted(rows[0]) == sorted(one)
