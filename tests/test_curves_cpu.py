"""Heat-map evaluation curves without a GPU: dram_amd.curves.curves_from_tables against the numpy restatement
(tests/curves_restatement.py) on the tables of every case, the restatement against sklearn.metrics and inference.dice / iou, and
the argument checks of the C entry points, which come before the first launch."""
import ctypes
import os
import re

import numpy as np
import pytest

import curves_cases as CC
import curves_restatement as CR

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
assert_curves_equal, _n_cal = CC.assert_curves_equal, CC.n_cal


@pytest.mark.parametrize("name", CC.names())
def test_curves_from_tables_matches_the_restatement(name):
    from dram_amd.curves import curves_from_tables
    c = CC.case(name)
    hist, conf = CC.expected(name)
    assert hist.shape == (c["nregions"], 2, c["nbins"] + 1) and (conf is None) == (not c["conf"])
    if conf is not None:
        assert not conf[:, :, 0].any() and np.all(conf <= hist * CR.TWO24)
    got = curves_from_tables(hist, conf, _n_cal(c))
    ref = CR.curves(hist, conf, _n_cal(c))
    assert_curves_equal(got, ref)
    rows, nbins = c["nregions"] + 1, c["nbins"]
    assert got["tp"].shape == (rows, nbins) and got["auc_roc"].shape == (rows,)
    assert np.array_equal(got["tp"] + got["fn"], np.broadcast_to(got["tp"][:, :1] + got["fn"][:, :1], (rows, nbins)))
    assert np.array_equal(got["tp"][-1], got["tp"][:-1].sum(axis=0))               # the last row is the regions pooled
    if conf is not None:
        assert got["cal_count"].shape == (rows, _n_cal(c))
        assert np.array_equal(got["cal_count"].sum(axis=1), hist.sum(axis=1)[:, 1:].sum(axis=1).tolist() + [hist[:, :, 1:].sum()])


def _rows_to_check(c):
    """(row, voxel selection) for up to four regions and the pooled row."""
    n = c["score"].size
    reg = np.ones(n, dtype=np.int64) if c["region"] is None else c["region"].astype(np.int64)
    some = sorted({1, 2, c["nregions"] // 2 + 1, c["nregions"]})
    return [(r - 1, reg == r) for r in some if r <= c["nregions"]] + [(c["nregions"], (reg >= 1) & (reg <= c["nregions"]))]


SKLEARN_CASES = ("size_4097", "multi_lap_big", "multi_lap_global_noconf", "specials_256", "specials_4096", "region_null", "regions_5",
                 "regions_255_global", "no_positive", "no_negative", "empty_region", "gate_random_noconf", "gate_off", "one_bin_64k")


@pytest.mark.parametrize("name", SKLEARN_CASES)
def test_auc_and_average_precision_match_sklearn(name):
    """Both sides are fp64 sums of at most 4097 terms of size <= 1: 1e-10."""
    metrics = pytest.importorskip("sklearn.metrics")
    c = CC.case(name)
    hist, _ = CC.expected(name)
    ref = CR.curves(hist, None, None)
    level = CR.bin_index(c["score"], c["gate"], c["nbins"])
    y = (c["ref"].reshape(-1) != 0).astype(np.int64)
    for row, sel in _rows_to_check(c):
        P, N = int(y[sel].sum()), int(sel.sum() - y[sel].sum())
        if P and N:
            assert abs(ref["auc_roc"][row] - metrics.roc_auc_score(y[sel], level[sel])) <= 1e-10, row
        else:
            assert np.isnan(ref["auc_roc"][row]), row
        if P:
            assert abs(ref["average_precision"][row] - metrics.average_precision_score(y[sel], level[sel])) <= 1e-10, row
        else:
            assert np.isnan(ref["average_precision"][row]), row


@pytest.mark.parametrize("name", ("size_4097", "specials_256", "regions_5", "gate_off", "no_positive", "region_null", "multi_lap_global"))
def test_dice_and_iou_are_those_of_the_thresholded_arrays(name):
    from dram_amd import inference
    c = CC.case(name)
    hist, _ = CC.expected(name)
    ref = CR.curves(hist, None, None)
    nbins = c["nbins"]
    score, target = c["score"].reshape(-1), c["ref"].reshape(-1)
    on = np.ones(score.size, dtype=bool) if c["gate"] is None else c["gate"].reshape(-1) != 0
    for j in sorted({0, 1, nbins // 2, nbins - 2, nbins - 1}):
        with np.errstate(invalid="ignore"):
            predict = (score >= np.float32(ref["thresholds"][j])) & on
        for row, sel in _rows_to_check(c):
            assert ref["dice"][row, j] == inference.dice(predict[sel], target[sel]), (j, row)
            assert ref["iou"][row, j] == inference.iou(predict[sel], target[sel]), (j, row)
            assert ref["tp"][row, j] == np.count_nonzero(predict[sel] & (target[sel] != 0))
    best = np.argmax(ref["dice"], axis=1)                                          # the first of equal maxima
    assert np.array_equal(ref["best_dice_threshold"], best / nbins)


def test_tables_of_two_scans_add_to_the_table_of_both():
    a, b = CC.case("offset_none"), CC.case("offset_score_1")
    assert (a["nregions"], a["nbins"]) == (b["nregions"], b["nbins"])
    both = CR.tables(*(np.concatenate([a[k], b[k]]) for k in ("score", "ref", "region")), a["nregions"],
                     np.concatenate([a["gate"], b["gate"]]), a["nbins"], True)
    for x, y, z in zip(CC.expected("offset_none"), CC.expected("offset_score_1"), both):
        assert np.array_equal(x + y, z)
    from dram_amd.curves import curves_from_tables
    pooled = curves_from_tables(CC.expected("offset_none")[0] + CC.expected("offset_score_1")[0])
    assert pooled["tp"][-1, 0] == both[0][:, 1, 1:].sum() and "ece" not in pooled


def test_special_scores_land_where_the_definition_says():
    nbins = 256
    f = np.float32
    score = np.array([0.0, -0.0, 1e-45, 1.0, np.nextafter(f(1), f(0)), 1.5, np.inf, -1e-30, -np.inf, np.nan, 0.5, np.nextafter(f(0.5), f(0))],
                     dtype=np.float32)
    assert CR.bin_index(score, None, nbins).tolist() == [1, 1, 1, 256, 256, 256, 256, 0, 0, 0, 129, 128]
    assert CR.bin_index(score, np.zeros(score.size, np.uint8), nbins).tolist() == [0] * score.size
    q = CR.confidence_q(score)
    assert q.tolist() == [0, 0, 0, 1 << 24, (1 << 24) - 1, 1 << 24, 1 << 24, 0, 0, 0, 1 << 23, (1 << 23) - 1]
    # the fp32 product of the kernel is the fp64 product of the restatement: nbins is a power of two
    rng = np.random.default_rng(3)
    s = rng.random(200000).astype(np.float32)
    for nb in (2, 256, 1024, 4096):
        assert np.array_equal(np.floor(s * f(nb)).astype(np.int64), np.floor(s.astype(np.float64) * nb).astype(np.int64))


def test_curves_from_tables_refuses_bad_tables():
    from dram_amd.curves import curves_from_tables
    hist = np.zeros((2, 2, 257), dtype=np.int64)
    with pytest.raises(ValueError, match="power of two"):
        curves_from_tables(np.zeros((2, 2, 4), dtype=np.int64))
    with pytest.raises(ValueError, match="integer"):
        curves_from_tables(hist.astype(np.float64))
    with pytest.raises(ValueError, match="n_cal"):
        curves_from_tables(hist, hist, n_cal=3)
    with pytest.raises(ValueError, match="n_cal"):
        curves_from_tables(hist, hist, n_cal=512)
    with pytest.raises(ValueError, match="shape"):
        curves_from_tables(hist, hist[:1])
    empty = curves_from_tables(hist, hist)
    assert np.isnan(empty["auc_roc"]).all() and np.isnan(empty["ece"]).all() and np.isnan(empty["tpr"]).all()
    assert (empty["dice"] == 1.0).all() and (empty["best_dice_threshold"] == 0.0).all()


def _header_functions():
    src = open(os.path.join(ROOT, "include", "dram_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(?:int|size_t|const char\*)\s+(dram_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        args = m.group(2).strip()
        out[m.group(1)] = 0 if args in ("", "void") else len(args.split(","))
    return out


def test_curve_entry_points_are_exported_with_the_declared_argument_counts():
    import inspect
    import dram_amd
    from dram_amd import _lib, inference
    decl = _header_functions()
    lib = ctypes.CDLL(os.path.join(ROOT, "bodyct-dram_amd", "libdram_hip.so"))
    for name, nargs in {"dram_score_hist_plan": 3, "dram_score_hist": 10}.items():
        assert hasattr(lib, name), f"libdram_hip.so does not export {name}"
        assert decl[name] == nargs and len(_lib.SIGNATURES[name][1]) == nargs, name
    assert _lib.lib.dram_abi_version() == 2
    for name in ("score_tables", "curves_from_tables", "heatmap_curves"):
        assert callable(getattr(dram_amd, name)) and name in dram_amd.__all__
    for fn in (inference.LobeInference.run, inference.LobeInference.post_process):
        assert inspect.signature(fn).parameters["curves"].default is None


def test_score_hist_argument_errors_are_reported_without_a_gpu():
    """Every check comes before the first launch, so the error paths answer on a machine without a GPU (dummy non-null
    pointers)."""
    from dram_amd import _lib
    q = 16

    def run(score=q, ref=q, region=q, gate=None, nregions=5, nbins=1024, hist=q, conf=q, nvox=1000):
        return _lib.lib.dram_score_hist(score, ref, region, gate, nregions, nbins, hist, conf, nvox, None)

    err = lambda: _lib.lib.dram_last_error()
    for null in ("score", "ref", "hist"):
        assert run(**{null: None}) == -1 and b"null" in err(), null
    assert run(nvox=0) == -1 and run(nvox=1 << 31) == -1 and b"2^31" in err()
    for nbins in (0, 3, 8192, 1, -4, 4097):
        assert run(nbins=nbins) == -1 and b"power of two" in err(), nbins
        assert CC.plan(5, nbins, 1) == -1 and b"power of two" in err(), nbins
    for nregions in (0, 256, -1):
        assert run(nregions=nregions) == -1 and CC.plan(nregions, 1024, 0) == -1, nregions
    assert run(region=None, nregions=2) == -1 and b"one region" in err()
    assert run(score=18) == -1 and b"misaligned" in err()


def test_plan_is_a_function_of_its_arguments_and_every_path_is_exercised():
    plan = CC.plan
    for args in ((1, 2, 0), (5, 1024, 1), (5, 4096, 0), (255, 4096, 1)):
        assert plan(*args) in (0, 1) and plan(*args) == plan(*args)
    assert plan(5, 1024, 1) == 0 and plan(5, 256, 1) == 0 and plan(1, 4096, 1) == 0       # the lobes at the default bins, with conf
    assert plan(5, 4096, 0) == 1 and plan(5, 4096, 1) == 1 and plan(255, 256, 0) == 1
    assert plan(5, 1024, 7) == plan(5, 1024, 1)                                           # with_conf is a flag
    for name, r in CC.REGIMES.items():
        assert CC.regime(name) == r, name
    seen = {(CC.regime(name), CC.case(name)["conf"]) for name in CC.names()}
    assert seen == {(0, False), (0, True), (1, False), (1, True)}
    assert {CC.case(name)["nbins"] for name in CC.names()} >= {2, 256, 1024, 4096}
    assert {CC.case(name)["nregions"] for name in CC.names()} >= {1, 5, 255}
