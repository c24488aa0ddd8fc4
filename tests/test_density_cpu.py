"""CPU-side checks of the lesion density report: the numpy restatement (tests/density_restatement.py) against scipy.ndimage and
np.percentile on the named cases, its report arithmetic on a hand-made case, and the C ABI surface of csrc/density.hip (no
kernel runs)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import density_cases as DC
import density_restatement as DR

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ENTRY_ARGS = {"dram_label_density_plan": 3, "dram_label_density": 16, "dram_hist_summary": 12}


@pytest.mark.parametrize("name", DC.NAMES_WITHOUT_LIBRARY + tuple(DC.WAVE_ONLY))
def test_restatement_moments_and_histogram_like_scipy(name):
    ndimage = pytest.importorskip("scipy.ndimage")
    c = DC.case(name)
    count, total, sumsq, vmin, vmax, hist = DC.expected(name)
    n, index = c["n"], np.arange(1, c["n"] + 1)
    scan = c["scan"].astype(np.int64)
    labels = c["labels"].astype(np.int64)
    labels = np.where((labels < 0) | (labels > n), 0, labels)              # scipy is asked for 1..n only, like the entry
    if c["mask"] is not None:
        labels = np.where(c["mask"] != 0, labels, 0)
    assert np.array_equal(count, ndimage.sum_labels(np.ones_like(scan), labels, index).astype(np.int64))
    # scipy sums in fp64: exact while the sums stay below 2^53, which every case here does
    assert np.array_equal(total, ndimage.sum_labels(scan.astype(np.float64), labels, index).astype(np.int64))
    assert np.array_equal(sumsq, ndimage.sum_labels((scan * scan).astype(np.float64), labels, index).astype(np.int64))
    present = count > 0
    assert np.array_equal(vmin[present], np.asarray(ndimage.minimum(scan, labels, index))[present])
    assert np.array_equal(vmax[present], np.asarray(ndimage.maximum(scan, labels, index))[present])
    assert np.all(vmin[~present] == 32767) and np.all(vmax[~present] == -32768)
    assert count.dtype == total.dtype == sumsq.dtype == np.int64 and vmin.dtype == vmax.dtype == np.int32
    if hist is None:
        return
    lo, width, nbins = c["bins"]
    assert hist.shape == (n, nbins + 2) and np.array_equal(hist.sum(axis=1), count)
    # scipy (np.histogram) closes the last bin on the right; here every bin is half-open, so a value on the top edge is kept
    # from scipy and counted with the overflow entry below
    inner = ndimage.histogram(scan, lo, lo + nbins * width, nbins, np.where(scan == lo + nbins * width, 0, labels), index)
    for k in range(n):
        row = np.zeros(nbins, np.int64) if inner[k] is None else np.asarray(inner[k]).astype(np.int64)
        assert np.array_equal(hist[k, 1:-1], row)
        assert hist[k, 0] == np.count_nonzero((labels == k + 1) & (scan < lo))
        assert hist[k, -1] == np.count_nonzero((labels == k + 1) & (scan >= lo + nbins * width))


def test_extremes_leave_int32_and_2_to_the_32():
    count, total, sumsq, vmin, vmax, _ = DC.expected("extremes")
    assert count.tolist() == [71680, 71680]
    assert total.tolist() == [71680 * 32767, -71680 * 32768] and abs(total[0]) > 2 ** 31 and abs(total[1]) > 2 ** 31
    assert sumsq.tolist() == [71680 * 32767 ** 2, 71680 * 32768 ** 2] and sumsq.min() > 2 ** 32
    assert vmin.tolist() == [32767, -32768] and vmax.tolist() == [32767, -32768]


def test_bins_at_the_edges():
    for lo, width, nbins in ((-50, 1, 10), (-1000, 7, 100), (-5, 7, 1), (-1024, 1, 4096)):
        v = [lo - 1, lo, lo + width - 1, lo + width, lo + nbins * width - 1, lo + nbins * width]
        assert DR.bin_of(v, lo, width, nbins).tolist() == [0, 1, 1, min(2, nbins + 1), nbins, nbins + 1]


@pytest.mark.parametrize("count", [1, 2, 7, 10, 999, 1001, 1337])
def test_restatement_percentile_like_numpy_inverted_cdf(count):
    """np.percentile(method="inverted_cdf") is the nearest-rank percentile where q * count / 1000 is no integer; where it is one
    numpy's floating rank is not a definition to pin against, so those q are left to the sorted-array definition alone."""
    x = np.random.default_rng(count).integers(-1100, 400, size=count).astype(np.int16)
    for q in (0, 1, 150, 333, 500, 850, 999, 1000):
        mine = DR.percentile_of_values(x, q)
        assert mine == np.sort(x)[DR.rank_of(q, count) - 1]
        if q in (0, 1000) or (q * count) % 1000 != 0:
            assert mine == np.percentile(x, q / 10.0, method="inverted_cdf"), (q, count)
    assert DR.percentile_of_values(x, 0) == x.min() and DR.percentile_of_values(x, 1000) == x.max()


def test_summary_with_width_one_is_the_percentile_of_the_values():
    rng = np.random.default_rng(8)
    scan = rng.integers(-1024, 3072, size=500).astype(np.int16)
    labels = rng.integers(0, 4, size=500).astype(np.uint8)
    q = (0, 150, 500, 850, 1000)
    pct, bands = DR.summary(DR.histogram(scan, labels, 3, -1024, 1, 4096), -1024, 1, 4096, q, (-950, -750, -300))
    for k in range(3):
        x = scan[labels == k + 1].astype(np.int64)
        assert pct[k].tolist() == [DR.percentile_of_values(x, qq) for qq in q]
        assert bands[k].tolist() == [np.count_nonzero(x < -950), np.count_nonzero((x >= -950) & (x < -750)),
                                     np.count_nonzero((x >= -750) & (x < -300)), np.count_nonzero(x >= -300)]


def test_summary_cases_are_what_they_are_meant_to_be():
    e = {k: DC.summary_expected(k) for k in DC.SUMMARY_CASES}
    assert e["even_count_median"][0].tolist() == [[-10, -5, 5, 5, -10], [-10, -10, 5, 5, -10], [-10, 0, 5, 0, -10]]
    assert e["even_count_median"][1].tolist() == [[1, 4, 5], [5, 0, 5], [2, 4, 4]]
    assert e["rank_in_underflow"][0].tolist() == [[DR.INT32_MIN, DR.INT32_MIN, DR.INT32_MIN, DR.INT32_MIN, DR.INT32_MAX],
                                                  [DR.INT32_MIN, DR.INT32_MIN, DR.INT32_MAX, DR.INT32_MAX, DR.INT32_MAX]]
    assert e["rank_only_in_overflow"][0].tolist() == [[-3, -3, DR.INT32_MAX, DR.INT32_MAX], [DR.INT32_MAX] * 4]
    assert e["empty_row"][0][0].tolist() == [DR.INT32_MAX] * 3 and e["empty_row"][1][0].tolist() == [0, 0, 0]
    assert e["edges_on_both_ends"][1].tolist() == [[3, 3, 3, 4], [0, 5, 0, 6]]       # underflow in band 0, overflow in band ne
    assert e["no_percentiles"][0].shape == (4, 0) and e["no_edges"][1].shape == (4, 1)
    for name, (pct, bands) in e.items():
        assert np.array_equal(bands.sum(axis=1), DC.SUMMARY_CASES[name]["hist"].sum(axis=1)), name
        assert pct.dtype == np.int32 and bands.dtype == np.int64


def test_report_arithmetic_on_a_hand_made_case():
    from dram_amd import density
    count = np.array([4, 0, 2, 200000], dtype=np.int64)
    total = np.array([-10, 0, 3, 200000 * 32767], dtype=np.int64)                     # values -4, -3, -2, -1 and 1, 2
    sumsq = np.array([30, 0, 5, 200000 * 32767 ** 2], dtype=np.int64)
    vmin, vmax = np.array([-4, 32767, 1, 32767], np.int32), np.array([-1, -32768, 2, 32767], np.int32)
    pct = np.array([[-4, -3], [DR.INT32_MAX] * 2, [1, 1], [DR.INT32_MAX] * 2], dtype=np.int32)
    bands = np.array([[1, 3], [0, 0], [0, 2], [0, 200000]], dtype=np.int64)
    for rep in (DR.report_from_tables(count, total, sumsq, vmin, vmax, pct, bands),
                density.report_from_tables(count, total, sumsq, vmin, vmax, pct, bands)):
        assert rep["voxels"].tolist() == [4, 0, 2, 200000]
        assert rep["mean_hu"][0] == -2.5 and rep["std_hu"][0] == math.sqrt(1.25)     # (4 * 30 - 100) / 16
        assert math.isnan(rep["mean_hu"][1]) and math.isnan(rep["std_hu"][1]) and np.isnan(rep["band_fraction"][1]).all()
        assert rep["mean_hu"][2] == 1.5 and rep["std_hu"][2] == 0.5
        # count * sumsq is 4.3e19, past int64: formed in Python integers the variance of a constant is exactly zero
        assert 200000 * int(sumsq[3]) > 2 ** 63 and rep["mean_hu"][3] == 32767.0 and rep["std_hu"][3] == 0.0
        assert rep["band_fraction"][0].tolist() == [0.25, 0.75] and rep["band_fraction"][3].tolist() == [0.0, 1.0]
        assert rep["min_hu"].tolist() == vmin.tolist() and rep["max_hu"].tolist() == vmax.tolist()
        assert np.array_equal(rep["percentiles_hu"], pct) and np.array_equal(rep["band_voxels"], bands)
    assert density.BAND_NAMES == ("laa", "aerated", "ggo", "consolidation") and density.BAND_EDGES_HU == (-950, -750, -300)


def _header_functions():
    src = open(os.path.join(ROOT, "include", "dram_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(?:int|size_t|const char\*)\s+(dram_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        args = m.group(2).strip()
        out[m.group(1)] = 0 if args in ("", "void") else len(args.split(","))
    return out


def test_density_entry_points_are_exported_with_the_declared_argument_counts():
    from dram_amd import _lib
    decl = _header_functions()
    lib = ctypes.CDLL(os.path.join(ROOT, "bodyct-dram_amd", "libdram_hip.so"))
    for name, nargs in ENTRY_ARGS.items():
        assert hasattr(lib, name), f"libdram_hip.so does not export {name}"
        assert decl[name] == nargs and len(_lib.SIGNATURES[name][1]) == nargs, name
    import dram_amd
    for name in ("label_density", "hist_summary", "label_report"):
        assert callable(getattr(dram_amd, name)) and name in dram_amd.__all__
    import inspect
    assert {"scan", "percentiles_permille", "band_edges_hu"} <= set(inspect.signature(dram_amd.lesion_report).parameters)


def test_density_argument_errors_are_reported_without_a_gpu():
    """Every check comes before the first launch, so the error paths answer on a machine without a GPU (dummy non-null
    pointers)."""
    from dram_amd import _lib
    q = 16

    def density(scan=q, labels=q, kind=0, mask=None, n=5, count=q, total=q, sumsq=q, vmin=q, vmax=q, hist=q, lo=-1024, width=1,
                nbins=4096, nvox=1000):
        return _lib.lib.dram_label_density(scan, labels, kind, mask, n, count, total, sumsq, vmin, vmax, hist, lo, width, nbins, nvox, None)

    err = lambda: _lib.lib.dram_last_error()
    for null in ("scan", "labels", "count", "total", "sumsq", "vmin", "vmax"):
        assert density(**{null: None}) == -1 and b"null" in err(), null
    assert density(nvox=0) == -1 and density(nvox=1 << 31) == -1 and b"2^31" in err()
    assert density(n=0) == -1 and density(n=-2) == -1
    assert density(kind=0, n=256) == -1 and density(kind=2) == -1 and density(kind=-1) == -1
    assert density(nbins=-1) == -1 and density(nbins=4097) == -1
    assert density(width=0) == -1 and density(width=-3) == -1 and b"width" in err()
    assert density(kind=1, n=(1 << 31) // 4098 + 1) == -1                            # n * (nbins + 2) >= 2^31
    assert density(kind=1, n=1 << 30, hist=None, nbins=0) == -1                      # ... and without a histogram: 2^30 * 2
    assert density(lo=2 ** 31 - 4096, width=1) == -1 and density(lo=0, width=2 ** 20) == -1 and b"int32" in err()
    assert density(hist=None) == -1 and b"together" in err()
    assert density(nbins=0) == -1 and b"together" in err()

    def summary(hist=q, n=3, lo=-10, width=5, nbins=4, qs=(0, 500), edges=(-5, 5), pct=q, bands=q, nq=None, ne=None):
        qa, ea = np.asarray(qs, dtype=np.int32), np.asarray(edges, dtype=np.int32)
        return _lib.lib.dram_hist_summary(hist, n, lo, width, nbins, qa.ctypes.data if qa.size else None, qa.size if nq is None else nq,
                                          ea.ctypes.data if ea.size else None, ea.size if ne is None else ne, pct, bands, None)

    assert summary(hist=None) == -1 and summary(n=0) == -1 and summary(nbins=4097) == -1 and summary(width=0) == -1
    assert summary(pct=None) == -1 and summary(bands=None) == -1
    assert summary(qs=(0, 1001)) == -1 and summary(qs=(-1,)) == -1 and b"per mille" in err()
    assert summary(qs=(1,) * 17) == -1 and summary(edges=tuple(range(-10, 11, 5)) * 4) == -1
    assert summary(edges=(-4,)) == -1 and b"lo + j * width" in err()                 # off the bin edges
    assert summary(edges=(-15,)) == -1 and summary(edges=(15,)) == -1                # below lo, above lo + nbins * width
    assert summary(edges=(5, -5)) == -1 and summary(edges=(5, 5)) == -1 and b"ascend" in err()
    assert summary(qs=(), edges=(), pct=None, bands=None) == 0                       # nothing asked for: nothing launched


def test_plan_is_a_function_of_its_arguments_and_refuses_what_the_entry_refuses():
    plan = DC.plan
    for args in ((0, 5, 4096), (0, 5, 0), (1, 3000, 0), (1, 3000, 4096), (0, 255, 4096), (1, 1, 0)):
        assert plan(*args) in (0, 1) and plan(*args) == plan(*args)
    assert plan(0, 5, 4096) == 0 and plan(0, 5, 0) == 0                              # the lobe map, with and without histogram
    assert plan(1, 3000, 4096) == 1 and plan(0, 255, 4096) == 1                      # component labels; many labels with one
    for args in ((0, 0, 0), (1, -1, 0), (0, 256, 0), (2, 5, 0), (-1, 5, 0), (1, 5, -1), (1, 5, 4097), (1, (1 << 31) // 4098 + 1, 4096),
                 (1, 1 << 30, 0)):
        assert plan(*args) < 0, args
    assert plan(1, (1 << 31) // 4098, 4096) == 1 and plan(1, (1 << 30) - 1, 0) == 1  # the last sizes in range
    # monotone in n and in nbins, so the searched seams are the only ones; and they are where the cases say
    n0, b0, n4 = DC.last_n_in_lds(1, 0), DC.last_nbins_in_lds(0, 255), DC.last_n_in_lds(1, 4096)
    assert [plan(1, n, 0) for n in (1, n0, n0 + 1, 10 * n0)] == [0, 0, 1, 1]
    assert [plan(0, 255, b) for b in (0, b0, b0 + 1, 4096)] == [0, 0, 1, 1]
    assert [plan(1, n, 4096) for n in (1, n4, n4 + 1)] == [0, 0, 1] and n4 >= 5
    assert sorted({plan(1, n, 0) for n in range(1, 2 * n0, 97)}) == [0, 1]
    for name, want in DC.SEAM_REGIMES.items():
        assert DC.regime(name) == want, name
    assert {DC.regime(name) for name in DC.names()} == {0, 1}
    assert all(DC.regime(name) == 1 for name in DC.names() if name.endswith("/wave") or name in DC.WAVE_ONLY)
    assert all(DC.regime(name) == 0 for name in DC.NAMES_WITHOUT_LIBRARY)
