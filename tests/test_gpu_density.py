"""csrc/density.hip and dram_amd/density.py on the device against the numpy restatement (tests/density_restatement.py, itself
held against scipy.ndimage and np.percentile by tests/test_density_cpu.py): everything is integers, so every comparison is
exact."""
import numpy as np
import pytest
import torch

import density_cases as DC
import density_restatement as DR

pytestmark = pytest.mark.gpu


def _st():
    return torch.cuda.current_stream().cuda_stream


def _placed(a, offset):
    """A device copy of the flat array whose first element lies `offset` elements past a 16-byte boundary; (holder, pointer)."""
    flat = np.ascontiguousarray(a).reshape(-1)
    holder = torch.zeros(flat.size + offset, dtype=torch.from_numpy(flat[:1].copy()).dtype, device="cuda")
    assert holder.data_ptr() % 16 == 0
    holder[offset:] = torch.from_numpy(flat.copy())
    return holder, holder.data_ptr() + offset * flat.itemsize


def gpu_density(c):
    from dram_amd._lib import call
    n, bins = c["n"], c["bins"]
    scan, p_scan = _placed(c["scan"], c["offsets"][0])
    labels, p_labels = _placed(c["labels"], c["offsets"][1])
    mask, p_mask = (None, None) if c["mask"] is None else _placed(c["mask"], c["offsets"][2])
    i64 = [torch.full((n,), -7, dtype=torch.int64, device="cuda") for _ in range(3)]           # poisoned: the entry initialises
    i32 = [torch.full((n,), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
    lo, width, nbins = bins if bins is not None else (0, 0, 0)
    hist = None if bins is None else torch.full((n, nbins + 2), -7, dtype=torch.int64, device="cuda")
    call("dram_label_density", p_scan, p_labels, 0 if c["labels"].dtype == np.uint8 else 1, p_mask, n, *(t.data_ptr() for t in i64),
         *(t.data_ptr() for t in i32), None if hist is None else hist.data_ptr(), lo, width, nbins, c["scan"].size, _st())
    out = tuple(t.cpu().numpy() for t in i64 + i32) + (None if hist is None else hist.cpu().numpy(),)
    del scan, labels, mask
    return out


def _same(a, b):
    return all((x is None and y is None) or (x is not None and y is not None and x.dtype == y.dtype and np.array_equal(x, y))
               for x, y in zip(a, b))


@pytest.mark.parametrize("name", DC.names())
def test_label_density_matches_the_restatement(name):
    c = DC.case(name)
    ref = DC.expected(name)
    got = gpu_density(c)
    for key, g, r in zip(("count", "sum", "sumsq", "min", "max", "hist"), got, ref):
        assert (g is None) == (r is None), key
        if g is not None:
            assert g.dtype == r.dtype and np.array_equal(g, r), key
    assert _same(gpu_density(c), got)                                                          # no dependence on the order of the atomics
    if name in DC.SEAM_REGIMES:
        assert DC.regime(name) == DC.SEAM_REGIMES[name]
    if name.endswith("/wave") or name in DC.WAVE_ONLY:
        assert DC.regime(name) == 1


def test_both_regimes_and_label_kinds_are_exercised():
    seen = {(DC.regime(name), DC.case(name)["labels"].dtype.name, DC.case(name)["bins"] is not None, DC.case(name)["mask"] is not None)
            for name in DC.names()}
    for regime in (0, 1):
        for kind in ("uint8", "int32"):
            assert {(h, m) for r, k, h, m in seen if r == regime and k == kind} >= {(True, True), (True, False)}, (regime, kind)
    assert (0, "uint8", False, False) in seen and (0, "int32", False, False) in seen and (1, "int32", False, False) in seen


def gpu_summary(c):
    from dram_amd._lib import call
    hist = torch.from_numpy(np.array(c["hist"])).cuda()
    n, nq, ne = hist.shape[0], len(c["q"]), len(c["edges"])
    q, edges = np.asarray(c["q"], dtype=np.int32), np.asarray(c["edges"], dtype=np.int32)
    pct = torch.full((n, nq), -7, dtype=torch.int32, device="cuda")
    bands = torch.full((n, ne + 1), -7, dtype=torch.int64, device="cuda")
    call("dram_hist_summary", hist.data_ptr(), n, c["lo"], c["width"], c["nbins"], q.ctypes.data if nq else None, nq,
         edges.ctypes.data if ne else None, ne, pct.data_ptr() if nq else None, bands.data_ptr(), _st())
    return pct.cpu().numpy(), bands.cpu().numpy()


@pytest.mark.parametrize("name", list(DC.SUMMARY_CASES))
def test_hist_summary_matches_the_restatement(name):
    c = DC.SUMMARY_CASES[name]
    pct_ref, bands_ref = DC.summary_expected(name)
    pct, bands = gpu_summary(c)
    assert pct.dtype == np.int32 and np.array_equal(pct, pct_ref)
    assert bands.dtype == np.int64 and np.array_equal(bands, bands_ref)
    assert np.array_equal(bands.sum(axis=1), c["hist"].sum(axis=1))
    again = gpu_summary(c)
    assert np.array_equal(again[0], pct) and np.array_equal(again[1], bands)


def test_hist_summary_without_bands_writes_percentiles_only():
    from dram_amd._lib import call
    c = DC.SUMMARY_CASES["no_edges"]
    hist = torch.from_numpy(np.array(c["hist"])).cuda()
    q = np.asarray(c["q"], dtype=np.int32)
    pct = torch.full((hist.shape[0], q.size), -7, dtype=torch.int32, device="cuda")
    call("dram_hist_summary", hist.data_ptr(), hist.shape[0], c["lo"], c["width"], c["nbins"], q.ctypes.data, q.size, None, 0,
         pct.data_ptr(), None, _st())
    assert np.array_equal(pct.cpu().numpy(), DC.summary_expected("no_edges")[0])


def _assert_report_equal(rep, ref):
    assert sorted(rep) == sorted(ref)
    for key in ref:
        a, b = np.asarray(rep[key]), np.asarray(ref[key])
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), key


@pytest.mark.parametrize("name", ["multi_lap_u8", "skipped_i32", "mask_200", "absent_label"])
def test_label_report_end_to_end(name):
    from dram_amd import label_density, label_report
    c = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in DC.case(name).items()}      # writable copies
    ref = DR.label_report(c["scan"], c["labels"], c["n"], c["mask"])
    rep = label_report(torch.from_numpy(c["scan"].copy()).cuda(), torch.from_numpy(c["labels"].copy()).cuda(), c["n"], mask=c["mask"])
    _assert_report_equal(rep, ref)
    assert np.isnan(rep["mean_hu"]).sum() == np.count_nonzero(rep["voxels"] == 0)
    # other percentiles, edges and bins; a host scan goes in as it is
    kw = dict(percentiles_permille=(0, 1000), band_edges_hu=(-1000, 0), hist_range=(-2000, 50, 100))
    _assert_report_equal(label_report(c["scan"], c["labels"], c["n"], mask=c["mask"], **kw),
                         DR.label_report(c["scan"], c["labels"], c["n"], c["mask"], **kw))
    d = label_density(c["scan"], c["labels"], c["n"], mask=c["mask"], bins=c["bins"])
    for key, r in zip(("count", "sum", "sumsq", "min", "max"), DC.expected(name)):
        assert np.array_equal(d[key], r) and d[key].dtype == r.dtype
    assert (d["hist"] is None) == (c["bins"] is None)
    if d["hist"] is not None:
        assert d["hist"].is_cuda and np.array_equal(d["hist"].cpu().numpy(), DC.expected(name)[5])
    with pytest.raises(ValueError, match="int16"):
        label_report(c["scan"].astype(np.int32), c["labels"], c["n"])
    with pytest.raises(ValueError, match="uint8 or int32"):
        label_report(c["scan"], c["labels"].astype(np.int64), c["n"])


def _planted():
    """12 x 20 x 24: three lobes, four blobs of different density (one of them a speck that the filter drops, one across two
    lobes), noise everywhere."""
    rng = np.random.default_rng(17)
    shape = (12, 20, 24)
    lobe = np.zeros(shape, dtype=np.uint8)
    lobe[:, 2:, 0:8], lobe[:, 2:, 8:16], lobe[:, 2:, 16:24] = 1, 2, 4              # label 3 is absent
    scan = rng.integers(-990, -700, size=shape).astype(np.int16)
    scan[lobe == 0] = 40
    blobs = {"ggo": ((slice(2, 5), slice(4, 8), slice(1, 5)), (-700, -350)), "dense": ((slice(6, 10), slice(10, 14), slice(6, 11)), (-250, 60)),
             "mixed": ((slice(3, 8), slice(14, 18), slice(17, 22)), (-800, 20)), "speck": ((10, 18, slice(20, 22)), (-100, 0))}
    mask = np.zeros(shape, dtype=np.uint8)
    for sl, (a, b) in blobs.values():
        mask[sl] = 1
        scan[sl] = rng.integers(a, b, size=scan[sl].shape).astype(np.int16)
    return mask, lobe, scan


def test_lesion_report_with_a_scan():
    import components_restatement as CR
    from dram_amd import lesion_report
    mask, lobe, scan = _planted()
    spacing = (2.0, 1.0, 1.0)
    kw = dict(connectivity=1, min_volume_mm3=6.0)
    plain = lesion_report(mask, lobe, spacing, **kw)
    assert "density" not in plain and plain["n_lesions"] == 3
    rep = lesion_report(mask, lobe, spacing, scan=torch.from_numpy(scan).cuda(), **kw)
    assert sorted(rep) == sorted(list(plain) + ["density"])
    for key in plain:                                                              # every other key as without the scan
        if isinstance(plain[key], torch.Tensor):
            assert torch.equal(rep[key], plain[key]), key
        elif isinstance(plain[key], np.ndarray):
            assert np.array_equal(rep[key], plain[key]), key
        else:
            assert rep[key] == plain[key], key
    ref_rep = CR.report(mask, lobe, spacing, **kw)
    ref = DR.lesion_density(scan, ref_rep["labels"], ref_rep["n_lesions"], ref_rep["mask"], lobe)
    _assert_report_equal(rep["density"]["lesions"], ref["lesions"])
    assert rep["density"]["lesions"]["voxels"].shape == rep["volumes_ml"].shape
    assert np.array_equal(rep["density"]["lesions"]["voxels"] * 2.0 / 1000.0, rep["volumes_ml"])
    assert sorted(rep["density"]["lobes"]) == sorted(ref["lobes"]) == sorted(rep["lobes"]) == [1, 2, 4]
    for v in ref["lobes"]:
        for part in ("parenchyma", "lesion"):
            _assert_report_equal(rep["density"]["lobes"][v][part], ref["lobes"][v][part])
        assert rep["density"]["lobes"][v]["parenchyma"]["voxels"] == rep["lobes"][v]["voxels"]
        assert rep["density"]["lobes"][v]["lesion"]["voxels"] == rep["lobes"][v]["lesion_voxels"]
    # the blobs are told apart by density: the dense one has no voxel below -300 HU, the ground-glass one none at or above
    bands = rep["density"]["lesions"]["band_voxels"]
    assert bands[0, 3] == 0 and bands[2, :3].sum() == 0 and bands[1, 3] > 0 and bands[1, :3].sum() > 0
    # other settings travel through; a wrong scan is refused
    other = lesion_report(mask, lobe, spacing, scan=scan, percentiles_permille=(500,), band_edges_hu=(-500,), **kw)
    ref2 = DR.lesion_density(scan, ref_rep["labels"], ref_rep["n_lesions"], ref_rep["mask"], lobe, percentiles_permille=(500,),
                             band_edges_hu=(-500,))
    _assert_report_equal(other["density"]["lesions"], ref2["lesions"])
    with pytest.raises(ValueError, match="scan"):
        lesion_report(mask, lobe, spacing, scan=scan[:, :, :-1])
    with pytest.raises(ValueError, match="scan"):
        lesion_report(mask, lobe, spacing, scan=scan.astype(np.float32))
    # nothing kept: no lesion rows, the lobes still reported
    none = lesion_report(np.zeros_like(mask), lobe, spacing, scan=scan)
    assert none["density"]["lesions"]["voxels"].shape == (0,) and none["density"]["lesions"]["percentiles_hu"].shape == (0, 3)
    assert none["density"]["lobes"][2]["lesion"]["voxels"] == 0 and np.isnan(none["density"]["lobes"][2]["lesion"]["mean_hu"])


def test_density_error_paths_launch_nothing():
    from dram_amd._lib import DramHipError, call, lib
    c = DC.case("odd_size_105")
    scan, labels = torch.from_numpy(c["scan"].copy()).cuda(), torch.from_numpy(c["labels"].copy()).cuda()
    out = torch.full((5, 8), -7, dtype=torch.int64, device="cuda")
    args = lambda n, hist, nbins, width=1: (scan.data_ptr(), labels.data_ptr(), 0, None, n, out[0].data_ptr(), out[1].data_ptr(),
                                            out[2].data_ptr(), out[3].data_ptr(), out[4].data_ptr(), hist, -1024, width, nbins, 105, _st())
    assert lib.dram_label_density(*args(256, None, 0)) == -1 and lib.dram_label_density(*args(5, None, 16)) == -1
    assert lib.dram_label_density(*args(5, out.data_ptr(), 16, 0)) == -1
    with pytest.raises(DramHipError, match="together"):
        call("dram_label_density", *args(5, out.data_ptr(), 0))
    torch.cuda.synchronize()
    assert bool((out == -7).all())
