"""csrc/distribution.hip and dram_amd/distribution.py on the device against the numpy restatement
(tests/distribution_restatement.py, itself held against a brute-force loop and scipy by tests/test_distribution_cpu.py): the
tables are integers and bit patterns and the report's floats are fp64 quotients of those integers, so every comparison is exact."""
import numpy as np
import pytest
import torch

import distribution_cases as XC
import distribution_restatement as XR

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


def gpu_tables(c):
    from dram_amd._lib import call
    n, nbins, nzt = c["n"], c["nbins"], XC.nzones_of(c)
    depth, p_depth = _placed(c["depth"], c["offsets"][0])
    labels, p_labels = _placed(c["labels"], c["offsets"][1])
    mask, p_mask = (None, None) if c["mask"] is None else _placed(c["mask"], c["offsets"][2])
    poison = lambda shape, dtype=torch.int64: torch.full(shape, -7, dtype=dtype, device="cuda")       # the entry initialises
    count, qsum, possum = poison((n,)), poison((n,)), poison((n, 3))
    dmin, dmax = poison((n,), torch.int32), poison((n,), torch.int32)
    hist = poison((n, nbins + 2)) if nbins else None
    zones = poison((n, nzt)) if nzt else None
    box = None if c["box"] is None else np.asarray(c["box"], dtype=np.int32)
    nz, ny, nx = c["zones"] if c["zones"] is not None else (1, 1, 1)
    call("dram_label_depth", p_depth, p_labels, XC.kind_of(c), p_mask, n, count.data_ptr(), qsum.data_ptr(), dmin.data_ptr(), dmax.data_ptr(),
         possum.data_ptr(), None if hist is None else hist.data_ptr(), c["bins_per_mm"], nbins, None if zones is None else zones.data_ptr(),
         None if box is None else box.ctypes.data, nz, ny, nx, *c["depth"].shape, _st())
    host = lambda t: None if t is None else t.cpu().numpy()
    out = {"count": host(count), "qsum": host(qsum), "dmin": host(dmin).view(np.uint32), "dmax": host(dmax).view(np.uint32),
           "possum": host(possum), "hist": host(hist), "zones": host(zones)}
    del depth, labels, mask
    return out


def _assert_tables_equal(got, ref):
    for key in XR.KEYS:
        assert (got[key] is None) == (ref[key] is None), key
        if ref[key] is not None:
            assert got[key].dtype == ref[key].dtype and got[key].shape == ref[key].shape and np.array_equal(got[key], ref[key]), key


@pytest.mark.parametrize("name", XC.names())
def test_label_depth_matches_the_restatement(name):
    c = XC.case(name)
    got = gpu_tables(c)
    _assert_tables_equal(got, XC.expected(name))
    _assert_tables_equal(gpu_tables(c), got)                                                   # no dependence on the order of the atomics
    if name in XC.SEAM_REGIMES:
        assert XC.regime(name) == XC.SEAM_REGIMES[name]
    if name.endswith("/wave") or name in XC.WAVE_ONLY:
        assert XC.regime(name) == 1


def test_both_regimes_and_label_kinds_are_exercised():
    seen = {(XC.regime(name), XC.case(name)["labels"].dtype.name, XC.case(name)["nbins"] > 0, XC.case(name)["zones"] is not None,
             XC.case(name)["mask"] is not None) for name in XC.names()}
    for regime in (0, 1):
        for kind in ("uint8", "int32"):
            assert {(h, z, m) for r, k, h, z, m in seen if r == regime and k == kind} >= {(True, True, True), (True, True, False)}, (regime, kind)
    for want in ((0, "uint8", False, False, False), (0, "int32", False, False, False), (1, "int32", False, False, False),
                 (0, "uint8", True, False, False), (1, "int32", False, True, False), (0, "uint8", False, True, False)):
        assert want in seen, want


@pytest.mark.parametrize("name", ["multi_lap_u8_hist", "skipped_i32", "mask_200", "values_bpm4", "zones_no_box", "zones_one_with_box", "n1_u8"])
def test_label_depth_python(name):
    from dram_amd import label_depth
    c = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in XC.case(name).items()}      # writable copies
    ref = XC.expected(name)
    zones = c["zones"] if c["zones"] is not None else (1, 1, 1)
    got = label_depth(torch.from_numpy(c["depth"].copy()).cuda(), torch.from_numpy(c["labels"].copy()).cuda(), c["n"], mask=c["mask"],
                      bins_per_mm=c["bins_per_mm"], nbins=c["nbins"], zones=zones, box=c["box"])
    _assert_tables_equal(got, ref)
    _assert_tables_equal(label_depth(c["depth"], c["labels"], c["n"], mask=c["mask"], bins_per_mm=c["bins_per_mm"], nbins=c["nbins"],
                                     zones=zones, box=c["box"]), ref)                          # host arrays go in as they are
    with pytest.raises(ValueError, match="float32"):
        label_depth(c["depth"].astype(np.float64), c["labels"], c["n"])
    with pytest.raises(ValueError, match="uint8 or int32"):
        label_depth(c["depth"], c["labels"].astype(np.int64), c["n"])
    with pytest.raises(ValueError, match="zones"):
        label_depth(c["depth"], c["labels"], c["n"], zones=(9, 1, 1))
    with pytest.raises(ValueError, match="box"):
        label_depth(c["depth"], c["labels"], c["n"], box=(0, 0, 0, 1, 0, 1))


def test_error_paths_launch_nothing():
    from dram_amd._lib import DramHipError, call, lib
    c = XC.case("odd_size_105")
    depth, labels = torch.from_numpy(c["depth"].copy()).cuda(), torch.from_numpy(c["labels"].copy()).cuda()
    out = torch.full((7, 5 * 66), -7, dtype=torch.int64, device="cuda")
    good = np.array([0, 3, 0, 5, 0, 7], dtype=np.int32)

    def args(n=5, kind=0, hist=out[5].data_ptr(), bpm=4, nbins=64, zones=out[6].data_ptr(), box=good, nz=3, ny=2, nx=2, D=3, H=5, W=7,
             d=depth.data_ptr(), lab=labels.data_ptr()):
        return (d, lab, kind, None, n, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), out[4].data_ptr(), hist, bpm, nbins,
                zones, None if box is None else box.ctypes.data, nz, ny, nx, D, H, W, _st())

    empty = good.copy()
    empty[3] = 0
    refused = (dict(n=0), dict(n=256), dict(kind=2), dict(hist=None), dict(nbins=0), dict(nbins=4097), dict(bpm=3), dict(bpm=0), dict(zones=None),
               dict(box=None, nz=1, ny=1, nx=1), dict(nz=9), dict(ny=0), dict(nx=-1), dict(box=empty), dict(D=0), dict(D=1 << 20, H=1 << 10, W=2),
               dict(d=depth.data_ptr() + 2), dict(kind=1, lab=labels.data_ptr() + 1))
    for kw in refused:
        assert lib.dram_label_depth(*args(**kw)) == -1, kw
    with pytest.raises(DramHipError, match="together"):
        call("dram_label_depth", *args(hist=None))
    torch.cuda.synchronize()
    assert bool((out == -7).all())


# ---- end to end
def _planted():
    """24 x 40 x 40: two lobes, each a box with an ellipsoid cap, a gap between them; one lesion touching the lung surface, one in
    the core of the other lobe, and a speck that the volume filter drops."""
    shape = (24, 40, 40)
    z, y, x = np.meshgrid(*(np.arange(s, dtype=np.float64) for s in shape), indexing="ij")
    lobe = np.zeros(shape, dtype=np.uint8)
    lobe[4:20, 6:34, 3:18] = 1
    lobe[(((z - 12) / 9.0) ** 2 + ((y - 20) / 15.0) ** 2 + ((x - 10) / 9.0) ** 2 <= 1.0) & (x < 18)] = 1
    lobe[5:19, 8:32, 22:37] = 3                                                        # label 2 is absent
    lobe[(((z - 12) / 8.0) ** 2 + ((y - 20) / 14.0) ** 2 + ((x - 30) / 9.0) ** 2 <= 1.0) & (x >= 22)] = 3
    mask = np.zeros(shape, dtype=np.uint8)
    mask[10:14, 6:10, 5:9] = 1                                                         # on the lobe's y = 6 face
    mask[10:14, 17:23, 28:32] = 1                                                      # the core of lobe 3
    mask[17, 30, 25] = 1                                                               # a speck
    mask[lobe == 0] = 0
    return mask, lobe, (2.0, 0.8, 0.8)


def _assert_row_equal(got, ref, where):
    assert sorted(got) == sorted(ref), where
    for key in ref:
        a, b = np.asarray(got[key]), np.asarray(ref[key])
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), (where, key)


def _assert_entry_equal(got, ref, where):
    assert sorted(got) == sorted(ref) == ["depth_ratio", "lesion", "parenchyma", "peripheral_share"]
    for part in ("parenchyma", "lesion"):
        _assert_row_equal(got[part], ref[part], (where, part))
    for key in ("peripheral_share", "depth_ratio"):
        assert got[key] == ref[key] or (got[key] != got[key] and ref[key] != ref[key]), (where, key)


def _assert_distribution_equal(got, ref):
    assert sorted(got["lobes"]) == sorted(ref["lobes"]) and got["box"] == ref["box"]
    for v in ref["lobes"]:
        _assert_entry_equal(got["lobes"][v], ref["lobes"][v], v)
    _assert_entry_equal(got["lungs"], ref["lungs"], "lungs")
    assert ("lesions" in got) == ("lesions" in ref)
    if "lesions" in ref:
        assert got["lesions"]["zone"] == ref["lesions"]["zone"]
        _assert_row_equal({k: v for k, v in got["lesions"].items() if k != "zone"}, {k: v for k, v in ref["lesions"].items() if k != "zone"}, "lesions")


def test_lesion_distribution_end_to_end():
    import components_restatement as CR
    from dram_amd import lesion_distribution, lesion_report, lung_depth
    mask, lobe, spacing = _planted()
    kw = dict(connectivity=1, min_volume_mm3=6.0)
    depth = lung_depth(torch.from_numpy(lobe).cuda(), spacing)
    assert depth.dtype == torch.float32 and np.array_equal(depth.cpu().numpy().view(np.uint32), XR.lung_depth(lobe, spacing).view(np.uint32))
    plain = lesion_report(mask, lobe, spacing, **kw)
    assert "distribution" not in plain and plain["n_lesions"] == 2
    rep = lesion_report(mask, lobe, spacing, distribution=True, **kw)
    assert sorted(rep) == sorted(list(plain) + ["distribution"])
    for key in plain:                                                                  # every other key as without the keyword
        if isinstance(plain[key], torch.Tensor):
            assert torch.equal(rep[key], plain[key]), key
        elif isinstance(plain[key], np.ndarray):
            assert np.array_equal(rep[key], plain[key]), key
        else:
            assert rep[key] == plain[key], key
    ref_rep = CR.report(mask, lobe, spacing, **kw)
    ref = XR.lesion_distribution(ref_rep["mask"], lobe, spacing, labels=ref_rep["labels"], n=ref_rep["n_lesions"])
    _assert_distribution_equal(rep["distribution"], ref)
    own = lesion_distribution(rep["mask"], lobe, spacing, labels=rep["labels"], n=rep["n_lesions"], depth=depth)
    _assert_distribution_equal(own, ref)
    dist = rep["distribution"]
    assert sorted(dist["lobes"]) == [1, 3] and dist["box"] == ref["box"] and dist["zones"] == (3, 2, 1)
    les = dist["lesions"]
    assert les["voxels"].shape == rep["volumes_ml"].shape and np.array_equal(les["voxels"] * (2.0 * 0.8 * 0.8) / 1000.0, rep["volumes_ml"])
    assert les["subpleural"].tolist() == [True, False]                                 # the lesion on the surface, the one in the core
    assert les["depth_min_mm"][0] == np.float32(0.8) and les["depth_min_mm"][1] > 3.0
    assert dist["lobes"][1]["peripheral_share"] > 0.0 and dist["lobes"][3]["peripheral_share"] == 0.0     # none of the core lesion in the outer third
    assert dist["lobes"][3]["depth_ratio"] > 1.0 and les["depth_mean_mm"][0] < les["depth_mean_mm"][1]
    for v in (1, 3):
        assert dist["lobes"][v]["parenchyma"]["voxels"] == rep["lobes"][v]["voxels"]
        assert dist["lobes"][v]["lesion"]["voxels"] == rep["lobes"][v]["lesion_voxels"]
    assert dist["lungs"]["parenchyma"]["voxels"] == sum(rep["lobes"][v]["voxels"] for v in (1, 3))
    # other settings travel through
    other_kw = dict(shells_mm=(0.25, 2.0), zones=(2, 3, 4), box=(2, 22, 0, 40, 1, 39), percentiles_permille=(0, 500, 1000), subpleural_mm=0.5)
    other = lesion_report(mask, lobe, spacing, distribution=True, **other_kw, **kw)
    ref2 = XR.lesion_distribution(ref_rep["mask"], lobe, spacing, labels=ref_rep["labels"], n=ref_rep["n_lesions"], **other_kw)
    _assert_distribution_equal(other["distribution"], ref2)
    assert other["distribution"]["lesions"]["subpleural"].tolist() == [False, False]
    with pytest.raises(ValueError):
        lesion_report(mask, lobe, spacing, distribution=True, shells_mm=(0.3,), **kw)
    # without lesion labels there is no "lesions" entry; nothing kept: no rows, the lobes still reported
    assert "lesions" not in lesion_distribution(mask, lobe, spacing)
    none = lesion_report(np.zeros_like(mask), lobe, spacing, distribution=True)["distribution"]
    assert none["lesions"]["voxels"].shape == (0,) and none["lesions"]["zone"] == [] and none["lesions"]["centroid"].shape == (0, 3)
    assert none["lobes"][3]["lesion"]["voxels"] == 0 and np.isnan(none["lobes"][3]["lesion"]["depth_mean_mm"])
    assert np.isnan(none["lobes"][3]["peripheral_share"]) and np.isnan(none["lungs"]["depth_ratio"])
