"""csrc/distance.hip and dram_amd/surface.py on the device against the numpy restatement (tests/surface_restatement.py, itself held
against scipy.ndimage by tests/test_surface_cpu.py).  The distance transform is compared bit for bit (float32) with the
brute-force definition; counts are integers and compared exactly."""
import math

import numpy as np
import pytest
import torch

import surface_restatement as SR

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()            # a copy: the shared cases are read-only arrays


def _st():
    return torch.cuda.current_stream().cuda_stream


def gpu_edt(feature, spacing):
    from dram_amd._lib import call, lib
    D, H, W = feature.shape
    f = _dev(feature)
    dist = torch.full(feature.shape, -7.0, dtype=torch.float32, device="cuda")      # poisoned: every voxel must be written
    ws_bytes = lib.dram_edt_ws_bytes(D, H, W)
    ws = torch.full((ws_bytes // 8,), float("nan"), dtype=torch.float64, device="cuda")
    call("dram_edt", f.data_ptr(), dist.data_ptr(), *[float(s) for s in spacing], D, H, W, ws.data_ptr(), ws_bytes, _st())
    return dist.cpu().numpy()


def gpu_surface(mask):
    from dram_amd._lib import call
    m = _dev(mask)
    surf = torch.full(mask.shape, 9, dtype=torch.uint8, device="cuda")
    count = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    call("dram_mask_surface", m.data_ptr(), surf.data_ptr(), count.data_ptr(), *mask.shape, _st())
    return surf.cpu().numpy(), int(count.item())


@pytest.mark.parametrize("name", list(SR.CASES))
def test_edt_equals_the_definition_bit_for_bit(name):
    """The long-axis cases (SR.LONG = 65) are one more than a lap of each pass: edt_x resolves a row in ballots of 64 voxels,
    a block of edt_axis produces EDT_OC = 64 outputs per lap from LDS chunks of EDT_SC = 64 sources (csrc/distance.hip)."""
    feature, spacing = SR.feature_of(name), SR.CASES[name][1]
    ref = SR.expected(name)
    dist = gpu_edt(feature, spacing)
    assert dist.dtype == np.float32 and np.array_equal(dist.view(np.uint32), ref.view(np.uint32))
    assert np.all(dist[feature != 0] == 0)
    if not feature.any():
        assert np.all(np.isposinf(dist))
    if name in SR.UNIT_CASES and feature.any():
        d2 = SR.brute_d2_of(name)
        assert np.array_equal(d2, np.rint(d2)) and np.array_equal(dist, np.sqrt(d2).astype(np.float32))


def test_distance_transform_takes_any_non_zero_value_and_any_input_kind():
    from dram_amd import distance_transform
    name = "random_3x67x130"
    feature, spacing = SR.feature_of(name), SR.CASES[name][1]
    ref = SR.expected(name)
    for given in (feature * np.uint8(200), feature.astype(bool), _dev(feature.astype(np.float32))):
        dist = distance_transform(given, spacing)
        assert dist.is_cuda and dist.dtype == torch.float32 and np.array_equal(dist.cpu().numpy().view(np.uint32), ref.view(np.uint32))


def test_edt_refuses_sizes_above_the_bound_and_a_short_workspace():
    from dram_amd._lib import DramHipError, call, lib
    cap = lib.dram_edt_max_dim()
    assert cap >= 1024
    f = torch.zeros(cap + 1, dtype=torch.uint8, device="cuda")
    dist = torch.full((cap + 1,), -7.0, dtype=torch.float32, device="cuda")
    ws = torch.zeros(2 * (cap + 1), dtype=torch.float64, device="cuda")
    for shape in ((1, 1, cap + 1), (1, cap + 1, 1), (cap + 1, 1, 1)):
        with pytest.raises(DramHipError, match="sizes must be"):
            call("dram_edt", f.data_ptr(), dist.data_ptr(), 1.0, 1.0, 1.0, *shape, ws.data_ptr(), ws.numel() * 8, _st())
    need = lib.dram_edt_ws_bytes(1, 1, cap)
    with pytest.raises(DramHipError, match="workspace too small"):
        call("dram_edt", f.data_ptr(), dist.data_ptr(), 1.0, 1.0, 1.0, 1, 1, cap, ws.data_ptr(), need - 1, _st())
    torch.cuda.synchronize()
    assert bool((dist == -7.0).all())                                     # nothing was launched
    # the bound itself is accepted: one row of cap voxels, the feature at its far end
    f[cap - 1] = 1
    call("dram_edt", f.data_ptr(), dist.data_ptr(), 1.0, 1.0, 0.5, 1, 1, cap, ws.data_ptr(), need, _st())
    got = dist[:cap].cpu().numpy()
    assert np.array_equal(got, (np.arange(cap - 1, -1, -1, dtype=np.float64) * 0.5).astype(np.float32)) and float(dist[cap]) == -7.0


def _surface_masks():
    rng = np.random.default_rng(3)
    dense = (rng.random((5, 9, 70)) < 0.8).astype(np.uint8) * 3           # non-zero means set
    dense[0], dense[-1], dense[:, 0], dense[:, -1], dense[:, :, 0], dense[:, :, -1] = 1, 1, 1, 1, 1, 1
    pred, ref = SR.blob_pair()
    return {"full": np.ones((4, 5, 6), np.uint8), "dense": dense, "blob_pred": pred, "blob_ref": ref,
            "empty": np.zeros((3, 4, 5), np.uint8), "thin": np.ones((1, 1, 9), np.uint8), "one": np.ones((1, 1, 1), np.uint8)}


SURFACE_MASKS = _surface_masks()


@pytest.mark.parametrize("name", list(SURFACE_MASKS))
def test_mask_surface_and_its_count(name):
    mask = SURFACE_MASKS[name]
    ref = SR.surface(mask)
    surf, n = gpu_surface(mask)
    assert np.array_equal(surf, ref) and n == int(ref.sum())
    from dram_amd import mask_surface
    surf2, n2 = mask_surface(mask)
    assert n2 == n and surf2.dtype == torch.uint8 and np.array_equal(surf2.cpu().numpy(), ref)


def test_surface_gather_is_the_sorted_multiset():
    from dram_amd._lib import call
    from dram_amd.surface import gather_surface
    rng = np.random.default_rng(8)
    shape = (3, 67, 130)
    surf = (rng.random(shape) < 0.3).astype(np.uint8) * 5
    surf[0, 0, :64] = 0                                                    # a wave without a surface voxel
    dist = rng.random(shape).astype(np.float32)
    dist[1, 2, 3] = np.inf
    surf[1, 2, 3] = 1
    want = np.sort(dist[surf != 0])
    got = gather_surface(_dev(surf), _dev(dist), len(want)).cpu().numpy()
    assert np.array_equal(np.sort(got), want)
    # a short output is not written past its end, and the cursor still counts every surface voxel
    cap = 100
    out = torch.full((cap + 64,), -7.0, dtype=torch.float32, device="cuda")
    cursor = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    s, d = _dev(surf), _dev(dist)
    call("dram_surface_gather", s.data_ptr(), d.data_ptr(), out.data_ptr(), cursor.data_ptr(), cap, s.numel(), _st())
    assert int(cursor.item()) == len(want) and bool((out[cap:] == -7.0).all()) and bool((out[:cap] != -7.0).all())
    none = gather_surface(torch.zeros(shape, dtype=torch.uint8, device="cuda"), d, 0)
    assert none.numel() == 0


def _close(a, b, rel=1e-12):
    return abs(a - b) <= rel * abs(b)


def test_surface_distances_end_to_end():
    from dram_amd import surface_distances
    pred, ref = SR.blob_pair()
    want = SR.blob_metrics()
    got = surface_distances(_dev(pred), ref, SR.ANISO, tolerances_mm=SR.TOLERANCES)
    assert set(got) == {"hd", "hd95", "assd", "n_pred_surface", "n_ref_surface", "nsd"}
    n = want["n_pred_surface"] + want["n_ref_surface"]
    assert got["n_pred_surface"] == want["n_pred_surface"] > 100 and got["n_ref_surface"] == want["n_ref_surface"] > 100
    assert got["hd"] == want["hd"] and math.isfinite(got["hd"]) and got["hd"] > 0
    assert list(got["nsd"]) == list(SR.TOLERANCES)
    for tol in SR.TOLERANCES:
        assert round(got["nsd"][tol] * n) == want["within"][tol] and got["nsd"][tol] == want["within"][tol] / n
    assert 0 < want["within"][0.0] < want["within"][1.0] < want["within"][2.5] < n        # the tolerances tell something apart
    assert _close(got["assd"], want["assd"]) and _close(got["hd95"], want["hd95"])
    other = surface_distances(pred, ref, SR.ANISO, percentile=50.0)
    both = SR.surface_metrics(pred, ref, SR.ANISO, 50.0)
    assert "hd50" in other and "hd95" not in other and other["nsd"] == {} and _close(other["hd50"], both["hd50"])
    same = surface_distances(pred, pred, SR.ANISO, tolerances_mm=(0.0,))
    assert same["hd"] == 0.0 and same["assd"] == 0.0 and same["hd95"] == 0.0 and same["nsd"][0.0] == 1.0


def test_surface_distances_of_empty_masks():
    from dram_amd import surface_distances
    pred, _ = SR.blob_pair()
    zero = np.zeros_like(pred)
    both = surface_distances(zero, zero, SR.ANISO, tolerances_mm=(1.0,))
    assert all(math.isnan(both[k]) for k in ("hd", "hd95", "assd")) and math.isnan(both["nsd"][1.0])
    assert both["n_pred_surface"] == 0 and both["n_ref_surface"] == 0
    for a, b in ((pred, zero), (zero, pred)):
        one = surface_distances(a, b, SR.ANISO, tolerances_mm=(1.0, 2.0))
        assert one["hd"] == math.inf and one["hd95"] == math.inf and one["assd"] == math.inf and one["nsd"] == {1.0: 0.0, 2.0: 0.0}
        assert one["n_pred_surface"] + one["n_ref_surface"] == SR.blob_metrics()["n_pred_surface"]


def test_lesion_report_with_and_without_the_surface_metrics():
    from dram_amd import lesion_report, surface_distances
    pred, ref = SR.blob_pair()
    lobe = np.ones(pred.shape, np.uint8)
    plain = lesion_report(pred, lobe, SR.ANISO, reference=ref)
    assert set(plain) == {"mask", "labels", "n_lesions", "volumes_ml", "bboxes", "lobes", "n_reference", "n_found", "sensitivity",
                          "n_false"}
    assert set(lesion_report(pred, lobe, SR.ANISO)) == {"mask", "labels", "n_lesions", "volumes_ml", "bboxes", "lobes"}
    rep = lesion_report(pred, lobe, SR.ANISO, reference=ref, surface=True, tolerances_mm=SR.TOLERANCES)
    assert set(rep) == set(plain) | {"surface"}
    for k in ("n_lesions", "n_reference", "n_found", "sensitivity", "n_false", "lobes"):
        assert rep[k] == plain[k]
    assert torch.equal(rep["mask"], plain["mask"]) and torch.equal(rep["labels"], plain["labels"])
    assert rep["surface"] == surface_distances(pred, ref, SR.ANISO, tolerances_mm=SR.TOLERANCES)
    # the metrics are those of the FILTERED mask: without its smallest blob the prediction has fewer surface voxels
    small = lesion_report(pred, lobe, SR.ANISO, min_volume_mm3=300.0, reference=ref, surface=True)
    assert small["n_lesions"] < plain["n_lesions"]
    assert small["surface"] == surface_distances(small["mask"], ref, SR.ANISO)
    assert small["surface"]["n_pred_surface"] < rep["surface"]["n_pred_surface"]
    with pytest.raises(ValueError, match="needs a reference"):
        lesion_report(pred, lobe, SR.ANISO, surface=True)
