"""CPU-side checks of the surface-distance metrics: the numpy restatements (tests/surface_restatement.py) against each other and
against scipy.ndimage, the percentile helper against numpy, and the host-side checks of dram_amd/surface.py and csrc/distance.hip
(no kernel runs)."""
import numpy as np
import pytest
import torch

import surface_restatement as SR

U = 2.0 ** -53          # fp64 unit roundoff


@pytest.mark.parametrize("name", list(SR.CASES))
def test_separable_passes_equal_the_definition_bit_for_bit(name):
    """Rounded addition is monotone, so the minimum commutes with it: (b) == (a) in every bit of the fp64 d2, not only of the
    float32 result."""
    feature, spacing = SR.feature_of(name), SR.CASES[name][1]
    d2 = SR.edt_passes_d2(feature, spacing)
    assert d2.dtype == np.float64 and np.array_equal(d2, SR.brute_d2_of(name))
    assert np.array_equal(SR.edt_passes(feature, spacing).view(np.uint32), SR.expected(name).view(np.uint32))
    assert np.all(SR.brute_d2_of(name)[feature != 0] == 0)
    if not feature.any():
        assert np.all(np.isposinf(d2))


@pytest.mark.parametrize("name", SR.UNIT_CASES)
def test_unit_spacing_gives_exact_integers(name):
    d2 = SR.brute_d2_of(name)
    finite = d2[np.isfinite(d2)]
    assert np.array_equal(finite, np.rint(finite))


@pytest.mark.parametrize("name", [n for n in SR.CASES if SR.feature_of(n).any()])
def test_definition_against_scipy(name):
    """Roundings, relative, to first order in u = 2^-53, for a distance sqrt(tz + ty + tx):
      here:  t = fl(d^2 * fl(s * s)) -> 2u per term (d^2 is exact); two additions of positive terms -> + 2u: d2 within 4u;
             the square root halves that and adds its own: 3u.
      scipy: t = fl(fl(d * s)^2) -> 3u per term (the product's u doubles under the square, which adds one); + 2u: d2 within 5u;
             the square root: 3.5u.
    Together 6.5u; one more u for the second-order terms and for a feature that scipy may pick in a tie within those roundings
    (its value then lies within the same bounds of the minimum): 7.5u, asserted as 8u.  A case without a feature is left out:
    scipy does not define it."""
    ndimage = pytest.importorskip("scipy.ndimage")
    feature, spacing = SR.feature_of(name), SR.CASES[name][1]
    ours = np.sqrt(SR.brute_d2_of(name))
    ref = ndimage.distance_transform_edt(feature == 0, sampling=spacing)
    assert ref.dtype == np.float64
    assert np.all(np.abs(ours - ref) <= 8 * U * ref)


def _touching_masks():
    rng = np.random.default_rng(3)
    full = np.ones((4, 5, 6), np.uint8)                                  # touches every face: the surface is the shell
    dense = (rng.random((5, 9, 70)) < 0.8).astype(np.uint8) * 3          # non-zero means set
    dense[0], dense[-1], dense[:, 0], dense[:, -1], dense[:, :, 0], dense[:, :, -1] = 1, 1, 1, 1, 1, 1
    pred, ref = SR.blob_pair()
    return {"full": full, "dense": dense, "blob_pred": pred, "blob_ref": ref, "empty": np.zeros((3, 4, 5), np.uint8),
            "thin": np.ones((1, 1, 9), np.uint8)}


TOUCHING = _touching_masks()


@pytest.mark.parametrize("name", list(TOUCHING))
def test_surface_like_scipy_erosion(name):
    ndimage = pytest.importorskip("scipy.ndimage")
    mask = TOUCHING[name]
    eroded = ndimage.binary_erosion(mask != 0, ndimage.generate_binary_structure(3, 1), border_value=0)
    surf = SR.surface(mask)
    assert surf.dtype == np.uint8 and np.array_equal(surf != 0, (mask != 0) & ~eroded)
    if name == "full":
        assert int(surf.sum()) == 4 * 5 * 6 - 2 * 3 * 4


@pytest.mark.parametrize("q", [0.0, 5.0, 37.5, 50.0, 95.0, 99.9, 100.0])
@pytest.mark.parametrize("n", [1, 2, 3, 20, 21, 1000])
def test_percentile_helper_like_numpy(n, q):
    from dram_amd.surface import percentile_lerp, percentile_position
    rng = np.random.default_rng(n)
    a = rng.random(n // 2).astype(np.float32)
    b = (rng.random(n - n // 2) * 7).astype(np.float32)
    both = np.sort(np.concatenate((a, b)).astype(np.float64))
    lo, hi, t = percentile_position(n, q)
    assert 0 <= lo <= hi <= n - 1 and hi - lo <= 1 and 0.0 <= t < 1.0
    got = percentile_lerp(both[lo], both[hi], t)
    ref = float(np.percentile(both, q))
    assert abs(got - ref) <= 1e-12 * abs(ref)


def test_percentile_helper_edges():
    from dram_amd.surface import _float32_at_most, _percentile_name, percentile_lerp, percentile_position
    assert percentile_lerp(np.inf, np.inf, 0.3) == np.inf
    assert percentile_lerp(1.0, np.inf, 0.3) == np.inf
    with pytest.raises(ValueError):
        percentile_position(0, 50.0)
    with pytest.raises(ValueError):
        percentile_position(5, 100.5)
    assert _percentile_name(95.0) == "hd95" and _percentile_name(99.5) == "hd99.5"
    for v in (0.1, 0.8, 1.0, 2.5, 0.0, 1e-50):
        f = _float32_at_most(v)
        assert f <= v and float(np.float32(f)) == f and float(np.nextafter(np.float32(f), np.float32(np.inf))) > v


def test_restated_metrics_on_a_hand_made_pair():
    """Two single voxels 3 voxels apart along y (spacing 0.7): both directed sets are {2.1}."""
    pred = np.zeros((2, 6, 3), np.uint8)
    ref = np.zeros_like(pred)
    pred[1, 1, 1], ref[1, 4, 1] = 1, 1
    m = SR.surface_metrics(pred, ref, SR.ANISO, 95.0, (2.0, 2.2))
    d = float(np.float32(np.sqrt(9.0 * (np.float64(0.7) * np.float64(0.7)))))
    assert m["n_pred_surface"] == 1 and m["n_ref_surface"] == 1
    assert m["hd"] == d and m["hd95"] == d and m["assd"] == d and m["nsd"] == {2.0: 0.0, 2.2: 1.0}
    empty = SR.surface_metrics(np.zeros_like(pred), np.zeros_like(pred), SR.ANISO, 95.0, (1.0,))
    assert np.isnan(empty["hd"]) and np.isnan(empty["nsd"][1.0])
    one = SR.surface_metrics(pred, np.zeros_like(pred), SR.ANISO, 95.0, (1.0,))
    assert one["hd"] == np.inf and one["hd95"] == np.inf and one["assd"] == np.inf and one["nsd"][1.0] == 0.0


def test_host_side_argument_checks():
    """Every one of these is refused before a device is touched."""
    import dram_amd
    from dram_amd import surface as S
    assert dram_amd.surface_distances is S.surface_distances and dram_amd.distance_transform is S.distance_transform
    assert dram_amd.mask_surface is S.mask_surface
    vol = np.zeros((2, 3, 4), np.uint8)
    for bad in ((1.0, 1.0), (1.0, 1.0, 0.0), (1.0, -1.0, 1.0), (1.0, np.nan, 1.0), (np.inf, 1.0, 1.0)):
        with pytest.raises(ValueError, match="spacing"):
            S.distance_transform(vol, bad)
        with pytest.raises(ValueError, match="spacing"):
            S.surface_distances(vol, vol, bad)
    with pytest.raises(ValueError, match="volume"):
        S.distance_transform(np.zeros((3, 4), np.uint8), (1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="volume"):
        S.mask_surface(np.zeros((1, 2, 3, 4), np.uint8))
    with pytest.raises(ValueError, match="same shape"):
        S.surface_distances(vol, np.zeros((2, 3, 5), np.uint8), (1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="percentile"):
        S.surface_distances(vol, vol, (1.0, 1.0, 1.0), percentile=101.0)
    with pytest.raises(ValueError, match="tolerances"):
        S.surface_distances(vol, vol, (1.0, 1.0, 1.0), tolerances_mm=(1.0, -0.5))
    with pytest.raises(ValueError, match="gather_surface"):
        S.gather_surface(torch.zeros((2, 3, 4), dtype=torch.uint8), torch.zeros((2, 3, 4)), 0)


def test_edt_workspace_query_and_entry_checks_without_a_gpu():
    from dram_amd import _lib
    lib = _lib.lib
    cap = lib.dram_edt_max_dim()
    assert cap >= 1024
    ws = lib.dram_edt_ws_bytes
    assert ws(1, 1, 1) >= 12 and ws(1, 1, 1) % 8 == 0
    # an int32 and an fp64 per voxel, the second on an 8-byte boundary
    assert ws(3, 5, 7) == (3 * 5 * 7 * 4 + 7) // 8 * 8 + 3 * 5 * 7 * 8
    sizes = [(1, 1, 1), (1, 1, 2), (1, 3, 2), (2, 3, 2), (3, 67, 130), (64, 64, 64), (65, 64, 64), (1, cap, cap), (300, 512, 512)]
    got = [ws(*s) for s in sizes]
    assert all(a < b for a, b in zip(got, got[1:]))                       # monotone in the voxel count
    assert ws(300, 512, 512) == 300 * 512 * 512 * 12
    for refused in ((0, 4, 4), (4, -1, 4), (cap + 1, 1, 1), (1, cap + 1, 1), (1, 1, cap + 1), (2048, 2048, 512)):
        assert ws(*refused) == 0
    assert b"edt_ws_bytes" in lib.dram_last_error()
    one = 16                                                              # a stand-in address: nothing is dereferenced before the checks
    with pytest.raises(_lib.DramHipError, match="null pointer"):
        _lib.call("dram_edt", None, one, 1.0, 1.0, 1.0, 2, 2, 2, one, 1 << 20, None)
    with pytest.raises(_lib.DramHipError, match="sizes must be"):
        _lib.call("dram_edt", one, one, 1.0, 1.0, 1.0, 2, cap + 1, 2, one, 1 << 40, None)
    with pytest.raises(_lib.DramHipError, match="spacing"):
        _lib.call("dram_edt", one, one, 1.0, 0.0, 1.0, 2, 2, 2, one, 1 << 20, None)
    with pytest.raises(_lib.DramHipError, match="spacing"):
        _lib.call("dram_edt", one, one, 1.0, 1.0, float("nan"), 2, 2, 2, one, 1 << 20, None)
    with pytest.raises(_lib.DramHipError, match=r"\(-2\).*workspace too small"):
        _lib.call("dram_edt", one, one, 1.0, 1.0, 1.0, 2, 2, 2, one, ws(2, 2, 2) - 1, None)
    with pytest.raises(_lib.DramHipError, match="null pointer"):
        _lib.call("dram_mask_surface", one, None, one, 2, 2, 2, None)
    with pytest.raises(_lib.DramHipError, match="sizes must be"):
        _lib.call("dram_mask_surface", one, one, one, 2, 0, 2, None)
    with pytest.raises(_lib.DramHipError, match="null pointer"):
        _lib.call("dram_surface_gather", one, one, one, None, 4, 8, None)
    with pytest.raises(_lib.DramHipError, match="capacity"):
        _lib.call("dram_surface_gather", one, one, None, one, 4, 8, None)
    with pytest.raises(_lib.DramHipError, match="nvox"):
        _lib.call("dram_surface_gather", one, one, one, one, 4, 0, None)
