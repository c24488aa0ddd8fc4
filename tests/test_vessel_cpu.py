"""Host side of the pseudo-vessel mask (dram_amd/vessels.py) and its oracle (tests/vessel_restatement.py) against
scipy.ndimage, numpy.linalg and analytic anchors; the measured tolerances recorded in tests/vessel_cases.py; the argument
checks of the C ABI.  No kernel is launched."""
import numpy as np
import pytest
from scipy import ndimage

import vessel_cases as VC
import vessel_restatement as VR


def _ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


@pytest.mark.parametrize("sigma", [0.3, 0.8, 2.3, 7.9])
@pytest.mark.parametrize("order", [0, 1, 2])
def test_taps_equal_scipys_impulse_response(sigma, order):
    from dram_amd.vessels import gaussian_derivative_taps, gaussian_radius
    ref = VR.scipy_taps(sigma, order)
    taps = gaussian_derivative_taps(sigma, order)
    r = gaussian_radius(sigma)
    assert r == VR.radius_of(sigma) and taps.dtype == np.float64 and taps.shape == ref.shape == (2 * r + 1,)
    same = taps == ref
    assert np.all(same | (_ulps(taps, ref) <= 2.0)), _ulps(taps, ref)[~same].max()
    if order == 1:                                   # the response to an impulse FALLS on the far side: taps[r + 1] < 0 < taps[r - 1]
        assert taps[r + 1] < 0 < taps[r - 1] and np.sign(taps[r + 1]) == np.sign(ref[r + 1])
        assert np.array_equal(taps, -taps[::-1])
    else:
        assert np.array_equal(taps, taps[::-1])
    assert np.array_equal(gaussian_derivative_taps(sigma, order, radius=r + 2)[2:-2] != 0, taps != 0)


def test_taps_refuse_bad_arguments():
    from dram_amd.vessels import gaussian_derivative_taps
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sigma"):
            gaussian_derivative_taps(bad, 0)
    with pytest.raises(ValueError, match="order"):
        gaussian_derivative_taps(1.0, 3)


def test_restatement_equals_gaussian_filter_with_unrounded_taps():
    rng = np.random.default_rng(1)
    v = rng.normal(size=(9, 14, 17)).astype(np.float32).astype(np.float64)      # the restatement takes fp32 voxels
    sv = (0.8, 2.9, 1.3)                              # the y axis (14) is barely longer than its radius (12)
    h = VR.hessian(v, sv, clip=None, table=VR.tap_table(sv, rounded=False), scaled=False)
    for k, name in enumerate(VR.ORDER):
        ref = ndimage.gaussian_filter(v, sigma=sv, order=VR.ORDERS[name], mode="reflect", truncate=4.0)
        assert np.abs(h[k] - ref).max() <= 1e-13 * np.abs(ref).max(), name
    short = rng.normal(size=(5, 9, 33)).astype(np.float32).astype(np.float64)               # y shorter than its radius: the reflection folds more than once
    h = VR.hessian(short, sv, clip=None, table=VR.tap_table(sv, rounded=False), scaled=False)
    ref = ndimage.gaussian_filter(short, sigma=sv, order=(0, 2, 0), mode="reflect", truncate=4.0)
    assert np.abs(h[1] - ref).max() <= 1e-13 * np.abs(ref).max()
    # the package's own taps give the same Hessian
    from dram_amd.vessels import gaussian_derivative_taps
    own = VR.hessian(v, sv, table=VR.tap_table(sv, taps_of=gaussian_derivative_taps))
    assert np.abs(own - VR.hessian(v, sv)).max() == 0.0


N, TUBE_SD, AMP = 41, 2.0, 400.0


def _profile(d2):
    return AMP * np.exp(-d2 / (2.0 * TUBE_SD ** 2))


def _grid():
    return np.meshgrid(*[np.arange(N, dtype=np.float64) - N // 2] * 3, indexing="ij")


def _tube(direction):
    z, y, x = _grid()
    u = np.asarray(direction, dtype=np.float64)
    u = u / np.linalg.norm(u)
    along = z * u[0] + y * u[1] + x * u[2]
    return _profile(z * z + y * y + x * x - along * along)


def _centre(a):
    return a[..., N // 2, N // 2, N // 2]


def _v_at_centre(vol, sigma, c=50.0):
    return float(_centre(VR.tube_measure(VR.eigenvalues(VR.hessian(vol, (sigma,) * 3)), c=c)))


def test_analytic_anchors_on_a_gaussian_tube():
    tube = _tube((1, 0, 0))
    response = {}
    for sigma, expected in ((1.0, -64.0), (2.0, -100.0), (3.0, -85.207)):
        l = _centre(VR.eigenvalues(VR.hessian(tube, (sigma,) * 3)))
        closed = -AMP * TUBE_SD ** 2 * sigma ** 2 / (TUBE_SD ** 2 + sigma ** 2) ** 2
        assert abs(closed - expected) < 1e-3
        assert abs(l[0]) < 0.1
        assert abs(l[1] - closed) <= 1e-3 * abs(closed) and abs(l[2] - closed) <= 1e-3 * abs(closed), (sigma, l)
        response[sigma] = abs(l[2])
    assert response[2.0] > response[1.0] and response[2.0] > response[3.0]          # the response peaks at sigma = s
    v_tube = _v_at_centre(tube, 2.0)
    assert v_tube > 0.5
    z, y, x = _grid()
    assert _v_at_centre(_profile(z * z), 2.0) < 1e-6                                 # a sheet
    assert _v_at_centre(_profile(z * z + y * y + x * x), 2.0) < 0.25 * v_tube        # a blob
    for direction in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
        assert _v_at_centre(_tube(direction), 2.0) > 0.9 * v_tube, direction
    dark = VR.tube_measure(VR.eigenvalues(VR.hessian(AMP - tube, (2.0,) * 3)), c=50.0)
    assert _centre(dark) == 0.0 and np.all(dark[:, N // 2, N // 2] == 0.0)           # a dark tube on bright: exactly 0


def test_tie_and_sign_rules_on_diagonal_matrices():
    def l_of(*d):
        return VR.eigenvalues(np.array([d[0], d[1], d[2], 0, 0, 0], dtype=np.float64).reshape(6, 1))[:, 0]
    assert list(l_of(-60, -1, -50)) == [-1, -50, -60]
    assert list(l_of(2, -3, -2)) == [-2, 2, -3]                  # equal magnitudes: the smaller value first
    assert list(l_of(3, -3, -3)) == [-3, -3, 3]
    assert list(l_of(0, 0, 0)) == [0, 0, 0]
    v = lambda *d: float(VR.tube_measure(l_of(*d).reshape(3, 1), c=20.0)[0])
    assert v(-1, -50, -60) > 0.3
    assert v(2, -3, -2) == 0.0 and v(3, -3, -3) == 0.0           # l2 or l3 positive
    assert v(1, 5, -7) == 0.0 and v(1, 5, 7) == 0.0 and v(-1, 5, -7) == 0.0
    assert v(0, 0, 0) == 0.0                                     # 0 / 0: not finite
    assert v(0, -4, -4) > 0.0 and v(0, 0, -1) == 0.0             # l2 = 0 counts as l2 >= 0
    # the mirror of the device's solver orders the same way
    h = VC.vesselness_h6()[:, :14]
    assert np.array_equal(VC.jacobi_eigenvalues(h), VR.eigenvalues(h.astype(np.float64)))


def test_recorded_tolerances_are_the_measured_ones():
    """The solver's own error over the hand-made Hessians and the end-to-end tolerance, measured here as tests/vessel_cases.py
    says, must not exceed what it records (and the record must not be padded: within 5 %)."""
    err = VC.measured_solver_error(VC.vesselness_h6())
    assert err <= VC.EIG_TOLERANCE / 4 <= 1.05 * err, err
    assert VC.measured_solver_error(VC.vesselness_h6()[:, :]) < 1e-14
    scan, lobe = VC.e2e_volume()
    assert scan.shape == VC.E2E_SHAPE and scan.min() >= VC.E2E_CLIP[0] and scan.max() <= VC.E2E_CLIP[1]
    tol = VC.measured_e2e_tolerance(None, lobe)
    assert tol <= VC.E2E_TOLERANCE <= 1.05 * tol, tol
    ref = VC.e2e_vesselness(None, lobe)
    inside = lobe > 0
    near = (np.abs(ref - VC.MASK_THRESHOLD) <= VC.E2E_TOLERANCE) & inside
    assert 0 < near.sum() <= 0.01 * inside.sum()                 # the threshold of the mask test: the reference alone meets the 1 %
    assert VR.mask(ref, lobe, VC.MASK_THRESHOLD).sum() > 50
    # the content is what it claims: the thin tube answers, the sheet does not
    assert ref[14, 21, 15] > 0.5 and ref[30, 35, 20] < 1e-3
    assert np.array_equal(ref, VR.vesselness(scan, VC.E2E_SPACING, VC.E2E_SIGMAS, lobe=lobe))


def test_hessian_cases_cover_the_tiles():
    c = VC.HESSIAN_CASES
    assert c["x_tiles_D1"][0][2] > 2 * VC.VX_T and c["x_tiles_D1"][0][0] * c["x_tiles_D1"][0][1] > 2 * VC.VX_ROWS
    assert c["y_tiles"][0][1] > 2 * VC.VA_LT and c["y_tiles"][0][2] > 2 * VC.VA_TX
    assert c["z_tiles"][0][0] > 2 * VC.VA_LT and c["z_tiles"][0][1] * c["z_tiles"][0][2] > 2 * VC.VA_TX
    assert c["short"][0][1] < VR.radius_of(c["short"][1][1])
    assert VR.radius_of(c["cap"][1][1]) == VC.MAX_RADIUS
    for name in c:
        v = VC.hessian_input(name)
        assert v.min() < -1150 and v.max() > 350, name          # values outside the clip window are present


def test_norm_max_case_puts_its_maxima_where_it_says():
    """The planted Hessian is the largest norm and lies past 4096 x 256 voxels; once the lobe leaves it out the largest is the
    one planted in the first lap; both laps hold lobe voxels; the three expectations differ where they must."""
    h6, lobes = VC.norm_max_large()
    S, cap = h6.shape[1], VC.NORM_MAX_CAP
    assert S == VC.NORM_MAX_S == cap + 300 and h6.dtype == np.float32
    norms = VR.frobenius32(h6)
    assert norms.argmax() == VC.NORM_MAX_SECOND_LAP >= cap
    assert norms[:cap].argmax() == VC.NORM_MAX_FIRST_LAP and norms[VC.NORM_MAX_FIRST_LAP] > 2 * np.delete(norms, [
        VC.NORM_MAX_FIRST_LAP, VC.NORM_MAX_SECOND_LAP]).max()
    assert norms[VC.NORM_MAX_SECOND_LAP] > 2 * norms[VC.NORM_MAX_FIRST_LAP]
    assert list(lobes) == ["no_lobe", "lobe_holds_the_maximum", "lobe_leaves_it_out"] and lobes["no_lobe"] is None
    holds, leaves = lobes["lobe_holds_the_maximum"], lobes["lobe_leaves_it_out"]
    assert holds[VC.NORM_MAX_SECOND_LAP] and not leaves[VC.NORM_MAX_SECOND_LAP] and leaves[VC.NORM_MAX_FIRST_LAP]
    for lobe in (holds, leaves):
        assert lobe.dtype == np.uint8 and 0 < (lobe[:cap] > 0).mean() < 1 and 0 < (lobe[cap:] > 0).sum() < 300 and lobe.max() > 1
    half = np.float32(0.5)
    assert VR.frangi_c(h6) == VR.frangi_c(h6, holds) == half * norms[VC.NORM_MAX_SECOND_LAP]
    assert VR.frangi_c(h6, leaves) == half * norms[VC.NORM_MAX_FIRST_LAP] == half * norms[leaves > 0].max()
    # the norm is the fp64 expression rounded once (exact integers here)
    assert norms[VC.NORM_MAX_SECOND_LAP] == np.float32(np.sqrt(100.0 ** 2 + 200.0 ** 2 + 150.0 ** 2 + 2 * (50.0 ** 2 + 75.0 ** 2 + 25.0 ** 2)))


def test_argument_errors_are_reported_without_a_gpu():
    from dram_amd import _lib
    q, S = 16, 5 * 7 * 9
    assert _lib.lib.dram_vessel_max_radius() == VC.MAX_RADIUS
    need = _lib.lib.dram_hessian_ws_bytes(5, 7, 9)
    assert need == 9 * S * 4 and _lib.lib.dram_hessian_ws_bytes(0, 7, 9) == 0 and _lib.lib.dram_hessian_ws_bytes(2048, 2048, 2048) == 0
    import ctypes
    rad = lambda *r: (ctypes.c_int * 3)(*r)
    sv = (ctypes.c_double * 3)(1.0, 1.0, 1.0)
    inf = float("inf")
    hess = lambda **kw: [kw.get("scan", q), kw.get("dtype", 0), -inf, inf, q, kw.get("radius", rad(4, 4, 4)), kw.get("sv", sv),
                         kw.get("D", 5), 7, 9, q, q, kw.get("ws_bytes", need), None]
    with pytest.raises(_lib.DramHipError, match="hessian: null pointer"):
        _lib.call("dram_hessian", *hess(scan=None))
    with pytest.raises(_lib.DramHipError, match="hessian: dtype"):
        _lib.call("dram_hessian", *hess(dtype=2))
    with pytest.raises(_lib.DramHipError, match="hessian: sizes"):
        _lib.call("dram_hessian", *hess(D=0))
    with pytest.raises(_lib.DramHipError, match="radius 33 of axis 1"):
        _lib.call("dram_hessian", *hess(radius=rad(4, VC.MAX_RADIUS + 1, 4)))
    with pytest.raises(_lib.DramHipError, match="sigma in voxels"):
        _lib.call("dram_hessian", *hess(sv=(ctypes.c_double * 3)(1.0, 0.0, 1.0)))
    assert _lib.lib.dram_hessian(*hess(ws_bytes=need - 1)) == -2
    with pytest.raises(_lib.DramHipError, match="hessian: workspace too small"):
        _lib.call("dram_hessian", *hess(ws_bytes=need - 1))
    with pytest.raises(_lib.DramHipError, match="hessian_norm_max: null pointer"):
        _lib.call("dram_hessian_norm_max", q, None, S, None, None)
    with pytest.raises(_lib.DramHipError, match="hessian_norm_max: S"):
        _lib.call("dram_hessian_norm_max", q, None, 0, q, None)
    with pytest.raises(_lib.DramHipError, match="vesselness: null pointer"):
        _lib.call("dram_vesselness", q, S, 0.5, 0.5, None, q, 0, None, None)
    with pytest.raises(_lib.DramHipError, match="vesselness: alpha and beta"):
        _lib.call("dram_vesselness", q, S, 0.0, 0.5, q, q, 0, None, None)
    with pytest.raises(_lib.DramHipError, match="vesselness: S"):
        _lib.call("dram_vesselness", q, 1 << 31, 0.5, 0.5, q, q, 0, None, None)
    with pytest.raises(_lib.DramHipError, match="vessel_mask: null pointer"):
        _lib.call("dram_vessel_mask", q, None, 0.5, None, S, None)
    with pytest.raises(_lib.DramHipError, match="vessel_mask: n"):
        _lib.call("dram_vessel_mask", q, None, 0.5, q, 0, None)


def test_input_checks_of_the_python_layer():
    import torch
    import dram_amd
    from dram_amd import vessels
    assert dram_amd.pseudo_vessel_mask is vessels.pseudo_vessel_mask and dram_amd.vesselness is vessels.vesselness
    v = torch.zeros(4, 5, 6, dtype=torch.int16)
    for bad in ((1.0, 1.0), (1.0, 0.0, 1.0), (1.0, float("nan"), 1.0)):
        with pytest.raises(ValueError, match="spacing must be three positive finite numbers"):
            vessels.vesselness(v, bad)
        with pytest.raises(ValueError, match="spacing"):
            vessels.hessian(v, bad, 1.0)
    with pytest.raises(ValueError, match=r"\[D,H,W\]"):
        vessels.vesselness(torch.zeros(4, 5), (1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="needs a filter radius of 40"):
        vessels._scale_tables([1.0, 0.4, 1.0], 4.0, "vesselness")
    with pytest.raises(ValueError, match="positive finite number of mm"):
        vessels._scale_tables([1.0, 1.0, 1.0], -1.0, "vesselness")
    taps, radius, sv = vessels._scale_tables([1.0, 0.7, 0.7], 3.0, "vesselness")
    assert radius == [12, 17, 17] and taps.shape == (3, 3, VC.MAX_RADIUS + 1) and taps.dtype == np.float32
    assert np.all(taps[0, :, 13:] == 0) and taps[1, 1, 1] > 0 and taps[1, 1, 0] == 0      # the sample at +1 of order 1 counts positive
    table = VR.tap_table(sv)
    assert np.array_equal(taps[2, 2, :18].astype(np.float64), table[2, 2][17:])
