"""csrc/vessel.hip through the C ABI and dram_amd/vessels.py on the device against the fp64 restatement
(tests/vessel_restatement.py, itself held against scipy and analytic anchors by tests/test_vessel_cpu.py).  Inputs, tile
constants and the derived / measured tolerances: tests/vessel_cases.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import vessel_cases as VC
import vessel_restatement as VR

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()            # a copy: the shared cases are read-only arrays


def _st():
    return torch.cuda.current_stream().cuda_stream


def gpu_hessian(scan, sv, clip):
    from dram_amd import vessels
    from dram_amd._lib import call, lib
    D, H, W = scan.shape
    radius = [VR.radius_of(s) for s in sv]
    taps = np.zeros((3, 3, VC.MAX_RADIUS + 1), dtype=np.float32)
    for a in range(3):
        for o in range(3):
            taps[a, o, :radius[a] + 1] = vessels.gaussian_derivative_taps(sv[a], o, radius[a])[radius[a]::-1].astype(np.float32)
    x, t = _dev(scan), _dev(taps)
    h6 = torch.full((6, D, H, W), float("nan"), dtype=torch.float32, device="cuda")     # poisoned: every voxel must be written
    ws_bytes = lib.dram_hessian_ws_bytes(D, H, W)
    ws = torch.full((ws_bytes // 4,), float("nan"), dtype=torch.float32, device="cuda")
    lo, hi = (-np.inf, np.inf) if clip is None else clip
    call("dram_hessian", x.data_ptr(), 0 if scan.dtype == np.int16 else 1, lo, hi, t.data_ptr(), (ctypes.c_int * 3)(*radius),
         (ctypes.c_double * 3)(*sv), D, H, W, h6.data_ptr(), ws.data_ptr(), ws_bytes, _st())
    return h6.cpu().numpy()


@pytest.mark.parametrize("name", list(VC.HESSIAN_CASES))
def test_hessian_within_the_derived_bound(name):
    """1. Per output |device - restatement| <= k 2^-24 prod(sum|taps|) max|I| scale (VC.hessian_bound: the count k is written out
    there).  Two tiles and a ragged tail in every pass, an axis shorter than its radius, an axis of length 1, the radius cap,
    radius 0, anisotropic sigmas, int16 and float32, clip on and off."""
    _, sv, _, clip = VC.HESSIAN_CASES[name]
    got = gpu_hessian(VC.hessian_input(name), sv, clip)
    ref = VC.hessian_expected(name)
    bound = VC.hessian_bound(sv, VC.max_abs_input(name))
    assert got.dtype == np.float32 and np.all(np.isfinite(got))
    for k, out in enumerate(VR.ORDER):
        err = np.abs(got[k].astype(np.float64) - ref[k]).max()
        print(f"{name} {out}: max error {err:.3e}, bound {bound[k]:.3e}, max |H| {np.abs(ref[k]).max():.3e}")
        assert err <= bound[k], (name, out, err, bound[k])
    assert np.abs(ref).max() > 1.0                     # the case is no all-zero volume


def gpu_vesselness(h6, c, alpha=0.5, beta=0.5, vmax=None, want_eig=True):
    from dram_amd._lib import call
    S = h6.shape[1]
    h = _dev(h6)
    c_dev = torch.tensor([c], dtype=torch.float32, device="cuda")
    accumulate = vmax is not None
    v = _dev(vmax) if accumulate else torch.full((S,), float("nan"), dtype=torch.float32, device="cuda")
    eig = torch.full((3, S), float("nan"), dtype=torch.float64, device="cuda") if want_eig else None
    call("dram_vesselness", h.data_ptr(), S, alpha, beta, c_dev.data_ptr(), v.data_ptr(), int(accumulate),
         eig.data_ptr() if want_eig else None, _st())
    return v.cpu().numpy(), (eig.cpu().numpy() if want_eig else None)


def test_vesselness_on_hand_made_hessians():
    """2. eig against eigvalsh within the solver's own error (measured on the CPU, margin 4: VC.EIG_TOLERANCE, relative to the
    matrix' norm); V against the fp64 formula at the device's own eigenvalues within 2 ulp of fp32; accumulate keeps the larger
    value; eig = NULL is accepted."""
    h6 = VC.vesselness_h6()
    assert h6.shape[1] > 2 * 256 and h6.shape[1] % 256
    v, eig = gpu_vesselness(h6, VC.VESSELNESS_C)
    ref = VR.eigenvalues(h6.astype(np.float64))
    scale = VC.eig_scale(h6)
    err = np.abs(np.sort(eig, axis=0) - np.sort(ref, axis=0)).max(axis=0) / scale
    print(f"eigenvalues: max error {err.max():.3e} of the norm, tolerance {VC.EIG_TOLERANCE:.3e}")
    assert err.max() <= VC.EIG_TOLERANCE
    # the order: by magnitude, ties by value
    mag = np.abs(eig)
    assert np.all(mag[0] <= mag[1]) and np.all(mag[1] <= mag[2])
    assert np.all((mag[0] < mag[1]) | (eig[0] <= eig[1])) and np.all((mag[1] < mag[2]) | (eig[1] <= eig[2]))
    hand = 14                                            # the diagonal matrices come out exactly
    assert np.array_equal(eig[:, :hand], ref[:, :hand])
    want = VR.tube_measure(eig, 0.5, 0.5, np.float32(VC.VESSELNESS_C))
    w32 = want.astype(np.float32)
    assert np.all(np.abs(v.astype(np.float64) - want) <= 2.0 * np.spacing(np.maximum(w32, np.float32(1e-45))).astype(np.float64))
    assert np.all(v[(eig[1] >= 0) | (eig[2] >= 0)] == 0.0) and v[5] == 0.0 and (v > 0.3).sum() > 20
    # accumulate
    rng = np.random.default_rng(2)
    before = rng.uniform(0.0, 1.0, size=v.shape).astype(np.float32)
    after, _ = gpu_vesselness(h6, VC.VESSELNESS_C, vmax=before)
    assert np.array_equal(after, np.maximum(before, v)) and (after > before).any() and (after == before).any()
    # eig = NULL; other alpha / beta
    v2, none = gpu_vesselness(h6, VC.VESSELNESS_C, want_eig=False)
    assert none is None and np.array_equal(v2.view(np.uint32), v.view(np.uint32))
    v3, e3 = gpu_vesselness(h6, 7.0, alpha=0.3, beta=0.8)
    w3 = VR.tube_measure(e3, 0.3, 0.8, np.float32(7.0))
    assert np.all(np.abs(v3.astype(np.float64) - w3) <= 2.0 * np.spacing(np.maximum(w3.astype(np.float32), np.float32(1e-45))).astype(np.float64))


def gpu_norm_max(h6, lobe):
    from dram_amd._lib import call
    h = _dev(h6)
    lb = None if lobe is None else _dev(lobe)
    out = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")
    call("dram_hessian_norm_max", h.data_ptr(), None if lobe is None else lb.data_ptr(), h6.shape[1], out.data_ptr(), _st())
    return np.float32(out.item())


def test_norm_max_is_exact():
    """3. Frangi's c: exact equality with the restatement, with and without a lobe map; an all-zero lobe gives 1; the maximum
    sits in the last ragged element."""
    h6 = VC.vesselness_h6()
    S = h6.shape[1]
    norms = VR.frobenius32(h6)
    assert norms.argmax() == S - 1
    assert gpu_norm_max(h6, None) == VR.frangi_c(h6) == np.float32(0.5) * norms[-1]
    lobe = (np.random.default_rng(4).random(S) < 0.5).astype(np.uint8)
    lobe[-1] = 0
    c = gpu_norm_max(h6, lobe)
    assert c == VR.frangi_c(h6, lobe) and c < VR.frangi_c(h6)
    lobe[:] = 0
    lobe[-1] = 7
    assert gpu_norm_max(h6, lobe) == VR.frangi_c(h6)
    assert gpu_norm_max(h6, np.zeros(S, dtype=np.uint8)) == np.float32(1.0)
    assert gpu_norm_max(np.zeros_like(h6), None) == np.float32(1.0)


@pytest.mark.parametrize("variant", ["no_lobe", "lobe_holds_the_maximum", "lobe_leaves_it_out"])
def test_norm_max_past_the_grid_cap(variant):
    """4096 x 256 + 300 voxels: the grid-stride loop takes a second, ragged lap.  The largest norm lies in that lap; a lobe map
    that leaves it out makes the answer the first lap's largest (tests/vessel_cases.py: norm_max_large)."""
    h6, lobes = VC.norm_max_large()
    lobe = lobes[variant]
    norms = VR.frobenius32(h6)
    at = VC.NORM_MAX_FIRST_LAP if variant == "lobe_leaves_it_out" else VC.NORM_MAX_SECOND_LAP
    c = gpu_norm_max(h6, lobe)
    assert c == VR.frangi_c(h6, lobe) == np.float32(0.5) * norms[at]


@functools.lru_cache(maxsize=None)
def _e2e_device():
    from dram_amd.vessels import vesselness
    scan, lobe = VC.e2e_volume()
    return vesselness(_dev(scan), VC.E2E_SPACING, VC.E2E_SIGMAS, lobe=_dev(lobe)).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _e2e_reference():
    _, lobe = VC.e2e_volume()
    return VC.e2e_vesselness(None, lobe)


def test_vesselness_end_to_end():
    """4. vesselness (c = None over the lobes) on the 40 x 48 x 56 anisotropic volume against the restatement on the lobe
    voxels, within VC.E2E_TOLERANCE.  That tolerance is set by the few voxels where Frangi's V jumps (see the cases file), so
    the call is also compared bit for bit with the C ABI entries composed by hand, which tests 1 - 3 hold tightly."""
    from dram_amd import vessels
    from dram_amd._lib import call, lib
    scan, lobe = VC.e2e_volume()
    got, ref = _e2e_device(), _e2e_reference()
    inside = lobe > 0
    err = np.abs(got.astype(np.float64) - ref)[inside]
    print(f"end to end: max error {err.max():.3e}, 99.9th percentile {np.percentile(err, 99.9):.3e}, median {np.median(err):.3e}, "
          f"tolerance {VC.E2E_TOLERANCE:.3e}")
    assert got.dtype == np.float32 and err.max() <= VC.E2E_TOLERANCE
    assert got[14, 21, 15] > 0.5 and got[30, 35, 20] < 1e-3 + VC.E2E_TOLERANCE
    # the same call composed from the entry points, whole volume
    D, H, W = scan.shape
    S = D * H * W
    x, lb = _dev(scan), _dev(lobe)
    h6 = torch.empty((6, D, H, W), dtype=torch.float32, device="cuda")
    ws = torch.empty(lib.dram_hessian_ws_bytes(D, H, W) // 4, dtype=torch.float32, device="cuda")
    vmax = torch.empty((D, H, W), dtype=torch.float32, device="cuda")
    c_dev = torch.empty(1, dtype=torch.float32, device="cuda")
    for k, s in enumerate(VC.E2E_SIGMAS):
        vessels._hessian_into(x, vessels._scale_tables(list(VC.E2E_SPACING), s, "test"), VC.E2E_CLIP, h6, ws)
        call("dram_hessian_norm_max", h6.data_ptr(), lb.data_ptr(), S, c_dev.data_ptr(), _st())
        c_ref = VR.frangi_c(VC.e2e_hessians()[k].astype(np.float32), lobe)
        # the norm moves by at most the Frobenius norm of the change of H: 3 max(bound); c is half of it
        assert abs(float(c_dev.item()) - float(c_ref)) <= 1.5 * VC.e2e_bound(s).max() + 1e-6 * float(c_ref)
        call("dram_vesselness", h6.data_ptr(), S, 0.5, 0.5, c_dev.data_ptr(), vmax.data_ptr(), int(k > 0), None, _st())
    by_hand = vmax.cpu().numpy()
    assert np.array_equal(by_hand[inside].view(np.uint32), got[inside].view(np.uint32))


def test_mask_equals_the_reference_away_from_the_threshold():
    """5. (vmax >= threshold) & (lobe > 0) equals the restatement's mask except where the reference V lies within the end-to-end
    tolerance of the threshold -- at most 1 % of the lobe voxels (checked for the reference alone on the CPU)."""
    from dram_amd.vessels import pseudo_vessel_mask, vessel_mask
    scan, lobe = VC.e2e_volume()
    ref = _e2e_reference()
    mask = pseudo_vessel_mask(_dev(scan), _dev(lobe), VC.E2E_SPACING, threshold=VC.MASK_THRESHOLD, sigmas_mm=VC.E2E_SIGMAS)
    assert mask.dtype == torch.uint8 and mask.is_cuda
    mask = mask.cpu().numpy()
    near = np.abs(ref - VC.MASK_THRESHOLD) <= VC.E2E_TOLERANCE
    inside = lobe > 0
    assert (near & inside).sum() <= 0.01 * inside.sum()
    want = VR.mask(ref, lobe, VC.MASK_THRESHOLD)
    assert np.array_equal(mask[~near], want[~near]) and set(np.unique(mask)) == {0, 1} and not mask[~inside].any()
    # the entry itself: >= (not >), the lobe gate, no lobe
    v = np.array([0.25, 0.5, np.nextafter(np.float32(0.5), np.float32(0)), 0.75, 0.5] * 120, dtype=np.float32).reshape(2, 3, 100)
    lb = np.ones(v.shape, dtype=np.uint8)
    lb[..., -1] = 0
    assert np.array_equal(vessel_mask(_dev(v), _dev(lb), 0.5).cpu().numpy(), ((v >= np.float32(0.5)) & (lb > 0)).astype(np.uint8))
    assert np.array_equal(vessel_mask(_dev(v), None, 0.5).cpu().numpy(), (v >= np.float32(0.5)).astype(np.uint8))


@pytest.mark.parametrize("c", [None, VC.E2E_C_GIVEN])
def test_bounding_box_equals_the_whole_volume_bit_for_bit(c):
    """6. vesselness(..., lobe=lobe) computes only the grown bounding box of the lobes: on lobe > 0 it equals the whole-volume
    call bit for bit, outside the box it is 0.  The box touches the z = 0, y = 0 and x = 0 faces and stays clear of the opposite
    ones by more than the radius.  With c = None the whole-volume side is composed from the entry points, so that both take
    Frangi's maximum over the same (lobe) voxels."""
    from dram_amd import vessels
    from dram_amd._lib import call, lib
    scan, _ = VC.e2e_volume()
    lobe = VC.bbox_lobe()
    x, lb = _dev(scan), _dev(lobe)
    boxed = vessels.vesselness(x, VC.E2E_SPACING, VC.E2E_SIGMAS, c=c, lobe=lb).cpu().numpy()
    if c is not None:
        whole = vessels.vesselness(x, VC.E2E_SPACING, VC.E2E_SIGMAS, c=c).cpu().numpy()
    else:
        D, H, W = scan.shape
        S = D * H * W
        h6 = torch.empty((6, D, H, W), dtype=torch.float32, device="cuda")
        ws = torch.empty(lib.dram_hessian_ws_bytes(D, H, W) // 4, dtype=torch.float32, device="cuda")
        vmax = torch.empty((D, H, W), dtype=torch.float32, device="cuda")
        c_dev = torch.empty(1, dtype=torch.float32, device="cuda")
        for k, s in enumerate(VC.E2E_SIGMAS):
            vessels._hessian_into(x, vessels._scale_tables(list(VC.E2E_SPACING), s, "test"), VC.E2E_CLIP, h6, ws)
            call("dram_hessian_norm_max", h6.data_ptr(), lb.data_ptr(), S, c_dev.data_ptr(), _st())
            call("dram_vesselness", h6.data_ptr(), S, 0.5, 0.5, c_dev.data_ptr(), vmax.data_ptr(), int(k > 0), None, _st())
        whole = vmax.cpu().numpy()
    inside = lobe > 0
    assert np.array_equal(boxed[inside].view(np.uint32), whole[inside].view(np.uint32)) and (whole[inside] > 0).any()
    # the box: lobe box 0:14, 0:12, 0:21 grown by the radii (12, 17, 17) at 3 mm, x widened to a multiple of 4
    outside = np.ones(scan.shape, dtype=bool)
    outside[0:26, 0:29, 0:40] = False
    assert not boxed[outside].any() and whole[outside].any()
    # no lobe voxel at all: zeros
    assert not vessels.vesselness(x, VC.E2E_SPACING, VC.E2E_SIGMAS, c=c, lobe=torch.zeros_like(lb)).any()


def test_two_runs_give_the_same_bits():
    """8. Determinism: the volume, its Hessian and the mask, twice."""
    from dram_amd.vessels import hessian, pseudo_vessel_mask, vesselness
    scan, lobe = VC.e2e_volume()
    x, lb = _dev(scan), _dev(lobe)
    first = _e2e_device()
    again = vesselness(x, VC.E2E_SPACING, VC.E2E_SIGMAS, lobe=lb).cpu().numpy()
    assert np.array_equal(first.view(np.uint32), again.view(np.uint32))
    h1, h2 = hessian(x, VC.E2E_SPACING, 2.0), hessian(x, VC.E2E_SPACING, 2.0)
    assert h1.shape == (6,) + scan.shape and torch.equal(h1.view(torch.int32), h2.view(torch.int32))
    m1, m2 = (pseudo_vessel_mask(x, lb, VC.E2E_SPACING, threshold=0.3) for _ in range(2))
    assert torch.equal(m1, m2) and m1.any()
    # the Python layer's Hessian is the entry's: float32 input of the same values, host arrays, clip None
    h3 = hessian(np.asarray(scan, dtype=np.float32), VC.E2E_SPACING, 2.0)
    assert torch.equal(h1.view(torch.int32), h3.view(torch.int32))


def _model():
    """The slim model of tests/test_gpu_inference.py (a copy of its helper)."""
    import models
    from dram_amd.configs import SLIM
    torch.manual_seed(3)
    m = models.DC3D(**SLIM, norm_method="bn")
    m.init(models.HeNorm(mode="fan_in"))
    g = torch.Generator().manual_seed(4)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm3d):
            mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g) * 0.1)
            mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) + 0.5)
    return m


def test_lobe_inference_takes_a_callable_vessel():
    """9. run(..., vessel=partial(pseudo_vessel_mask, ...)) returns key by key and bit for bit what run(..., vessel=<that mask>)
    returns; None and an array behave as before."""
    from dram_amd.inference import LobeInference, synthetic_ct
    from dram_amd.vessels import pseudo_vessel_mask
    scan, lobe, spacing = synthetic_ct((41, 57, 66), (2.5, 1.0, 1.0), seed=7, n_lesions=8)
    fn = functools.partial(pseudo_vessel_mask, threshold=0.05, sigmas_mm=(1.0, 2.0))
    calls = []

    def counted(s, l, sp):
        calls.append((s.is_cuda and s.dtype == torch.int16, l.is_cuda and l.dtype == torch.uint8, tuple(sp)))
        return fn(s, l, sp)

    inf = LobeInference(_model().cuda().eval(), resample_size=24)
    mask = fn(_dev(scan), _dev(lobe), spacing)
    assert mask.any() and not mask.all()
    by_call = inf.run(scan, lobe, spacing, vessel=counted)
    by_mask = inf.run(scan, lobe, spacing, vessel=mask)
    by_host = inf.run(scan, lobe, spacing, vessel=mask.cpu().numpy())
    plain = inf.run(scan, lobe, spacing)
    assert calls == [(True, True, tuple(spacing))]
    assert set(by_call) == set(by_mask) == set(by_host) and "mask_post" in by_call and "mask_post" not in plain

    def same(a, b):
        if torch.is_tensor(a):
            return torch.equal(a, b)
        if isinstance(a, float):
            return a == b or (a != a and b != b)
        return a == b
    for key in by_call:
        assert same(by_call[key], by_mask[key]) and same(by_call[key], by_host[key]), key
    for key in plain:
        assert same(plain[key], by_call[key]), key
    no_vessel = inf.post_process(_dev(scan), _dev(lobe), plain["htp"], plain["threshold"], vessel=torch.zeros_like(mask))["mask_post"]
    assert torch.equal(by_call["mask_post"], no_vessel * (mask == 0).to(torch.uint8))
