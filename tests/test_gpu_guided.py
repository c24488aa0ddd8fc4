"""csrc/guided.hip through the C ABI and dram_amd/refine.py on the device against the fp64 restatement
(tests/guided_restatement.py, itself held against scipy and analytic anchors by tests/test_guided_cpu.py).  Inputs, tile
constants and the written-out tolerance: tests/guided_cases.py.  Before every call q, ab and the workspace are NaN."""
import ctypes

import numpy as np
import pytest
import torch

import guided_cases as GC
import guided_restatement as GR

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()       # a copy: the shared cases are read-only arrays


def gpu_filter(guide, p, mask, radius, eps=GC.EPS, window=None, want_ab=True):
    from dram_amd._lib import call, lib
    D, H, W = p.shape
    g, pp, m = _dev(guide), _dev(p), _dev(mask)
    q = torch.full((D, H, W), NAN, dtype=torch.float32, device="cuda")
    ab = torch.full((2, D, H, W), NAN, dtype=torch.float64, device="cuda") if want_ab else None
    ws_bytes = lib.dram_guided_ws_bytes(D, H, W)
    ws = torch.full((ws_bytes // 8,), NAN, dtype=torch.float64, device="cuda")
    lo, hi = window if window is not None else (0.0, 0.0)
    call("dram_guided_filter", g.data_ptr(), 0 if guide.dtype == np.int16 else 1, lo, hi, pp.data_ptr(), m.data_ptr(),
         (ctypes.c_int * 3)(*radius), eps, D, H, W, q.data_ptr(), ab.data_ptr() if want_ab else None, ws.data_ptr(), ws_bytes,
         torch.cuda.current_stream().cuda_stream)
    return q.cpu().numpy(), (ab.cpu().numpy() if want_ab else None)


def _case(name):
    guide, p, mask = GC.inputs(name)
    return guide, p, mask, GC.CASES[name][1], GC.window_of(name)


@pytest.mark.parametrize("name", list(GC.CASES))
def test_parity_within_the_bound(name):
    """1. q and ab against the restatement within 2^-24 |ref| + the fp64 term (GC.fp64_terms), both guide kinds, isotropic and
    anisotropic radii, the shapes of GC.CASES."""
    guide, p, mask, radius, window = _case(name)
    q, ab = gpu_filter(guide, p, mask, radius, window=window)
    ref = GC.expected(name)
    terms = GC.fp64_terms(radius, GC.EPS, *GC.magnitudes(guide, p, mask, window))
    assert q.dtype == np.float32 and np.isfinite(q).all() and np.isfinite(ab).all()
    ratios = GC.check(name, q, ab, ref, terms)
    assert max(ratios) <= 1.0, (name, ratios)
    assert not q[mask == 0].any() and not ab[:, mask == 0].any()
    assert (mask != 0).sum() > 1 and np.abs(ref["q64"]).max() > 0.1


def test_anchor_radius_zero_is_the_identity():
    guide, p, mask, _, window = _case("ragged_i16")
    q, ab = gpu_filter(guide, p, mask, (0, 0, 0), window=window)
    inside = mask != 0
    assert np.array_equal(q[inside].view(np.uint32), p[inside].view(np.uint32)) and not q[~inside].any()
    assert not ab[0].any()                                       # var and cov are exactly 0 in fp64


def test_anchor_constant_p():
    guide, _, mask, radius, window = _case("ragged_f32")
    c = np.float32(0.7315)
    q, _ = gpu_filter(guide, np.full(guide.shape, c, dtype=np.float32), mask, radius, window=window)
    inside = mask != 0
    err = np.abs(q[inside].astype(np.float64) - float(c)).max()
    print(f"constant p: max |q - c| {err:.3e}, one ulp {np.spacing(c):.3e}")
    assert err <= np.spacing(c) and not q[~inside].any()


def test_anchor_empty_mask_gives_zeros():
    guide, p, mask, radius, window = _case("ragged_i16")
    q, ab = gpu_filter(guide, p, np.zeros_like(mask), radius, window=window)
    assert not q.any() and not ab.any()


@pytest.mark.parametrize("kind", ["i16", "f32"])
def test_outside_the_region_nothing_counts(kind):
    """3. NaN and 1e30 in G and P wherever M == 0: the same bits as with zeros there."""
    guide, p, mask, radius, window = _case("ragged_" + kind)
    outside = mask == 0
    g0, p0 = guide.copy(), p.copy()
    g0[outside] = 0
    p0[outside] = 0
    base_q, base_ab = gpu_filter(g0, p0, mask, radius, window=window)
    for bad in (np.nan, 1e30):
        g1, p1 = guide.copy(), p.copy()
        p1[outside] = bad
        g1[outside] = bad if kind == "f32" else (-32768 if np.isnan(bad) else 32767)
        q, ab = gpu_filter(g1, p1, mask, radius, window=window)
        assert np.array_equal(q.view(np.uint32), base_q.view(np.uint32))
        assert np.array_equal(ab.view(np.uint64), base_ab.view(np.uint64))


def test_determinism_and_null_ab():
    guide, p, mask, radius, window = _case("w_mod4")
    q1, ab1 = gpu_filter(guide, p, mask, radius, window=window)
    q2, ab2 = gpu_filter(guide, p, mask, radius, window=window)
    q3, none = gpu_filter(guide, p, mask, radius, window=window, want_ab=False)
    assert none is None
    assert np.array_equal(q1.view(np.uint32), q2.view(np.uint32)) and np.array_equal(ab1.view(np.uint64), ab2.view(np.uint64))
    assert np.array_equal(q1.view(np.uint32), q3.view(np.uint32))


def _lobe_scene():
    """A 24 x 30 x 45 scan with two lobes whose bounding box starts at x = 5 (odd) and ends short of every face."""
    rng = np.random.default_rng(77)
    shape = (24, 30, 45)
    scan = np.rint(rng.uniform(-1300.0, 500.0, size=shape)).astype(np.int16)
    htp = rng.random(size=shape).astype(np.float32)
    z, y, x = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij", sparse=True)
    lobe = np.zeros(shape, dtype=np.uint8)
    lobe[(((z - 11) / 8.0) ** 2 + ((y - 14) / 10.0) ** 2 + ((x - 13) / 8.5) ** 2) < 1.0] = 1
    lobe[(((z - 12) / 7.0) ** 2 + ((y - 15) / 9.0) ** 2 + ((x - 31) / 8.0) ** 2) < 1.0] = 4
    xs = np.nonzero(lobe.any(axis=(0, 1)))[0]
    assert xs[0] == 5 and xs[-1] < shape[2] - 1
    return scan, htp, lobe


def test_refine_heatmap_on_the_lobe_box_is_the_whole_volume_call():
    """5. Bit for bit, with a box that starts at odd x; iterations=2 is two calls; the wrapper against the restatement."""
    from dram_amd import guided_filter, refine_heatmap
    scan, htp, lobe = _lobe_scene()
    spacing = (1.5, 1.0, 0.75)
    radius = (2, 3, 4)                                            # round(3 / 1.5), round(3 / 1), round(3 / 0.75)
    s, h, l = _dev(scan), _dev(htp), _dev(lobe)
    whole, ab = guided_filter(h, s, l, radius, 1e-3, window=(-1150, 350), return_ab=True)
    boxed = refine_heatmap(h, s, l, spacing)
    assert boxed.dtype == torch.float32 and boxed.shape == h.shape
    assert torch.equal(whole.view(torch.int32), boxed.view(torch.int32))
    assert not bool(boxed[l == 0].any()) and ab.dtype == torch.float64 and tuple(ab.shape) == (2, *scan.shape)
    ref = GR.guided_filter(scan, htp, lobe, radius, 1e-3, (-1150.0, 350.0))
    terms = GC.fp64_terms(radius, 1e-3, *GC.magnitudes(scan, htp, lobe, (-1150.0, 350.0)))
    assert max(GC.check("wrapper", whole.cpu().numpy(), ab.cpu().numpy(), ref, terms)) <= 1.0
    twice = refine_heatmap(h, s, l, spacing, iterations=2)
    again = guided_filter(whole, s, l, radius, 1e-3, window=(-1150, 350))
    assert torch.equal(twice.view(torch.int32), again.view(torch.int32)) and not torch.equal(twice, whole)
    # a float32 guide and a bool mask go the same way
    gf = torch.from_numpy(GR.guide_values(scan, (-1150.0, 350.0)).astype(np.float32)).cuda()
    a = guided_filter(h, gf, l > 0, radius, 1e-3)
    b = refine_heatmap(h, gf, l, spacing, window=None)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # no lobe voxel: zeros
    assert not bool(refine_heatmap(h, s, torch.zeros_like(l), spacing).any())


def test_wrapper_refusals_on_the_device():
    from dram_amd import guided_filter, refine_heatmap
    scan, htp, lobe = _lobe_scene()
    s, h, l = _dev(scan), _dev(htp), _dev(lobe)
    with pytest.raises(ValueError):
        guided_filter(h, s, l, (1, 1, 17), 1e-3, window=(-1150, 350))
    with pytest.raises(ValueError):
        guided_filter(h, s, l, (1, 1, 1), 0.0, window=(-1150, 350))
    with pytest.raises(ValueError):
        guided_filter(h, s, l, (1, 1, 1), 1e-3, window=(350, 350))
    with pytest.raises(ValueError):
        guided_filter(h, s.cpu(), l, (1, 1, 1), 1e-3, window=(-1150, 350))
    with pytest.raises(ValueError):
        refine_heatmap(h, s, l, (0.1, 1.0, 1.0))                  # 3 mm at 0.1 mm: 30 voxels
