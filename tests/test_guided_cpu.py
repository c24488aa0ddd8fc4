"""The fp64 restatement of the masked guided filter (tests/guided_restatement.py) against a second route and analytic anchors,
and everything of dram_amd/refine.py and the C ABI that answers without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import guided_cases as GC
import guided_restatement as GR


def second_route(guide, p, mask, radius, eps, window):
    """The same filter through scipy.ndimage.uniform_filter(mode="constant") * window size, the region applied as products
    (legal here: the inputs are finite)."""
    from scipy.ndimage import uniform_filter
    size = [2 * r + 1 for r in radius]
    box = lambda v: uniform_filter(v, size=size, mode="constant", cval=0.0) * float(np.prod(size))
    m = (np.asarray(mask) != 0).astype(np.float64)
    g = GR.guide_values(guide, window) * m
    pp = np.asarray(p, dtype=np.float64) * m
    n = np.maximum(np.rint(box(m)), 1.0)
    mg, mp = box(g) / n, box(pp) / n
    a = (box(g * pp) / n - mg * mp) / ((box(g * g) / n - mg * mg) + eps) * m
    b = (mp - a * mg) * m
    return (box(a) / n * g + box(b) / n) * m, a, b


@pytest.mark.parametrize("name", ["faces", "ragged_i16", "ragged_f32", "radius0", "short_z"])
def test_restatement_against_uniform_filter(name):
    """A full mask and ragged ones.  uniform_filter sums in another order (and as running sums), so the two differ by fp64
    rounding: well inside 1e-4 of the any-order bound's 1 / eps amplification, asked here as 1e-9."""
    guide, p, mask = GC.inputs(name)
    ref = GC.expected(name)
    q, a, b = second_route(guide, p, mask, GC.CASES[name][1], GC.EPS, GC.window_of(name))
    for key, other in (("q64", q), ("a", a), ("b", b)):
        err = np.abs(ref[key] - other).max()
        print(f"{name} {key}: restatement against uniform_filter {err:.3e}")
        assert err <= 1e-9
    assert np.abs(ref["q64"]).max() > 0.1 and (mask != 0).any()


def _small(seed=3, shape=(7, 8, 9)):
    rng = np.random.default_rng(seed)
    g = rng.random(size=shape).astype(np.float32)
    p = rng.random(size=shape).astype(np.float32)
    m = (rng.integers(0, 4, size=shape) > 0).astype(np.uint8)
    return g, p, m


def test_anchor_radius_zero_returns_p():
    g, p, m = _small()
    ref = GR.guided_filter(g, p, m, (0, 0, 0), 1e-3)
    assert np.array_equal(ref["q"][m != 0], p[m != 0]) and not ref["q"][m == 0].any()
    assert not ref["a"].any()                                    # var and cov are exactly 0


def test_anchor_constant_p():
    g, _, m = _small()
    c = np.float32(0.7315)
    ref = GR.guided_filter(g, np.full(g.shape, c, dtype=np.float32), m, (1, 2, 2), 1e-3)
    inside = m != 0
    assert np.abs(ref["q"][inside].astype(np.float64) - float(c)).max() <= np.spacing(c)
    assert not ref["q"][~inside].any()


def test_anchor_empty_and_outside():
    g, p, m = _small()
    ref = GR.guided_filter(g, p, np.zeros_like(m), (1, 1, 1), 1e-3)
    assert not ref["q"].any() and not ref["a"].any() and not ref["b"].any()
    # nothing outside the region counts: NaN and 1e30 there change no bit
    base = GR.guided_filter(g, p, m, (1, 2, 1), 1e-3)
    for bad in (np.nan, 1e30):
        g2, p2 = g.copy(), p.copy()
        g2[m == 0] = bad
        p2[m == 0] = bad
        other = GR.guided_filter(g2, p2, m, (1, 2, 1), 1e-3)
        assert all(np.array_equal(base[k], other[k]) for k in base)


def test_anchor_linear_relation_is_kept():
    """p = 2 g + 0.25 on a full mask with eps -> 0: a -> 2, b -> 0.25, q -> p (the filter's defining property)."""
    rng = np.random.default_rng(5)
    g = rng.random(size=(6, 7, 8)).astype(np.float32)
    p = (2.0 * g.astype(np.float64) + 0.25).astype(np.float32)
    ref = GR.guided_filter(g, p, np.ones(g.shape, np.uint8), (1, 1, 1), 1e-12)
    assert np.abs(ref["a"] - 2.0).max() < 1e-5 and np.abs(ref["q64"] - p).max() < 1e-5


def test_fp64_term_is_below_one_fp32_ulp():
    """The any-order worst-case bound (not an estimate of the error) stays more than a factor of ten below one fp32 ulp at 1
    in every case, the radius cap included: the fp32 rounding of q is what the tolerance is made of."""
    for name, (_, radius, _, _) in GC.CASES.items():
        guide, p, mask = GC.inputs(name)
        t = GC.fp64_terms(radius, GC.EPS, *GC.magnitudes(guide, p, mask, GC.window_of(name)))
        assert t["q"] < 0.1 * 2.0 ** -23, (name, t)


def test_abi_answers_without_a_gpu():
    from dram_amd._lib import lib
    cap = lib.dram_guided_max_radius()
    assert cap == GC.MAX_RADIUS and cap >= 8
    assert lib.dram_guided_ws_bytes(3, 4, 5) == 12 * 60 * 8
    assert lib.dram_guided_ws_bytes(0, 4, 5) == 0 and lib.dram_guided_ws_bytes(2048, 1024, 1024) == 0
    # the refusals of the C call come before any launch: dummy aligned pointers do
    q = 64
    r = lambda *v: (ctypes.c_int * 3)(*v)
    ws = lib.dram_guided_ws_bytes(3, 4, 5)
    ok = dict(guide=q, kind=0, lo=-1150.0, hi=350.0, p=q, mask=q, radius=r(1, 1, 1), eps=1e-3, q=q, ab=None, ws=q, ws_bytes=ws)
    for change in (dict(eps=0.0), dict(eps=-1.0), dict(eps=float("inf")), dict(eps=float("nan")), dict(radius=r(-1, 1, 1)),
                   dict(radius=r(1, cap + 1, 1)), dict(hi=-1150.0), dict(hi=-2000.0), dict(ws_bytes=ws - 1), dict(kind=2),
                   dict(ws=q + 8), dict(p=None)):
        a = {**ok, **change}
        rc = lib.dram_guided_filter(a["guide"], a["kind"], a["lo"], a["hi"], a["p"], a["mask"], a["radius"], a["eps"], 3, 4, 5, a["q"],
                                    a["ab"], a["ws"], a["ws_bytes"], None)
        assert rc != 0, change


def test_wrapper_refusals():
    from dram_amd import guided_filter, refine_heatmap
    from dram_amd._lib import lib
    cap = lib.dram_guided_max_radius()
    shape = (3, 4, 5)
    p, gf, gi, m = torch.zeros(shape), torch.zeros(shape), torch.zeros(shape, dtype=torch.int16), torch.ones(shape, dtype=torch.uint8)
    bad = [
        dict(radius=(1, 1)), dict(radius=(1, 1, -1)), dict(radius=(1, cap + 1, 1)), dict(radius=(1.0, 1, 1)), dict(radius=3),
        dict(eps=0.0), dict(eps=-1e-3), dict(eps=float("inf")), dict(eps=float("nan")),
        dict(guide=gi), dict(guide=gi, window=(350, -1150)), dict(guide=gi, window=(0.0, 0.0)), dict(guide=gi, window=(0.0, float("inf"))),
        dict(window=(0.0, 1.0)), dict(guide=gf.double()), dict(p=p.double()), dict(mask=m.float()),
        dict(mask=torch.ones((3, 4, 6), dtype=torch.uint8)), dict(p=torch.zeros((4, 5))), dict(p=torch.zeros((0, 4, 5)), guide=torch.zeros((0, 4, 5)),
                                                                                              mask=torch.zeros((0, 4, 5), dtype=torch.uint8)),
    ]
    for change in bad:
        a = {**dict(p=p, guide=gf, mask=m, radius=(1, 1, 1), eps=1e-3, window=None), **change}
        with pytest.raises(ValueError):
            guided_filter(a["p"], a["guide"], a["mask"], a["radius"], a["eps"], a["window"])
    with pytest.raises(ValueError, match="GPU"):                 # valid arguments, tensors on the host
        guided_filter(p, gf, m, (1, 1, 1), 1e-3)
    for kw in (dict(radius_mm=0.0), dict(radius_mm=float("nan")), dict(radius_mm=(cap + 1) * 0.5), dict(eps=0.0), dict(iterations=0),
               dict(iterations=1.5), dict(window=None), dict(window=(1, 1))):
        with pytest.raises(ValueError):
            refine_heatmap(p, gi, m, (1.0, 0.5, 0.5), **kw)
    with pytest.raises(ValueError):
        refine_heatmap(p, gi, m, (1.0, 0.0, 0.5))
    with pytest.raises(ValueError, match="GPU"):
        refine_heatmap(p, gi, m, (1.0, 0.5, 0.5))


def test_radius_mm_maps_to_voxels():
    from dram_amd.refine import radius_voxels
    assert radius_voxels(3.0, (1.0, 0.7, 0.7)) == [3, 4, 4]
    assert radius_voxels(3.0, (5.0, 2.5, 0.75)) == [1, 1, 4]     # never below 1; 1.2 -> 1
    assert radius_voxels(4.0, (0.5, 0.5, 0.5)) == [8, 8, 8]      # 4 mm at 0.5 mm spacing is served
    assert radius_voxels(2.5, (1.0, 1.0, 1.0)) == [2, 2, 2]      # Python's round: halves to the even neighbour


def test_inference_refine_argument():
    from dram_amd.inference import LobeInference
    assert LobeInference(None).refine is None and LobeInference(None, refine=True).refine == {}
    assert LobeInference(None, refine=dict(radius_mm=2.0, iterations=2)).refine == dict(radius_mm=2.0, iterations=2)
    for bad in (False, 3, dict(radius=2), "yes"):
        with pytest.raises(ValueError, match="refine"):
            LobeInference(None, refine=bad)
