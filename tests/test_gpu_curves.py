"""csrc/curves.hip and dram_amd/curves.py on the device against the numpy restatement (tests/curves_restatement.py, itself held
against sklearn.metrics and inference.dice / iou by tests/test_curves_cpu.py): the tables are integers, so they are compared
exactly; the curves are the same host arithmetic on equal tables."""
import numpy as np
import pytest
import torch

import curves_cases as CC
import curves_restatement as CR

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
    keep = []
    ptr = []
    for key, off in zip(("score", "ref", "region", "gate"), c["offsets"]):
        if c[key] is None:
            ptr.append(None)
        else:
            holder, p = _placed(c[key], off)
            keep.append(holder)
            ptr.append(p)
    shape = (c["nregions"], 2, c["nbins"] + 1)
    hist = torch.full(shape, -7, dtype=torch.int64, device="cuda")                             # poisoned: the entry initialises
    conf = torch.full(shape, -7, dtype=torch.int64, device="cuda") if c["conf"] else None
    call("dram_score_hist", *ptr, c["nregions"], c["nbins"], hist.data_ptr(), None if conf is None else conf.data_ptr(),
         c["score"].size, _st())
    out = hist.cpu().numpy(), None if conf is None else conf.cpu().numpy()
    del keep
    return out


@pytest.mark.parametrize("name", CC.names())
def test_score_hist_matches_the_restatement(name):
    c = CC.case(name)
    ref = CC.expected(name)
    got = gpu_tables(c)
    for key, g, r in zip(("hist", "conf"), got, ref):
        assert (g is None) == (r is None), key
        if g is not None:
            assert g.dtype == r.dtype and g.shape == r.shape, key
            bad = np.argwhere(g != r)
            assert bad.size == 0, (key, len(bad), bad[:4].tolist(), g[tuple(bad[0])], r[tuple(bad[0])])
    again = gpu_tables(c)                                                                      # no dependence on the order of the atomics
    assert np.array_equal(again[0], got[0]) and (got[1] is None or np.array_equal(again[1], got[1]))
    if name in CC.REGIMES:
        assert CC.regime(name) == CC.REGIMES[name]


def test_every_path_is_exercised_with_and_without_conf():
    seen = {(CC.regime(name), CC.case(name)["conf"]) for name in CC.names()}
    assert seen == {(0, False), (0, True), (1, False), (1, True)}
    assert {CC.case(name)["nbins"] for name in CC.names()} >= {2, 256, 1024, 4096}


def test_heatmap_curves_end_to_end():
    from dram_amd import curves_from_tables, heatmap_curves, score_tables
    c = CC.case("multi_lap_big")
    assert c["gate"] is not None and c["nregions"] == 5
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    got = heatmap_curves(dev(c["score"]), dev(c["ref"]), dev(c["region"]), 5, dev(c["gate"]), nbins=1024, n_cal=16)
    ref = CR.heatmap_curves(c["score"], c["ref"], c["region"], 5, c["gate"], 1024, 16)
    CC.assert_curves_equal(got, ref)
    assert 0.5 < got["auc_roc"][-1] < 1.0 and 0.0 <= got["ece"][-1] <= 1.0
    # host arrays go in as they are; a 3-D shape; no conf; other bins
    shape = (3, 1, -1)
    t = score_tables(np.array(c["score"]).reshape(shape), np.array(c["ref"]).reshape(shape), np.array(c["region"]).reshape(shape), 5,
                     None, nbins=256, conf=False)
    h, _ = CR.tables(c["score"], c["ref"], c["region"], 5, None, 256, False)
    assert t["conf"] is None and t["hist"].dtype == np.int64 and np.array_equal(t["hist"], h)
    CC.assert_curves_equal(curves_from_tables(t["hist"]), CR.curves(h))
    one = score_tables(dev(c["score"]), dev(c["ref"]), nbins=4096)                             # no region map: one region
    h1, c1 = CR.tables(c["score"], c["ref"], None, 1, None, 4096)
    assert np.array_equal(one["hist"], h1) and np.array_equal(one["conf"], c1)
    sc, rf = np.array(c["score"]), np.array(c["ref"])
    with pytest.raises(ValueError, match="float32"):
        score_tables(sc.astype(np.float64), rf)
    with pytest.raises(ValueError, match="power of two"):
        score_tables(sc, rf, nbins=1000)
    with pytest.raises(ValueError, match="one region"):
        score_tables(sc, rf, n_regions=2)
    with pytest.raises(ValueError, match="same shape"):
        score_tables(sc, rf[:-1])
    with pytest.raises(ValueError, match="uint8"):
        score_tables(sc, rf, np.array(c["region"], dtype=np.int32), 5)


def test_score_hist_error_paths_launch_nothing():
    from dram_amd._lib import DramHipError, call, lib
    c = CC.case("size_4097")
    score, ref = torch.from_numpy(np.array(c["score"])).cuda(), torch.from_numpy(np.array(c["ref"])).cuda()
    out = torch.full((2, 2, 257), -7, dtype=torch.int64, device="cuda")
    args = lambda nregions, nbins, region=None: (score.data_ptr(), ref.data_ptr(), region, None, nregions, nbins, out[0].data_ptr(),
                                                 out[1].data_ptr(), 4097, _st())
    assert lib.dram_score_hist(*args(1, 100)) == -1 and lib.dram_score_hist(*args(0, 256, ref.data_ptr())) == -1
    with pytest.raises(DramHipError, match="one region"):
        call("dram_score_hist", *args(2, 256))
    torch.cuda.synchronize()
    assert bool((out == -7).all())


def _model():
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


def _same_value(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(_same_value(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b


@pytest.mark.parametrize("original", [False, True])
def test_lobe_inference_curves(original):
    from dram_amd._lib import call
    from dram_amd.inference import LobeInference, resample_volume, synthetic_ct
    scan, lobe, spacing = synthetic_ct((48, 64, 64), (1.0, 0.7, 0.7), seed=7, n_lesions=6)
    rng = np.random.default_rng(3)
    vessel = ((rng.random(scan.shape) > 0.9) & (lobe > 0)).astype(np.uint8)
    lesion = ((scan > -600) & (lobe > 0)).astype(np.uint8)
    kw = dict(original_spacing=(1.5, 0.9, 0.6), original_size=(32, 50, 75)) if original else {}
    inf = LobeInference(_model().cuda().eval(), resample_size=24)
    plain = inf.run(scan, lobe, spacing, vessel=vessel, lesion=lesion, **kw)
    res = inf.run(scan, lobe, spacing, vessel=vessel, lesion=lesion, curves=256, **kw)
    assert sorted(res) == sorted(list(plain) + ["curves", "curves_post"])
    for key in plain:                                                                          # curves=None: what it returns today
        assert _same_value(plain[key], res[key]), key
    assert sorted(inf.run(scan, lobe, spacing, vessel=vessel, lesion=lesion, curves=None, **kw)) == sorted(plain)

    scan_d, lobe_d, vessel_d = (torch.from_numpy(a).cuda() for a in (scan, lobe, vessel))
    gate = torch.empty(scan.shape, dtype=torch.uint8, device="cuda")
    call("dram_lesion_post", res["htp"].data_ptr(), scan_d.data_ptr(), vessel_d.data_ptr(), None, gate.data_ptr(), float("-inf"),
         -1150, 350, float(res["threshold_scan"]), scan_d.numel(), _st())
    assert 0 < int(((gate > 0) & (lobe_d > 0)).sum()) < int((lobe_d > 0).sum())    # the gate is on for some lung voxels, not all
    if original:
        back = lambda v: resample_volume(v, spacing, kw["original_spacing"], kw["original_size"], "nearest")
        score, ref, regions, gate = res["original"]["htp"], res["original"]["lesion"], back(lobe_d), back(gate)
    else:
        score, ref, regions = res["htp"], torch.from_numpy(lesion), lobe_d
    host = lambda t: t.cpu().numpy()
    n_regions = int(lobe.max())
    assert n_regions == 5
    ref_plain = CR.heatmap_curves(host(score), host(ref), host(regions), n_regions, None, 256, 16)
    ref_post = CR.heatmap_curves(host(score), host(ref), host(regions), n_regions, host(gate), 256, 16)
    CC.assert_curves_equal(res["curves"], ref_plain)
    CC.assert_curves_equal(res["curves_post"], ref_post)
    assert res["curves"]["tp"].shape == (6, 256)
    assert (res["curves_post"]["tp"] <= res["curves"]["tp"]).all() and (res["curves_post"]["tp"] < res["curves"]["tp"]).any()
    if not original:
        # on the working grid the Otsu mask (htp > th) lies between the two cuts around th: t_j <= th < t_(j+1)
        j = int(np.floor(res["threshold"] * 256))
        assert 0 <= j < 255
        tp_mask = int(((res["mask"] > 0) & (torch.from_numpy(lesion).cuda() > 0)).sum())
        assert res["curves"]["tp"][-1, j + 1] <= tp_mask <= res["curves"]["tp"][-1, j]


def test_curves_without_a_reference_mask_are_refused():
    from dram_amd.inference import LobeInference
    inf = LobeInference(_model().cuda().eval(), resample_size=24)
    scan = np.zeros((4, 4, 4), dtype=np.int16)
    with pytest.raises(ValueError, match="lesion"):
        inf.run(scan, np.ones_like(scan, dtype=np.uint8), (1.0, 1.0, 1.0), curves=256)
    with pytest.raises(ValueError, match="lesion"):
        inf.post_process(None, None, torch.zeros(1), 0.5, curves=256)
