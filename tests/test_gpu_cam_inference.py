"""LobeInference(head="cam"): the lobe-wise class head of the reference's inference entry point (LesionSegTest.run,
job_runner.py:985-1004) on the device, against the oracle's forward plus the restatement of tests/cam_cases.py
(cam_scan_ref), at the scan and resample sizes tests/test_gpu_inference.py uses for its slim models.

The six-channel heads are the HeNorm ones scaled (so that the lobes' pooled rows differ by more than rounding) with biases
chosen on the oracle so that the lobes get different classes, one of them class 0, and every row's top-2 gap is at least
cam_cases.MIN_GAP = 100 x the dense-output tolerance -- asserted below on the CPU side, so that `lobe_cls` can be held to
equality."""
import numpy as np
import pytest
import torch

import cam_cases as CK
from oracle import dram_oracle as O
from dram_amd.configs import SLIM, SLIM_ATT

pytestmark = pytest.mark.gpu

#        kind    scan shape    spacing          R   head scale  head biases
CASES = {
    "dc3d_60x96x96": ("dc3d", (60, 96, 96), (1.0, 0.7, 0.7), 32, 16.0, [3.359, -2.684, 1.162, -5.242, 0.002, -3.155]),
    "dc3d_41x57x66": ("dc3d", (41, 57, 66), (2.5, 1.0, 1.0), 24, 16.0, [3.186, -2.59, 0.779, -4.838, 0.002, -3.118]),
    "att_41x57x66": ("att", (41, 57, 66), (2.5, 1.0, 1.0), 24, 32.0, [-48.332, 0.0, 0.0, 0.0, 0.0, 0.0]),
}


def build(kind, out_ch, scale=1.0, bias=None):
    """The slim model of tests/test_gpu_inference.py (HeNorm, non-trivial running statistics) with `out_ch` channels."""
    import models
    torch.manual_seed(3)
    cfg = dict(SLIM_ATT if kind == "att" else SLIM, out_ch=out_ch)
    m = (models.DC3DATGeneric if kind == "att" else models.DC3D)(**cfg)
    m.init(models.HeNorm(mode="fan_in"))
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm3d):
                mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g) * 0.1)
                mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) + 0.5)
        m.top_layer.weight.mul_(scale)
        if bias is not None:
            m.top_layer.bias.copy_(torch.tensor(bias, dtype=torch.float32))
    return cfg, m


def oracle_forward(kind, cfg, model):
    params, buffers = O.split_state_dict({k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
    if kind == "att":           # the refined (second) output is what the head reads (job_runner.py:985)
        return lambda t, mask: O.dc3dat_forward(cfg, params, buffers, t, training=False, attention=True)[1]
    return lambda t, mask: O.dc3d_forward(cfg, params, buffers, t, training=False)


@pytest.mark.parametrize("case", sorted(CASES))
def test_cam_head_matches_oracle_and_restatement(case):
    from dram_amd.inference import LobeInference, lobewise_records, synthetic_ct
    kind, shape, spacing, R, scale, bias = CASES[case]
    scan, lobe, spacing = synthetic_ct(shape, spacing, seed=7, n_lesions=8)
    cfg, model = build(kind, 6, scale, bias)
    htp_ref, tol, cls_ref, pool_ref, absmax = CK.cam_scan_ref(oracle_forward(kind, cfg, model), scan, lobe, spacing, R)
    # the CPU side: what the inputs have to be for the comparison below to mean something
    assert sorted(cls_ref) == [1, 2, 3, 4, 5]
    for label, row in pool_ref.items():
        top = np.sort(row)
        assert np.isfinite(row).all() and top[-1] - top[-2] >= CK.MIN_GAP, (label, row)
    assert 0 in cls_ref.values() and len(set(cls_ref.values())) >= 2
    zero_lobes = [k for k, v in cls_ref.items() if v == 0]
    assert all((htp_ref[lobe == k] == 0).all() for k in zero_lobes) and 0.5 < htp_ref.max() <= 1.0

    res = LobeInference(model.cuda().eval(), resample_size=R, head="cam").run(scan, lobe, spacing)
    assert res["lobe_cls"] == cls_ref                                         # every lobe, none left out
    chunks = [tuple(c) for c in res["chunks"]]
    assert [c[6] for c in chunks] == [1, 2, 3, 4, 5]
    assert np.array_equal(res["lobe_mask"].cpu().numpy()[:, 0], CK.chunk_mask_ref(lobe, chunks, R))
    pool = res["pool"].cpu().numpy()
    assert pool.shape == (5, 6)
    for i, label in enumerate(sorted(pool_ref)):                              # a masked mean of values that agree to DENSE_TOL
        assert np.abs(pool[i] - pool_ref[label]).max() <= 2 * CK.DENSE_TOL * max(1.0, absmax[label])
    htp = res["htp"].cpu().numpy()
    err = np.abs(htp.astype(np.float64) - htp_ref)
    print(f"\ncam head {case}: classes {res['lobe_cls']}, htp max err {err.max():.2e} (bound up to {tol.max():.2e})")
    assert np.isfinite(htp).all() and (err <= tol).all()
    assert (htp[lobe == 0] == 0).all() and all((htp[lobe == k] == 0).all() for k in zero_lobes)
    assert 0.0 <= res["threshold"] <= 1.0 and res["mask"].shape == scan.shape
    # the records LesionSegTest.run keeps, from the device's classes
    targets = {1: 0, 2: 3, 3: 3, 4: 1, 5: 0}
    preds, tgts, acc = lobewise_records(res, targets)
    assert preds == [cls_ref[k] for k in range(1, 6)] and tgts == [targets[k] for k in range(1, 6)]
    assert acc == np.mean([cls_ref[k] == targets[k] for k in range(1, 6)])


@pytest.mark.parametrize("kind", ["dc3d", "att"])
def test_one_channel_model_predicts_class_0_and_an_all_zero_map(kind):
    """NR_CLASS = 1, the shipped setting: the arg-max of a one-channel row is 0, so the reference writes an all-zero map."""
    from dram_amd.inference import LobeInference, synthetic_ct
    scan, lobe, spacing = synthetic_ct((41, 57, 66), (2.5, 1.0, 1.0), seed=7, n_lesions=8)
    cfg, model = build(kind, 1)
    res = LobeInference(model.cuda().eval(), resample_size=24, head="cam").run(scan, lobe, spacing)
    assert res["lobe_cls"] == {1: 0, 2: 0, 3: 0, 4: 0, 5: 0} and tuple(res["pool"].shape) == (5, 1)
    assert not bool(res["htp"].any()) and not bool(res["mask"].any())
    assert res["lesion_ratio"] == 0.0 and res["ctss"] == 0


def test_sigmoid_head_is_the_default_and_unchanged():
    from dram_amd.inference import LobeInference, synthetic_ct
    scan, lobe, spacing = synthetic_ct((41, 57, 66), (2.5, 1.0, 1.0), seed=7, n_lesions=8)
    cfg, model = build("dc3d", 1)
    model = model.cuda().eval()
    a = LobeInference(model, resample_size=24).run(scan, lobe, spacing)
    b = LobeInference(model, resample_size=24, head="sigmoid").run(scan, lobe, spacing)
    assert set(a) == set(b) == {"htp", "mask", "threshold", "lesion_ratio", "ctss", "chunks", "input"}
    assert torch.equal(a["htp"], b["htp"]) and torch.equal(a["mask"], b["mask"]) and torch.equal(a["input"], b["input"])
    assert a["threshold"] == b["threshold"] and a["lesion_ratio"] == b["lesion_ratio"] and a["chunks"] == b["chunks"]
    params, buffers = O.split_state_dict({k: v.cpu().clone() for k, v in model.state_dict().items()})
    htp_ref = O.evaluate_scan(cfg, params, buffers, scan, lobe, spacing, resample=24)[0]
    assert np.abs(a["htp"].cpu().numpy() - htp_ref).max() <= 1e-4
    with pytest.raises(ValueError, match="head"):
        LobeInference(model, head="softmax")
