"""GPU parity of the per-lobe whole-scan inference path (BASELINE config 5 at
reduced size) against the CPU oracle's restatement of evaluate_scan + binary_cam."""
import numpy as np
import pytest
import torch

from oracle import dram_oracle as O
from dram_amd.configs import SLIM

pytestmark = pytest.mark.gpu


def _model(norm="bn"):
    import models
    torch.manual_seed(3)
    m = models.DC3D(**SLIM, norm_method=norm)
    m.init(models.HeNorm(mode="fan_in"))
    # non-trivial running statistics so that eval-mode BatchNorm is exercised
    g = torch.Generator().manual_seed(4)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm3d):
            mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g) * 0.1)
            mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) + 0.5)
    return m


@pytest.mark.parametrize("shape,spacing,R", [((60, 96, 96), (1.0, 0.7, 0.7), 32), ((41, 57, 66), (2.5, 1.0, 1.0), 24)])
def test_lobe_inference_matches_oracle(shape, spacing, R):
    from dram_amd.inference import LobeInference, dice, synthetic_ct
    scan, lobe, spacing = synthetic_ct(shape, spacing, seed=7, n_lesions=8)
    model = _model()
    params, buffers = O.split_state_dict({k: v.clone() for k, v in model.state_dict().items()})
    model = model.cuda().eval()
    res = LobeInference(model, resample_size=R).run(scan, lobe, spacing)
    htp_ref, mask_ref, th_ref, ratio_ref = O.evaluate_scan(SLIM, params, buffers, scan, lobe, spacing, resample=R)
    # crops (find_crops with the 5 mm border)
    for c in res["chunks"]:
        sl = O.find_crops(lobe == c[6], spacing, 5.0)
        assert [s.start for s in sl] == c[:3] and [s.stop - s.start for s in sl] == c[3:6]
    htp = res["htp"].cpu().numpy()
    assert np.abs(htp - htp_ref).max() <= 1e-4 * max(1.0, np.abs(htp_ref).max())
    assert (htp[lobe == 0] == 0).all()
    assert abs(res["threshold"] - th_ref) <= 1.0 / 255.0 + 1e-9        # the 8-bit Otsu bin may move by at most one
    d = dice(res["mask"].cpu().numpy(), mask_ref, 1e-5)
    assert d >= 0.999, d
    assert abs(res["lesion_ratio"] - ratio_ref) <= 1e-5 * max(1.0, abs(ratio_ref))


def test_inference_kernels_edge_cases():
    """absent labels, a single-voxel-thick lobe, windowing limits."""
    from dram_amd.inference import LobeInference
    scan = np.full((12, 20, 24), -1000, dtype=np.int16)
    lobe = np.zeros(scan.shape, dtype=np.uint8)
    lobe[3:9, 4:15, 5:20] = 2          # label 1 absent
    lobe[10, 2:6, 3:9] = 5             # one slice thick
    scan[lobe == 2] = -300             # window maximum -> 1.0
    scan[lobe == 5] = 500              # above the window -> clipped to 1.0
    model = _model().cuda().eval()
    res = LobeInference(model, resample_size=16).run(scan, lobe, (1.0, 1.0, 1.0))
    assert [c[6] for c in res["chunks"]] == [2, 5]
    x = res["input"].cpu().numpy()
    assert x.min() >= 0.0 and abs(x.max() - 1.0) < 1e-6
    params, buffers = O.split_state_dict({k: v.cpu().clone() for k, v in model.state_dict().items()})
    htp_ref, mask_ref, th_ref, _ = O.evaluate_scan(SLIM, params, buffers, scan, lobe, (1.0, 1.0, 1.0), resample=16)
    assert np.abs(res["htp"].cpu().numpy() - htp_ref).max() <= 1e-4


def test_lobe_inference_with_attention_model(golden_dir):
    """The same pipeline with DC3DATGeneric (what process_pipeline.py loads): the refined (second) output
    is what gets pasted (job_runner.py:764)."""
    import os
    import models
    from dram_amd.inference import LobeInference, dice, synthetic_ct
    from dram_amd.configs import SLIM_ATT
    z = np.load(os.path.join(golden_dir, "dc3dat_slim.npz"))
    sd = {k[len("slim_att/sd/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("slim_att/sd/")}
    m = models.DC3DATGeneric(**SLIM_ATT)
    m.load_state_dict(sd)
    params, buffers = O.split_state_dict(sd)
    scan, lobe, spacing = synthetic_ct((41, 57, 66), (2.5, 1.0, 1.0), seed=7, n_lesions=8)
    res = LobeInference(m.cuda().eval(), resample_size=24).run(scan, lobe, spacing)
    fwd = lambda t: O.dc3dat_forward(SLIM_ATT, params, buffers, t, training=False, attention=True)[1]
    htp_ref, mask_ref, th_ref, ratio_ref = O.evaluate_scan(SLIM_ATT, params, buffers, scan, lobe, spacing, resample=24,
                                                           forward=fwd)
    htp = res["htp"].cpu().numpy()
    assert np.abs(htp - htp_ref).max() <= 1e-4
    assert dice(res["mask"].cpu().numpy() > 0, mask_ref) >= 0.999


def test_lobe_inference_arbitrary_labels():
    """evaluate_scan visits every value of np.unique(lobe)[1:] (job_runner.py:729): labels above 5 and more
    than one kernel group (8) of them; a capped label range raises instead of silently dropping lobes."""
    from dram_amd.inference import LobeInference
    rng = np.random.default_rng(5)
    shape = (24, 40, 44)
    scan = rng.normal(-800, 120, size=shape).astype(np.int16)
    lobe = np.zeros(shape, dtype=np.uint8)
    labels = [4, 5, 6, 7, 8, 17, 40, 99, 200, 255]            # 10 lobes -> two model batches (8 + 2)
    for i, lab in enumerate(labels):
        z0, y0, x0 = 2 + 2 * (i % 5), 3 + 7 * (i % 5), 2 + 20 * (i // 5)
        lobe[z0:z0 + 9, y0:y0 + 6, x0:x0 + 17] = lab
    # two labels interleaved inside one 64-voxel wave span of a row (the bbox kernel peels them one by one)
    lobe[20, 30, 0:44:2] = 17
    lobe[20, 30, 1:44:2] = 40
    model = _model().cuda().eval()
    spacing = (1.5, 1.0, 1.0)
    res = LobeInference(model, resample_size=16).run(scan, lobe, spacing)
    assert [c[6] for c in res["chunks"]] == sorted(labels)
    for c in res["chunks"]:
        sl = O.find_crops(lobe == c[6], spacing, 5.0)
        assert [s.start for s in sl] == c[:3] and [s.stop - s.start for s in sl] == c[3:6]
    params, buffers = O.split_state_dict({k: v.cpu().clone() for k, v in model.state_dict().items()})
    htp_ref, mask_ref, th_ref, ratio_ref = O.evaluate_scan(SLIM, params, buffers, scan, lobe, spacing, resample=16)
    htp = res["htp"].cpu().numpy()
    assert np.abs(htp - htp_ref).max() <= 1e-4 * max(1.0, np.abs(htp_ref).max())
    assert abs(res["lesion_ratio"] - ratio_ref) <= 1e-5 * max(1.0, abs(ratio_ref))
    with pytest.raises(ValueError, match="max_labels"):
        LobeInference(model, resample_size=16, max_labels=5).run(scan, lobe, spacing)


def test_config5_full_size_whole_scan():
    """BASELINE config 5 at its stated size: a 300 x 512 x 512 synthetic CT with a 5-lobe label map through
    LobeInference (crop -> 80^3 -> model -> paste -> Otsu) on the device, against the oracle's evaluate_scan
    on the host (one lobe at a time, ~10 s).  Slim DC3D: the data path is what is at full size here; the
    full-width model at 80^3 is covered by test_full_width_eval_inference_5_lobes_at_80.  NB the crop -> 80^3
    resampling grid (restated from ITK's published semantics of the reference's ResampleImageFilter call) and the
    Otsu restatement are unpinned on both sides (SimpleITK / skimage absent), so the Dice below is GPU path vs this
    build's own CPU restatement."""
    import time
    from dram_amd.inference import LobeInference, dice, synthetic_ct
    scan, lobe, spacing = synthetic_ct((300, 512, 512), (1.0, 0.7, 0.7), seed=7, n_lesions=20)
    model = _model()
    params, buffers = O.split_state_dict({k: v.clone() for k, v in model.state_dict().items()})
    model = model.cuda().eval()
    inf = LobeInference(model, resample_size=80)
    scan_d, lobe_d = torch.as_tensor(scan).cuda(), torch.as_tensor(lobe).cuda()
    res = inf.run(scan_d, lobe_d, spacing)                      # warm-up (first launches)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = inf.run(scan_d, lobe_d, spacing)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    assert [c[6] for c in res["chunks"]] == [1, 2, 3, 4, 5]
    t0 = time.perf_counter()
    htp_ref, mask_ref, th_ref, ratio_ref = O.evaluate_scan(SLIM, params, buffers, scan, lobe, spacing, resample=80)
    cpu_s = time.perf_counter() - t0
    htp = res["htp"].cpu().numpy()
    err = float(np.abs(htp - htp_ref).max())
    d = dice(res["mask"].cpu().numpy(), mask_ref, 1e-5)
    print(f"\nconfig 5 (300x512x512, 5 lobes, slim DC3D @80^3): {ms:.1f} ms/scan on the device (scan resident in HBM), "
          f"oracle {cpu_s:.1f} s on the host; htp max-abs err {err:.2e}, mask Dice {d:.6f}")
    assert err <= 1e-4 * max(1.0, float(np.abs(htp_ref).max()))
    assert (htp[lobe == 0] == 0).all()
    assert abs(res["threshold"] - th_ref) <= 1.0 / 255.0 + 1e-9
    assert d >= 0.999, d
    assert abs(res["lesion_ratio"] - ratio_ref) <= 1e-5 * max(1.0, abs(ratio_ref))


def _full_width_model(kind):
    """The model process_pipeline.py loads (st_dram_ref_att: DC3DATGeneric, process_pipeline.py:11) / its plain counterpart
    (st_dram_ref: DC3D) at FULL channel widths, HeNorm-initialised, with non-trivial BatchNorm affine parameters and running
    statistics -- what eval mode reads."""
    import models
    from dram_amd.configs import ST_DRAM_REF_ATT_MODEL, ST_DRAM_REF_MODEL
    torch.manual_seed(5)
    m = models.DC3DATGeneric(**ST_DRAM_REF_ATT_MODEL) if kind == "att" else models.DC3D(**ST_DRAM_REF_MODEL)
    m.init(models.HeNorm(mode="fan_in"))
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm3d):
                mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g) * 0.05)
                mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) * 0.5 + 0.75)
                mod.weight.copy_(1.0 + 0.2 * torch.randn(mod.weight.shape, generator=g))
                mod.bias.copy_(0.1 * torch.randn(mod.bias.shape, generator=g))
    return m


@pytest.mark.parametrize("kind", ["dc3d", "att"])
def test_full_width_eval_inference_5_lobes_at_80(kind):
    """Config 5's model path at FULL width (the other inference tests run the slim model): five lobes -> 5 x 80^3 through
    the fused engine in EVAL mode (BatchNorm from running statistics: dram_bn_eval_coef; levels 80 / 40 / 20 / 10) for
    DC3D(st_dram_ref) and for DC3DATGeneric(st_dram_ref_att) -- the model process_pipeline.py:11 loads; its refined second
    output is what evaluate_scan pastes, job_runner.py:764 -- against the oracle's evaluate_scan on the host (one lobe at a
    time, torch CPU).  Match: job_runner.py:729-770, models.py:543-597.  (The PCM itself is pinned in tests/test_gpu_pcm.py.)"""
    import time
    from dram_amd import engine
    from dram_amd import functional as HF
    from dram_amd.configs import ST_DRAM_REF_ATT_MODEL, ST_DRAM_REF_MODEL
    from dram_amd.inference import LobeInference, dice, synthetic_ct
    torch.set_num_threads(16)
    cfg = ST_DRAM_REF_ATT_MODEL if kind == "att" else ST_DRAM_REF_MODEL
    scan, lobe, spacing = synthetic_ct((120, 160, 160), (1.0, 0.7, 0.7), seed=7, n_lesions=10)
    model = _full_width_model(kind)
    params, buffers = O.split_state_dict({k: v.clone() for k, v in model.state_dict().items()})
    model = model.cuda().eval()
    assert model.fused and engine.supports(model)
    before = HF.conv_launch_counts()
    res = LobeInference(model, resample_size=80).run(scan, lobe, spacing)
    torch.cuda.synchronize()
    delta = [a - b for a, b in zip(HF.conv_launch_counts(), before)]
    assert [c[6] for c in res["chunks"]] == [1, 2, 3, 4, 5] and tuple(res["input"].shape) == (5, 1, 80, 80, 80)
    assert sum(delta[k] for k in (HF.K3_FWD_C1, HF.K3_FWD_WZ, HF.K3_FWD_WZY, HF.K3_FWD_DIRECT)) == 14, delta   # one batch of 5
    fwd = None
    if kind == "att":
        fwd = lambda t: O.dc3dat_forward(cfg, params, buffers, t, training=False, attention=True)[1]
    t0 = time.perf_counter()
    htp_ref, mask_ref, th_ref, ratio_ref = O.evaluate_scan(cfg, params, buffers, scan, lobe, spacing, resample=80, forward=fwd)
    cpu_s = time.perf_counter() - t0
    htp = res["htp"].cpu().numpy()
    err = float(np.abs(htp - htp_ref).max())
    d = dice(res["mask"].cpu().numpy(), mask_ref, 1e-5)
    print(f"\nfull-width {kind} eval, 5 lobes x 80^3: htp max-abs err {err:.2e} (range {htp_ref.min():.3f}..{htp_ref.max():.3f}), "
          f"mask Dice {d:.6f}, oracle {cpu_s:.1f} s")
    assert float(htp_ref.max() - htp_ref[lobe > 0].min()) > 1e-3          # not a constant map
    assert err <= 1e-4 * max(1.0, float(np.abs(htp_ref).max()))
    assert (htp[lobe == 0] == 0).all()
    assert abs(res["threshold"] - th_ref) <= 1.0 / 255.0 + 1e-9
    assert d >= 0.999, d
    assert abs(res["lesion_ratio"] - ratio_ref) <= 1e-5 * max(1.0, abs(ratio_ref))


def test_lesion_post_processing_tail(golden_dir):
    """The tail of LesionSegTest.run on the device (job_runner.py:1003-1012, 1033-1037; csrc/infer.hip dram_scan_hist256 /
    dram_lesion_post / dram_mask_overlap): the 8-bit histogram of the default-windowed scan inside the lungs is BIT-exact
    against the reference's own numbers (tests/golden/infer_tail.npz), lesion_pred_post = lesion_pred & (w_scan > th) & ~vessel
    and IOU / Dice equal the oracle's restatement bit for bit (integer / fp64 work) on a synthetic scan through LobeInference."""
    import os
    from dram_amd import _lib
    from dram_amd.inference import LobeInference, synthetic_ct
    z = np.load(os.path.join(golden_dir, "infer_tail.npz"))
    st = torch.cuda.current_stream().cuda_stream
    scan_d, lobe_d = torch.as_tensor(z["scan"]).cuda(), torch.as_tensor(z["lobe"]).cuda()
    hist = torch.empty(256, dtype=torch.int64, device="cuda")
    _lib.call("dram_scan_hist256", scan_d.data_ptr(), lobe_d.data_ptr(), hist.data_ptr(), -1150, 350, scan_d.numel(), st)
    assert np.array_equal(hist.cpu().numpy(), z["hist"])
    a_d, b_d = torch.as_tensor(z["a"]).cuda(), torch.as_tensor(z["b"]).cuda()
    counts = torch.empty(4, dtype=torch.int64, device="cuda")
    _lib.call("dram_mask_overlap", a_d.data_ptr(), b_d.data_ptr(), counts.data_ptr(), a_d.numel(), st)
    c = [int(v) for v in counts.cpu()]
    assert (c[0] + 1e-5) / (c[1] + 1e-5) == float(z["iou"]) and (2.0 * c[0] + 1e-5) / (c[2] + c[3] + 1e-5) == float(z["dice"])

    scan, lobe, spacing = synthetic_ct((60, 96, 96), (1.0, 0.7, 0.7), seed=7, n_lesions=8)
    rng = np.random.default_rng(3)
    vessel = ((rng.random(scan.shape) > 0.9) & (lobe > 0)).astype(np.uint8)
    lesion = ((scan > -600) & (lobe > 0)).astype(np.uint8)
    model = _model().cuda().eval()
    res = LobeInference(model, resample_size=32).run(scan, lobe, spacing, vessel=vessel, lesion=lesion)
    htp = res["htp"].cpu().numpy()
    pred_ref, post_ref, th2_ref = O.lesion_post_process(htp, scan, lobe, vessel, res["threshold"])
    assert res["threshold_scan"] == th2_ref
    mask, post = res["mask"].cpu().numpy(), res["mask_post"].cpu().numpy()
    assert np.array_equal(mask, pred_ref) and np.array_equal(post, post_ref)
    assert (post <= mask).all() and (post[vessel > 0] == 0).all()
    print(f"\npost-processing tail: |mask| {int(mask.sum())}, |mask_post| {int(post.sum())}, brightness threshold {th2_ref:.4f}, "
          f"iou {res['iou']:.4f} -> {res['iou_post']:.4f}")
    assert res["iou"] == O.iou(pred_ref > 0, lesion > 0, 1e-5) and res["iou_post"] == O.iou(post_ref > 0, lesion > 0, 1e-5)
    assert res["dice"] == O.dice(pred_ref > 0, lesion > 0, 1e-5) and res["dice_post"] == O.dice(post_ref > 0, lesion > 0, 1e-5)
    # without a vessel mask: only the brightness gate
    res2 = LobeInference(model, resample_size=32).run(scan, lobe, spacing, lesion=lesion)
    _, post2, _ = O.lesion_post_process(htp, scan, lobe, None, res["threshold"])
    assert np.array_equal(res2["mask_post"].cpu().numpy(), post2)


def test_crop_resampling_grid_follows_the_itk_call():
    """The crop -> R^3 step restates sitk.ResampleImageFilter(identity transform, same origin, spacing * in / out, linear, default 0)
    (reference utils.py:371-381): output voxel o samples continuous index o * in / out; a crop SMALLER than R along an axis
    leaves the output planes at c >= in - 0.5 at the default value 0 (IsInsideBuffer), the plane before them clamped to the last
    voxel.  Device kernel against the oracle's fp64 restatement, and the two properties spelled out."""
    from dram_amd import _lib
    import ctypes
    rng = np.random.default_rng(11)
    D, H, W, R = 10, 50, 33, 16                       # z: upsampled (10 -> 16), y: downsampled, x: 33 -> 16
    scan = rng.integers(-1000, -300, size=(D, H, W)).astype(np.int16)
    lobe = np.ones((D, H, W), dtype=np.uint8)
    st = torch.cuda.current_stream().cuda_stream
    out = torch.empty((1, 1, R, R, R), device="cuda")
    scan_d, lobe_d = torch.as_tensor(scan).cuda(), torch.as_tensor(lobe).cuda()      # (kept alive across the launches)
    chunk = (ctypes.c_int * 7)(0, 0, 0, D, H, W, 1)
    _lib.call("dram_lobe_chunks", scan_d.data_ptr(), lobe_d.data_ptr(), out.data_ptr(), chunk, 1, D, H, W, R, -1000.0, -300.0, st)
    got = out[0, 0].cpu().numpy()
    img = O.windowing(scan.astype(np.float32), (-1000.0, -300.0)).astype(np.float32)
    ref = O.resample_itk_linear(img, (R, R, R))
    assert np.abs(got - ref).max() <= 1e-5
    # z: c = o * 10 / 16: o = 15 -> 9.375 (clamped to the last plane, inside: < 9.5); nothing outside.  A 4-plane crop: o >= 14 -> 0
    chunk4 = (ctypes.c_int * 7)(0, 0, 0, 4, H, W, 1)
    _lib.call("dram_lobe_chunks", scan_d.data_ptr(), lobe_d.data_ptr(), out.data_ptr(), chunk4, 1, D, H, W, R, -1000.0, -300.0, st)
    got4 = out[0, 0].cpu().numpy()
    assert (got4[14:] == 0).all() and (got4[13] != 0).any()            # c = 3.5 at o = 14: the first plane outside [-0.5, 3.5)
    assert np.abs(got4 - O.resample_itk_linear(img[:4], (R, R, R))).max() <= 1e-5


@pytest.mark.parametrize("case", ["up", "down", "mixed"])
def test_resample_back_to_the_original_grid(case):
    """`utils.resample(..., required_spacing=original_spacing, new_size=original_size)` of LesionSegTest.run (job_runner.py:1016-1032)
    on the device (csrc/infer.hip dram_resample_volume) against the oracle's numpy restatement of the same sitk call: masks
    (uint8, nearest) and the int16 scan (linear, clamp + truncation) BIT-exact -- the index arithmetic is the same fp64
    expression on both sides --, the float heat map to 1e-6.  Parity against SimpleITK itself is unpinned (library absent)."""
    from dram_amd.inference import resample_volume
    rng = np.random.default_rng(5)
    shape = (21, 34, 40)
    spacing = (1.25, 0.8, 0.8)
    if case == "up":                 # finer original grid; more voxels than the resampled extent covers along z (default value 0)
        req, size = (0.5, 0.4, 0.4), (56, 68, 80)
    elif case == "down":
        req, size = (2.5, 1.5, 1.7), (10, 19, 18)
    else:                            # same spacing along x (the identity there), coarser z, finer y, size cut short along y
        req, size = (2.0, 0.3, 0.8), (11, 70, 40)
    mask = (rng.random(shape) > 0.6).astype(np.uint8) * rng.integers(1, 6, size=shape).astype(np.uint8)
    scan = rng.integers(-1200, 600, size=shape).astype(np.int16)
    htp = rng.random(shape).astype(np.float32)
    for arr, how, tol in ((mask, "nearest", 0), (scan, "linear", 0), (scan, "nearest", 0), (htp, "linear", 1e-6), (htp, "nearest", 0),
                          (mask, "linear", 0)):
        got = resample_volume(torch.as_tensor(arr).cuda(), spacing, req, size, how).cpu().numpy()
        ref = O.resample_itk(arr, spacing, req, size, how)
        assert got.shape == tuple(size) and got.dtype == arr.dtype
        if tol == 0:
            assert np.array_equal(got, ref), (case, arr.dtype, how, int((got != ref).sum()))
        else:
            assert np.abs(got - ref).max() <= tol
    if case == "up":                 # c = o * 0.4: inside while c < 20.5 -> planes 52.. are the default value
        got = resample_volume(torch.as_tensor(scan).cuda(), spacing, req, size, "linear").cpu().numpy()
        assert (got[52:] == 0).all() and (got[51] != 0).any()
    if case == "mixed":              # x: same spacing, same size: every x column is an input column
        got = resample_volume(torch.as_tensor(htp).cuda(), (1.0, 1.0, 0.8), (1.0, 1.0, 0.8), shape, "linear")
        assert torch.equal(got.cpu(), torch.as_tensor(htp))
    with pytest.raises(NotImplementedError):
        resample_volume(torch.as_tensor(htp).cuda(), spacing, req, size, "bspline")


def test_lesion_metrics_on_the_original_grid():
    """LobeInference.run(..., original_spacing=, original_size=): the masks / scan / heat map taken back to the scan's original
    grid and IOU / Dice computed THERE (job_runner.py:1016-1037), against the oracle's restatement fed with the device heat map."""
    from dram_amd.inference import LobeInference, synthetic_ct
    scan, lobe, spacing = synthetic_ct((48, 80, 80), (1.4, 0.9, 0.9), seed=9, n_lesions=6)
    rng = np.random.default_rng(4)
    vessel = ((rng.random(scan.shape) > 0.92) & (lobe > 0)).astype(np.uint8)
    lesion = ((scan > -600) & (lobe > 0)).astype(np.uint8)
    o_spacing, o_size = (0.7, 0.6, 0.6), (96, 120, 120)
    model = _model().cuda().eval()
    res = LobeInference(model, resample_size=32).run(scan, lobe, spacing, vessel=vessel, lesion=lesion,
                                                     original_spacing=o_spacing, original_size=o_size)
    htp = res["htp"].cpu().numpy()
    pred, post, _ = O.lesion_post_process(htp, scan, lobe, vessel, res["threshold"])
    back = lambda a, how: O.resample_itk(a, spacing, o_spacing, o_size, how)
    ref = {"mask": back(pred, "nearest"), "mask_post": back(post, "nearest"), "lesion": back(lesion, "nearest"),
           "scan": back(scan, "linear"), "htp": back(htp, "linear")}
    got = {k: v.cpu().numpy() for k, v in res["original"].items()}
    assert set(got) == set(ref)
    for k in ("mask", "mask_post", "lesion", "scan"):
        assert got[k].shape == o_size and np.array_equal(got[k], ref[k]), k
    assert np.abs(got["htp"] - ref["htp"]).max() <= 1e-6
    assert res["mask"].shape == scan.shape                       # the working-resolution results stay what they were
    assert res["iou"] == O.iou(ref["mask"] > 0, ref["lesion"] > 0, 1e-5)
    assert res["iou_post"] == O.iou(ref["mask_post"] > 0, ref["lesion"] > 0, 1e-5)
    assert res["dice"] == O.dice(ref["mask"] > 0, ref["lesion"] > 0, 1e-5)
    assert res["dice_post"] == O.dice(ref["mask_post"] > 0, ref["lesion"] > 0, 1e-5)
    with pytest.raises(ValueError):
        LobeInference(model, resample_size=32).run(scan, lobe, spacing, lesion=lesion, original_size=o_size)
