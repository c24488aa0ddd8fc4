"""Times test-time augmentation of the per-lobe inference (csrc/infer_tta.hip, dram_amd/inference.py) on the scan of
inference.synthetic_ct() at 300x512x512, spacing (1.0, 0.7, 0.7), with the full-width attention model (DC3DATGeneric,
st_dram_ref_att) at 80^3, against the copy rate measured in the same process.

    python scripts/tta_bench.py [--out FILE] [--shape 300,512,512] [--reps 5] [--modes none,flip,full] [--no-kernels]
                                [--inference-module FILE]

Kernels (HIP events around each call on the launch stream, one warm-up, median and minimum of --reps), on the L chunks of the
scan, against the bytes the definition makes each move, at the copy rate:
  dram_tta_expand       reads L R^3 floats, writes V L R^3                                  V = 8 ("flip") and 48 ("full")
  dram_tta_combine      reads V L R^3 floats, writes 2 L R^3 (mean and spread)              "flip", "full", and separately the 16
                        views of "full" that keep x in place and the 32 that move it
  dram_lobe_paste_prob  reads 1 byte of the lobe map per crop voxel and the two fields (2 L R^3 floats), writes 8 bytes per
                        voxel inside a lobe
Whole runs (host clock around LobeInference.run; it ends in the histogram read-back): tta None, "flip" and "full", each beside
V times the model's forward on the L chunks (events), the least the ensemble can cost.
--inference-module loads LobeInference from another file (another revision's dram_amd/inference.py) for an A/B of the
tta=None path with this same script; with --modes none --no-kernels it needs nothing that revision lacks.
Prints a table, then one JSON line.
"""
import argparse
import ctypes
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "bodyct-dram_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def full_width_attention_model():
    """The model process_pipeline.py loads, at full channel widths, HeNorm-initialised, with non-trivial BatchNorm statistics."""
    import torch
    import models
    from dram_amd.configs import ST_DRAM_REF_ATT_MODEL
    torch.manual_seed(5)
    m = models.DC3DATGeneric(**ST_DRAM_REF_ATT_MODEL)
    m.init(models.HeNorm(mode="fan_in"))
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm3d):
                mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g) * 0.05)
                mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) * 0.5 + 0.75)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", default="300,512,512")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--modes", default="none,flip,full")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--inference-module", default=None)
    args = ap.parse_args()
    import torch
    from dram_amd import _lib
    if args.inference_module:
        spec = importlib.util.spec_from_file_location("dram_amd._bench_inference", args.inference_module)
        inference = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(inference)
    else:
        from dram_amd import inference
    if not torch.cuda.is_available():
        raise SystemExit("tta_bench: needs a GPU (times measured anywhere else say nothing)")
    dev = torch.device("cuda")
    st = torch.cuda.current_stream().cuda_stream
    shape = tuple(int(v) for v in args.shape.split(","))
    R = 80

    def timed(fn, reps=args.reps):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}

    n = 1 << 30
    src, dst = torch.zeros(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    copy = timed(lambda: _lib.call("dram_calibrate_hbm_copy", src.data_ptr(), dst.data_ptr(), n, st), 5)
    copy_tbs = 2.0 * n / (copy["ms_min"] * 1e-3) / 1e12
    del src, dst
    torch.cuda.empty_cache()

    scan, lobe, spacing = inference.synthetic_ct(shape, (1.0, 0.7, 0.7))
    D, H, W = shape
    scan_d, lobe_d = torch.from_numpy(scan).to(dev), torch.from_numpy(lobe).to(dev)
    model = full_width_attention_model().to(dev).eval()
    result = {"device": torch.cuda.get_device_name(0), "shape": list(shape), "R": R, "hbm_copy_tbs": copy_tbs,
              "inference_module": args.inference_module, "calls": {}, "runs": {}}

    def record(name, t, nbytes):
        floor = nbytes / (copy_tbs * 1e12) * 1e3
        t.update(bytes=nbytes, floor_ms=floor, over_floor=t["ms_median"] / floor, tbs=nbytes / (t["ms_median"] * 1e-3) / 1e12)
        result["calls"][name] = t

    plain = inference.LobeInference(model, resample_size=R).run(scan_d, lobe_d, spacing)      # also the warm-up of the model
    chunks, x = plain["chunks"], plain["input"]
    L, S = len(chunks), R ** 3
    result["chunks"] = L
    with torch.no_grad():
        fwd = timed(lambda: model(x, None))
    result["forward_ms"] = fwd

    if not args.no_kernels:
        full = inference.tta_views("full")
        sets = {"flip (8)": inference.tta_views("flip"), "full (48)": full,
                "keep x (16 of full)": tuple(v for v in full if v[0][2] == 2),
                "move x (32 of full)": tuple(v for v in full if v[0][2] != 2)}
        buf = torch.randn((48 * L, 1, R, R, R), dtype=torch.float32, device=dev)
        both = torch.empty((2, L, R, R, R), dtype=torch.float32, device=dev)
        for name, views in sets.items():
            V = len(views)
            varr = (ctypes.c_int * (6 * V))(*[a for perm, flip in views for a in perm + flip])
            if "of full" not in name:
                record(f"tta_expand {name}", timed(lambda: _lib.call("dram_tta_expand", x.data_ptr(), buf.data_ptr(), L, R, varr, V, st)),
                       4 * L * S * (1 + V))
            record(f"tta_combine {name}", timed(lambda: _lib.call("dram_tta_combine", buf.data_ptr(), both[0].data_ptr(),
                                                                  both[1].data_ptr(), L, R, varr, V, st)), 4 * L * S * (V + 2))
        carr = (ctypes.c_int * (7 * L))(*[v for c in chunks for v in c])
        htp, spread = torch.zeros(shape, dtype=torch.float32, device=dev), torch.zeros(shape, dtype=torch.float32, device=dev)
        crop_voxels = sum(c[3] * c[4] * c[5] for c in chunks)
        lobe_voxels = int((lobe > 0).sum())
        result.update(crop_voxels=crop_voxels, lobe_voxels=lobe_voxels)
        record("lobe_paste_prob (mean and spread)",
               timed(lambda: _lib.call("dram_lobe_paste_prob", both[0].data_ptr(), both[1].data_ptr(), lobe_d.data_ptr(), htp.data_ptr(),
                                       spread.data_ptr(), carr, L, D, H, W, R, st)), crop_voxels + 8 * lobe_voxels + 8 * L * S)
        del buf, both, htp, spread
        torch.cuda.empty_cache()

    for mode in args.modes.split(","):
        kw = {} if mode == "none" else {"tta": mode}
        inf = inference.LobeInference(model, resample_size=R, **kw)
        V = 1 if mode == "none" else len(inf.views)

        def whole():
            inf.run(scan_d, lobe_d, spacing)
            torch.cuda.synchronize()
        whole()
        ms = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            whole()
            ms.append((time.perf_counter() - t0) * 1e3)
        result["runs"][mode] = {"V": V, "ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms),
                                "forward_floor_ms": V * fwd["ms_median"]}

    print(f"{result['device']}: {shape}, {L} chunks at {R}^3, copy rate {copy_tbs:.2f} TB/s, forward on {L} chunks "
          f"{fwd['ms_median']:.2f} ms (min {fwd['ms_min']:.2f})")
    for name, t in result["calls"].items():
        print(f"  {name:36s} median {t['ms_median']:8.3f} ms (min {t['ms_min']:.3f}), {t['tbs']:.2f} TB/s, floor {t['floor_ms']:.3f} ms, "
              f"{t['over_floor']:.2f} x the floor")
    for mode, t in result["runs"].items():
        print(f"  run(tta={mode:4s}) V={t['V']:2d}: median {t['ms_median']:9.2f} ms (min {t['ms_min']:.2f}, max {t['ms_max']:.2f}); "
              f"V x forward = {t['forward_floor_ms']:.2f} ms; the rest {t['ms_median'] - t['forward_floor_ms']:.2f} ms")
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
