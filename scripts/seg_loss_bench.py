"""Times forward + backward of the device BootBinCrossEntropy and BinaryCrossEntropySmooth (functional.boot_bce /
bce_smooth) against the copy rate measured in the same process and against the same loss written in eager torch on the
device (the expression of oracle.dram_oracle.boot_bce, and the direct transcription of BinaryCrossEntropySmooth), as
scripts/dropout_bench.py times dropout.

    python scripts/seg_loss_bench.py [--out FILE] [--shapes 10x1x80,16x1x128] [--reps 10]

HIP events around forward + backward on the launch stream, one warm-up, median and minimum of --reps.  The traffic the
device form needs: forward reads p and the masks once (BootBinCrossEntropy with float32 masks 12 bytes per element, with
uint8 masks 6; BinaryCrossEntropySmooth 8 or 5), backward reads the same and writes 4.  The eager form is timed with
float32 masks only (it has no other form) and includes its host synchronisation on `tf.sum() > 0`.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "bodyct-dram_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="10x1x80,16x1x128")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--smoothing", type=float, default=0.1)
    args = ap.parse_args()
    import torch
    from dram_amd import _lib
    from dram_amd import functional as HF
    from oracle import dram_oracle as O
    if not torch.cuda.is_available():
        raise SystemExit("seg_loss_bench: needs a GPU (times measured anywhere else say nothing)")
    dev = torch.device("cuda")
    st = torch.cuda.current_stream().cuda_stream

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
        return {"ms_median": statistics.median(ms), "ms_min": min(ms)}

    n = 1 << 30
    src, dst = torch.zeros(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    copy = timed(lambda: _lib.call("dram_calibrate_hbm_copy", src.data_ptr(), dst.data_ptr(), n, st), 5)
    copy_tbs = 2.0 * n / (copy["ms_min"] * 1e-3) / 1e12
    del src, dst
    torch.cuda.empty_cache()

    def torch_bce_smooth(probs, targets, smooth, eps=1e-6):
        p, t = probs.view(-1), targets.view(-1)
        alpha = (1.0 - t.sum() / t.shape[0]).clamp(0.3, 0.7)
        p = p.clamp(eps, 1.0 - eps)
        w = alpha * t + (1.0 - alpha) * (1.0 - t)
        return (-smooth * (torch.log(p) * t + torch.log(1.0 - p) * (1.0 - t)) * w).sum() / w.sum()

    result = {"device": torch.cuda.get_device_name(0), "hbm_copy_tbs": copy_tbs, "smoothing": args.smoothing, "shapes": {}}
    for spec in args.shapes.split(","):
        N, C, size = (int(v) for v in spec.split("x"))
        g = torch.Generator(device=dev).manual_seed(1)
        shape = (N, C, size, size, size)
        p = torch.sigmoid(torch.randn(shape, device=dev, generator=g) * 2.0).requires_grad_(True)
        voi = (torch.rand(shape, device=dev, generator=g) < 0.6).float()
        t = ((torch.rand(shape, device=dev, generator=g) < 0.3) & (voi > 0)).float()
        t8, voi8 = t.to(torch.uint8), voi.to(torch.uint8)
        el = p.numel()
        rec = {"elements": el}

        def fwd_bwd(fn):
            def run():
                p.grad = None
                fn().backward()
            return run

        def finish(r, nbytes):
            ideal_ms = nbytes / (copy_tbs * 1e12) * 1e3
            r["bytes"] = nbytes
            r["at_copy_rate_ms"] = ideal_ms
            r["fraction_of_copy_rate"] = ideal_ms / r["ms_median"]
            r["gbs"] = nbytes / (r["ms_median"] * 1e-3) / 1e9
            return r
        rec["boot_bce_f32_masks"] = finish(timed(fwd_bwd(lambda: HF.boot_bce(p, t, voi, args.smoothing))), el * (12 + 16.0))
        rec["boot_bce_u8_masks"] = finish(timed(fwd_bwd(lambda: HF.boot_bce(p, t8, voi8, args.smoothing))), el * (6 + 10.0))
        rec["bce_smooth_f32_target"] = finish(timed(fwd_bwd(lambda: HF.bce_smooth(p, t, 1.0))), el * (8 + 12.0))
        rec["bce_smooth_u8_target"] = finish(timed(fwd_bwd(lambda: HF.bce_smooth(p, t8, 1.0))), el * (5 + 9.0))
        rec["eager_boot_bce"] = timed(fwd_bwd(lambda: O.boot_bce(p, t, voi, args.smoothing)))
        rec["eager_bce_smooth"] = timed(fwd_bwd(lambda: torch_bce_smooth(p, t, 1.0)))
        rec["eager_over_device_boot_bce"] = rec["eager_boot_bce"]["ms_median"] / rec["boot_bce_f32_masks"]["ms_median"]
        rec["eager_over_device_bce_smooth"] = rec["eager_bce_smooth"]["ms_median"] / rec["bce_smooth_f32_target"]["ms_median"]
        result["shapes"][spec] = rec
        del p, t, voi, t8, voi8
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line, flush=True)
    for spec, rec in result["shapes"].items():
        for k, r in rec.items():
            if isinstance(r, dict):
                tail = f"  {r['gbs']:8.1f} GB/s  {r['fraction_of_copy_rate']:.3f} of the copy rate ({copy_tbs * 1e3:.0f} GB/s)" \
                    if "gbs" in r else ""
                print(f"{spec:>12} {k:<24} {r['ms_median']:8.3f} ms{tail}", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
