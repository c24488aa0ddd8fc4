"""Times forward and backward of the device SegOverlap loss (functional.seg_overlap: per-sample Tversky + focal on logits)
at the benchmark's per-GPU micro-batch (16 x 128^3) and at the reference's shape (10 x 80^3), against the copy rate
measured in the same process, the bytes the definition must move, the existing BinaryCrossEntropySmooth pair
(functional.bce_smooth: the yardstick, same streaming pieces and one logf pair per element) and the definition written in
eager torch on the device (tests/seg_overlap_restatement.torch_seg_overlap), as scripts/seg_loss_bench.py times the BCE pair.

    python scripts/seg_overlap_bench.py [--out FILE] [--shapes 10x1x80,16x1x128] [--reps 10]

HIP events on the launch stream, one warm-up, median and minimum of --reps; forward alone, backward alone (the C entry
point on the forward's state) and the two through autograd.  Traffic of the device form: forward reads z, t and voi once
(float32 masks 12 bytes per voxel, uint8 masks 6, no voi 8 or 5), backward reads the same plus five floats per sample and
writes dz (4 more).  The eager form is timed with float32 masks only.  Prints one JSON line, then a table."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "bodyct-dram_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="10x1x80,16x1x128")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--gamma", type=float, default=2.0)
    args = ap.parse_args()
    import torch
    from dram_amd import _lib
    from dram_amd import functional as HF
    from seg_overlap_restatement import torch_seg_overlap
    if not torch.cuda.is_available():
        raise SystemExit("seg_overlap_bench: needs a GPU (times measured anywhere else say nothing)")
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

    prm = dict(a=.5, b=.5, smooth=1.0, alpha=.25, gamma=args.gamma)
    result = {"device": torch.cuda.get_device_name(0), "hbm_copy_tbs": copy_tbs, "params": prm, "shapes": {}}
    for spec in args.shapes.split(","):
        N, C, size = (int(v) for v in spec.split("x"))
        g = torch.Generator(device=dev).manual_seed(1)
        shape = (N, C, size, size, size)
        z = (torch.randn(shape, device=dev, generator=g) * 2.0).requires_grad_(True)
        voi = (torch.rand(shape, device=dev, generator=g) < 0.6).float()
        t = ((torch.rand(shape, device=dev, generator=g) < 0.05) & (voi > 0)).float()
        t8, voi8 = t.to(torch.uint8), voi.to(torch.uint8)
        el = z.numel()
        rec = {"elements": el}

        def finish(r, nbytes):
            ideal_ms = nbytes / (copy_tbs * 1e12) * 1e3
            r["bytes"] = nbytes
            r["at_copy_rate_ms"] = ideal_ms
            r["fraction_of_copy_rate"] = ideal_ms / r["ms_median"]
            r["gbs"] = nbytes / (r["ms_median"] * 1e-3) / 1e9
            return r

        def fwd_bwd(fn, leaf):
            def run():
                leaf.grad = None
                fn().sum().backward()
            return run

        def device(tt, vv, key, bytes_in):
            """forward alone, backward alone through the C ABI, and both through autograd."""
            zz, tc, kt, vc, kv, Nn, S = HF._seg_overlap_args(z.detach(), tt, vv)
            launch = lambda: HF._seg_overlap_launch(zz, tc, kt, vc, kv, Nn, S, prm["a"], prm["b"], prm["smooth"], prm["alpha"],
                                                    prm["gamma"])
            rec[key + "_fwd"] = finish(timed(launch), el * bytes_in)
            state = launch()[1]
            gout, dz = torch.ones(2, device=dev), torch.empty_like(zz)
            bwd = lambda: _lib.call("dram_seg_overlap_bwd", zz.data_ptr(), tc.data_ptr(), None if vc is None else vc.data_ptr(), kt,
                                    kv, Nn, S, prm["alpha"], prm["gamma"], state.data_ptr(), gout.data_ptr(), dz.data_ptr(), st)
            rec[key + "_bwd"] = finish(timed(bwd), el * (bytes_in + 4.0))
            rec[key] = finish(timed(fwd_bwd(lambda: HF.seg_overlap(z, tt, vv, **prm), z)), el * (2 * bytes_in + 4.0))

        device(t, voi, "seg_overlap_f32_masks", 12.0)
        device(t8, voi8, "seg_overlap_u8_masks", 6.0)
        device(t8, None, "seg_overlap_u8_no_voi", 5.0)
        # the yardstick: the BCE pair on probabilities (the same streaming pieces; two logf per element, no exponential)
        p = torch.sigmoid(z.detach()).requires_grad_(True)
        rec["bce_smooth_f32_target"] = finish(timed(fwd_bwd(lambda: HF.bce_smooth(p, t, 1.0), p)), el * (8 + 12.0))
        rec["bce_smooth_u8_target"] = finish(timed(fwd_bwd(lambda: HF.bce_smooth(p, t8, 1.0), p)), el * (5 + 9.0))
        del p
        torch.cuda.empty_cache()
        rec["eager_seg_overlap"] = timed(fwd_bwd(lambda: torch_seg_overlap(z, t, voi, prm["a"], prm["b"], prm["smooth"],
                                                                           prm["alpha"], prm["gamma"]), z))
        rec["eager_over_device"] = rec["eager_seg_overlap"]["ms_median"] / rec["seg_overlap_f32_masks"]["ms_median"]
        rec["device_over_bce_smooth_f32"] = rec["seg_overlap_f32_masks"]["ms_median"] / rec["bce_smooth_f32_target"]["ms_median"]
        result["shapes"][spec] = rec
        del z, t, voi, t8, voi8
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line, flush=True)
    for spec, rec in result["shapes"].items():
        for k, r in rec.items():
            if isinstance(r, dict):
                tail = f"  {r['gbs']:8.1f} GB/s  {r['fraction_of_copy_rate']:.3f} of the copy rate ({copy_tbs * 1e3:.0f} GB/s)" \
                    if "gbs" in r else ""
                print(f"{spec:>12} {k:<28} {r['ms_median']:8.3f} ms{tail}", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
