"""Times device dropout (dram_dropout: the forward; the backward is the same launch on the gradient) against the copy rate
measured in the same process, as scripts/augment_intensity_bench.py times the intensity transforms.

    python scripts/dropout_bench.py [--out FILE] [--shapes 16x32x128,10x32x80] [--p 0.1] [--reps 10]

HIP events around the launches on the launch stream, one warm-up, median and minimum of --reps.  The pass's traffic is one
read plus one write of the tensor (8 bytes per element).  16 x 32 x 128^3 is the widest stage of the reference model at the
per-GPU micro-batch; beside it the additive Gaussian noise of the augmentation pool (the same generator plus Box-Muller, on
the same number of elements) is timed as the figure dropout must not fall behind.  Prints one JSON line.
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
    ap.add_argument("--shapes", default="16x32x128,10x32x80")
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch
    from dram_amd import _lib
    from dram_amd import functional as HF
    if not torch.cuda.is_available():
        raise SystemExit("dropout_bench: needs a GPU (times measured anywhere else say nothing)")
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
    T, scale = HF.dropout_constants(args.p)
    result = {"device": torch.cuda.get_device_name(0), "hbm_copy_tbs": copy_tbs, "p": args.p, "shapes": {}}

    for spec in args.shapes.split(","):
        N, C, size = (int(v) for v in spec.split("x"))
        x = torch.randn((N, C, size, size, size), device=dev)
        y = torch.empty_like(x)
        nbytes = 2.0 * x.numel() * 4
        ideal_ms = nbytes / (copy_tbs * 1e12) * 1e3
        rec = {"elements": x.numel(), "one_read_one_write_at_copy_rate_ms": ideal_ms}

        def finish(r):
            r["fraction_of_copy_rate"] = ideal_ms / r["ms_median"]
            r["gbs"] = nbytes / (r["ms_median"] * 1e-3) / 1e9
            return r
        rec["dram_dropout"] = finish(timed(lambda: _lib.call("dram_dropout", x.data_ptr(), y.data_ptr(), x.numel(), T, scale,
                                                             1234, 0, st)))
        # the yardstick: dram_aug_gaussian_noise over the same elements as N * C samples (its min / max given, not timed)
        rows, S = N * C, size ** 3
        mm = torch.tensor([[-6.0, 6.0]] * rows, dtype=torch.float32, device=dev)
        sigma = torch.full((rows,), 0.05, dtype=torch.float32, device=dev)
        seeds = torch.arange(1, rows + 1, dtype=torch.int64, device=dev)
        flags = torch.ones(rows, dtype=torch.int32, device=dev)
        rec["dram_aug_gaussian_noise"] = finish(timed(lambda: _lib.call(
            "dram_aug_gaussian_noise", x.data_ptr(), y.data_ptr(), mm.data_ptr(), sigma.data_ptr(), seeds.data_ptr(),
            flags.data_ptr(), rows, None, rows, S, st)))
        rec["dropout_time_over_noise_time"] = rec["dram_dropout"]["ms_median"] / rec["dram_aug_gaussian_noise"]["ms_median"]
        result["shapes"][spec] = rec
        del x, y
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line, flush=True)
    for spec, rec in result["shapes"].items():
        for k in ("dram_dropout", "dram_aug_gaussian_noise"):
            print(f"{spec:>12} {k:<24} {rec[k]['ms_median']:8.3f} ms  {rec[k]['gbs']:8.1f} GB/s  "
                  f"{rec[k]['fraction_of_copy_rate']:.3f} of the copy rate ({copy_tbs * 1e3:.0f} GB/s)", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
