"""Times the four intensity transforms beyond the pool (IntensityInverse, GammaTransform, ContrastStretchingTransform,
ContrastJitter of dram_amd/augment.py) against the copy rate measured in the same process, as scripts/augment_bench.py times
the pool's five.

    python scripts/augment_intensity_bench.py [--out FILE] [--shapes 64x128,10x80] [--reps 10]

HIP events around the launches on the launch stream, one warm-up, median and minimum of --reps.  A transform's traffic is
counted as one read plus one write of the tensor (8 bytes per voxel); its pre-passes (min / max: one more read; the jitter's
mean: another) are timed with it and reported as `with_prepass_ms_median`.  A 10 x 80^3 batch (20 MB) fits the 256 MB Infinity
Cache, so its rates are cache rates, not HBM rates.  Prints one JSON line.
"""
import argparse
import json
import os
import random
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "bodyct-dram_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="64x128,10x80")
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch
    from dram_amd import _lib
    from dram_amd import augment as A
    if not torch.cuda.is_available():
        raise SystemExit("augment_intensity_bench: needs a GPU (times measured anywhere else say nothing)")
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
    result = {"device": torch.cuda.get_device_name(0), "hbm_copy_tbs": copy_tbs, "shapes": {}}

    for spec in args.shapes.split(","):
        N, size = (int(v) for v in spec.split("x"))
        shape = (size,) * 3
        random.seed(1)
        np.random.seed(1)
        x = torch.from_numpy(np.random.default_rng(0).random((N,) + shape, dtype=np.float32)).to(dev).unsqueeze(1)
        nbytes = 2.0 * x.numel() * 4
        ideal_ms = nbytes / (copy_tbs * 1e12) * 1e3
        rec = {"voxels": x.numel(), "one_read_one_write_at_copy_rate_ms": ideal_ms, "transforms": {}}
        flags = torch.ones(N, dtype=torch.int32, device=dev)
        y = torch.empty_like(x)
        mm = A.sample_minmax(x)
        for label, t in [("IntensityInverse", A.IntensityInverse()), ("GammaTransform", A.GammaTransform()),
                         ("ContrastStretchingTransform", A.ContrastStretchingTransform()),
                         ("ContrastJitter", A.ContrastJitter()), ("ContrastJitter_volume", A.ContrastJitter(channel_dim=None))]:
            tables = t._tables(t.draw(N, shape), shape, dev)
            if t.uses_minmax:
                r = timed(lambda: t._launch(x, tables, flags, out=y, minmax=mm))       # the kernel alone
                r["with_prepass_ms_median"] = timed(lambda: t._launch(x, tables, flags, out=y))["ms_median"]
            else:                                                                       # statistics of its own, always with it
                par, rows = tables
                row_flags = flags.repeat_interleave(rows)
                smm, mean = A.row_minmax(x, rows, row_flags), A.row_mean(x, rows, row_flags)
                r = timed(lambda: A._intensity_map(x, A.MAP_JITTER, smm, mean, par, True, row_flags, rows, y))
                r["row_mean_ms_median"] = timed(lambda: A.row_mean(x, rows, row_flags))["ms_median"]
                r["with_prepass_ms_median"] = timed(lambda: t._launch(x, tables, flags, out=y))["ms_median"]
            r["fraction_of_copy_rate"] = ideal_ms / r["ms_median"]
            r["tbs"] = nbytes / (r["ms_median"] * 1e-3) / 1e12
            rec["transforms"][label] = r
        result["shapes"][spec] = rec
        del x, y
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
