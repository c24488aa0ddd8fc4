"""Times the launches behind RandomCrop and StandarizeChannel (dram_aug_pad_min, dram_aug_crop_resample for fp32 linear and uint8
nearest with and without windows that leave the chunk, dram_aug_row_mean_std and the standardise map) against the copy rate
measured in the same process, as scripts/augment_region_bench.py times the region masks.

    python scripts/augment_crop_bench.py [--out FILE] [--shapes 64x128,10x80] [--reps 10]

HIP events around the launches on the launch stream, one warm-up, median and minimum of --reps.  The crop-resample, the map and
the standardise pair are counted as one read plus one write of the tensor; the two reductions as the reads they make (pad_min:
two reads of the samples that pad; row_mean_std: two reads).  The crop-resample reads only its windows, so its true traffic is
below what is counted.  A 10 x 80^3 batch (20 MB) fits the 256 MB Infinity Cache, so its rates are cache rates, not HBM rates.
Prints one JSON line.
"""
import argparse
import json
import os
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
        raise SystemExit("augment_crop_bench: needs a GPU (times measured anywhere else say nothing)")
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
        x = torch.from_numpy(np.random.default_rng(0).random((N,) + shape, dtype=np.float32)).to(dev).unsqueeze(1)
        m = (x * 5).to(torch.uint8)
        flags = torch.ones(N, dtype=torch.int32, device=dev)
        rec = {"voxels": x.numel(), "launches": {}}

        def add(label, fn, nbytes):
            ideal_ms = nbytes / (copy_tbs * 1e12) * 1e3
            r = timed(fn)
            r["counted_bytes_at_copy_rate_ms"] = ideal_ms
            r["fraction_of_copy_rate"] = ideal_ms / r["ms_median"]
            r["tbs"] = nbytes / (r["ms_median"] * 1e-3) / 1e12
            rec["launches"][label] = r

        y, ym = torch.empty_like(x), torch.empty_like(m)
        # every sample's window leaves the chunk (a wide setting, drawn until it does) / no window does
        np.random.seed(0)
        wide, narrow = A.RandomCrop((0.9,) * 3, (0.6,) * 3), A.RandomCrop((0.0,) * 3, (0.7,) * 3)
        padded = []
        while len(padded) < N:
            p = wide.draw_one(shape)
            if any(a or b for a, b in p["padding"]):
                padded.append(p)
        unpadded = narrow.draw(N, shape)
        assert not any(a or b for p in unpadded for a, b in p["padding"])
        rec["mean_window_fraction"] = {k: float(np.mean([np.prod(A.crop_window(p, shape)[1]) / np.prod(shape) for p in ps]))
                                       for k, ps in (("padded", padded), ("unpadded", unpadded))}
        for t in (x, m):
            name = "fp32" if t is x else "uint8"
            add(f"pad_min_{name}", lambda: A.pad_min(t, flags), 2.0 * t.numel() * t.element_size())
        for label, aug, ps in (("padded", wide, padded), ("unpadded", narrow, unpadded)):
            table, pads = aug._tables(ps, shape, dev)
            ws_x = A.pad_min(x, flags) if any(pads) else None
            ws_m = A.pad_min(m, flags) if any(pads) else None
            add(f"crop_resample_fp32_linear_{label}", lambda: A.crop_resample(x, table, flags, True, ws_x, y), 8.0 * x.numel())
            add(f"crop_resample_fp32_nearest_{label}", lambda: A.crop_resample(x, table, flags, False, ws_x, y), 8.0 * x.numel())
            add(f"crop_resample_uint8_nearest_{label}", lambda: A.crop_resample(m, table, flags, False, ws_m, ym), 2.0 * m.numel())
        add("row_mean_std", lambda: A.row_mean_std(x, 1, flags), 8.0 * x.numel())
        ms = A.row_mean_std(x, 1, flags)
        add("intensity_map_standardize", lambda: A._intensity_map(x, A.MAP_STANDARDIZE, None, None, ms, False, flags, 1, y),
            8.0 * x.numel())
        add("StandarizeChannel_pair", lambda: A.StandarizeChannel(0)._launch(x, None, flags, y), 8.0 * x.numel())
        result["shapes"][spec] = rec
        del x, y, m, ym
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
