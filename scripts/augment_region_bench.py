"""Times the launches behind the slab projections, region masks and axis moves (dram_aug_slab_project per axis and thickness,
dram_aug_keep_region for DiskMaskOut and RandomCubeMask on fp32 and uint8, dram_aug_permute_flip for RandomMoveAxis and
RandomRotateInplane90) against the copy rate measured in the same process, as scripts/augment_intensity_bench.py times the
intensity maps.

    python scripts/augment_region_bench.py [--out FILE] [--shapes 64x128,10x80] [--reps 10]

HIP events around the launches on the launch stream, one warm-up, median and minimum of --reps.  A launch's traffic is counted
as one read plus one write of the tensor (8 bytes per fp32 voxel, 2 per uint8 voxel).  A 10 x 80^3 batch (20 MB) fits the 256 MB
Infinity Cache, so its rates are cache rates, not HBM rates.  Prints one JSON line.
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
        raise SystemExit("augment_region_bench: needs a GPU (times measured anywhere else say nothing)")
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

        def add(label, fn, tensor):
            nbytes = 2.0 * tensor.numel() * tensor.element_size()
            ideal_ms = nbytes / (copy_tbs * 1e12) * 1e3
            r = timed(fn)
            r["one_read_one_write_at_copy_rate_ms"] = ideal_ms
            r["fraction_of_copy_rate"] = ideal_ms / r["ms_median"]
            r["tbs"] = nbytes / (r["ms_median"] * 1e-3) / 1e12
            rec["launches"][label] = r

        y, ym = torch.empty_like(x), torch.empty_like(m)
        for axis in (0, 1, 2):
            for t in (3, 9):
                tables = A.MaximumIntensityProjection()._tables([{"slab_thickness": t, "angle": axis}] * N, shape, dev)
                add(f"slab_project_max_axis{axis}_t{t}", lambda: A.slab_project(x, tables[0], tables[1], True, flags, y), x)
        tables = A.MinimalIntensityProjection()._tables([{"slab_thickness": 9, "angle": 2}] * N, shape, dev)
        add("slab_project_min_axis2_t9", lambda: A.slab_project(x, tables[0], tables[1], False, flags, y), x)
        for label, t in (("DiskMaskOut", A.DiskMaskOut()), ("RandomCubeMask", A.RandomCubeMask((0.2,) * 3, (0.5,) * 3))):
            tables = t._tables(t.draw(N, shape), shape, dev)
            add(f"keep_region_{label}_fp32", lambda: A.keep_region(x, tables[0], tables[1], flags, y), x)
            add(f"keep_region_{label}_uint8", lambda: A.keep_region(m, tables[0], tables[1], flags, ym), m)
        for label, t, p in (("RandomMoveAxis_-1_-2", A.RandomMoveAxis(3), {"sampled_comb": (-1, -2)}),
                            ("RandomMoveAxis_-1_-3", A.RandomMoveAxis(3), {"sampled_comb": (-1, -3)}),
                            ("RandomMoveAxis_-2_-3", A.RandomMoveAxis(3), {"sampled_comb": (-2, -3)}),
                            ("RandomRotateInplane90_1", A.RandomRotateInplane90(3), {"rotate_times": 1}),
                            ("RandomRotateInplane90_2", A.RandomRotateInplane90(3), {"rotate_times": 2})):
            tables = t._tables([p] * N, shape, dev)
            add(f"permute_flip_{label}_fp32", lambda: A._permute_flip(x, tables[0], tables[1], flags, y), x)
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
