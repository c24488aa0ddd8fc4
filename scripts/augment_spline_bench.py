"""Times the launches behind RandomAffineTransform3D and RandomRotate (dram_aug_spline_prefilter along three and along two axes,
dram_aug_spline_resample for order 3 in 3-d and in a plane and for order 0 on fp32 and uint8, dram_aug_minmax_u8) against the copy
rate measured in the same process, as scripts/augment_crop_bench.py times RandomCrop, and against scipy on the host.

    python scripts/augment_spline_bench.py [--out FILE] [--shapes 64x128,10x80] [--reps 10]

HIP events around the launches on the launch stream, one warm-up, median and minimum of --reps.  Counted bytes: the prefilter
as one fp32 read plus one fp64 write of the tensor (12 bytes per voxel; it really makes three passes per filtered axis over
the fp64 workspace), an order-3 gather as one fp64 read plus one fp32 write (12 bytes per voxel; it really fetches 64 or 16
coefficients per voxel through the caches), an order-0 gather as one read plus one write.  A 10 x 80^3 batch (20 MB, 41 MB of
coefficients) fits the 256 MB Infinity Cache, so its rates are cache rates, not HBM rates.  The host figure is
scipy.ndimage.affine_transform / rotate on ONE chunk of the shape with the first sample's parameters, times the batch size.
Prints one JSON line.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

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
    from scipy import ndimage
    from dram_amd import _lib
    from dram_amd import augment as A
    if not torch.cuda.is_available():
        raise SystemExit("augment_spline_bench: needs a GPU (times measured anywhere else say nothing)")
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
        host = np.random.default_rng(0).random((N,) + shape, dtype=np.float32)
        x = torch.from_numpy(host).to(dev).unsqueeze(1)
        m = (x * 5).to(torch.uint8)
        flags = torch.ones(N, dtype=torch.int32, device=dev)
        rec = {"voxels": x.numel(), "launches": {}, "host_scipy": {}}

        def add(label, fn, nbytes):
            ideal_ms = nbytes / (copy_tbs * 1e12) * 1e3
            r = timed(fn)
            r["counted_bytes_at_copy_rate_ms"] = ideal_ms
            r["fraction_of_copy_rate"] = ideal_ms / r["ms_median"]
            r["tbs"] = nbytes / (r["ms_median"] * 1e-3) / 1e12
            rec["launches"][label] = r

        np.random.seed(0)
        random.seed(0)
        affine, rotate = A.RandomAffineTransform3D(3), A.RandomRotate(3, (-20, 20))
        pa, pr = affine.draw(N, shape), rotate.draw(N, shape)
        ta, tr = affine._tables(pa, shape, dev), rotate._tables(pr, shape, dev)
        y, ym = torch.empty_like(x), torch.empty_like(m)
        mm, mm8 = A.sample_min_table(x, flags), A.sample_min_table(m, flags)
        add("minmax_u8", lambda: A.sample_min_table(m, flags), 1.0 * m.numel())
        add("prefilter_zyx", lambda: A.spline_prefilter(x, ta[1], flags), 12.0 * x.numel())
        add("prefilter_plane", lambda: A.spline_prefilter(x, tr[1], flags), 12.0 * x.numel())
        coef = A.spline_prefilter(x, ta[1], flags)
        add("resample_order3_affine", lambda: A.spline_resample(x, ta[0], mm, flags, 3, coef, y), 12.0 * x.numel())
        add("resample_order0_fp32_affine", lambda: A.spline_resample(x, ta[0], mm, flags, 0, None, y), 8.0 * x.numel())
        add("resample_order0_uint8_affine", lambda: A.spline_resample(m, ta[0], mm8, flags, 0, None, ym), 2.0 * m.numel())
        coef = A.spline_prefilter(x, tr[1], flags)
        add("resample_order3_rotate", lambda: A.spline_resample(x, tr[0], mm, flags, 3, coef, y), 12.0 * x.numel())
        add("resample_order0_uint8_rotate", lambda: A.spline_resample(m, tr[0], mm8, flags, 0, None, ym), 2.0 * m.numel())
        del coef
        add("RandomAffineTransform3D_image", lambda: affine._launch_key("#image", x, ta, flags, y), 20.0 * x.numel())
        add("RandomRotate_image", lambda: rotate._launch_key("#image", x, tr, flags, y), 20.0 * x.numel())

        a = host[0]
        mat, off = A.affine_matrix(pa[0]["scales"], pa[0]["rotate_angles"], shape)
        t0 = time.perf_counter()
        ndimage.affine_transform(a, mat, offset=off, output_shape=a.shape, mode="constant", order=3, cval=a.min())
        t1 = time.perf_counter()
        ndimage.rotate(a, pr[0]["rotate_angle"], reshape=False, axes=pr[0]["rotate_axis"], order=3, mode="constant", cval=a.min())
        t2 = time.perf_counter()
        for label, sec, dev_label in (("affine_order3", t1 - t0, "RandomAffineTransform3D_image"),
                                      ("rotate_order3", t2 - t1, "RandomRotate_image")):
            rec["host_scipy"][label] = {"ms_per_chunk": sec * 1e3, "ms_batch": sec * 1e3 * N,
                                        "device_speedup": sec * 1e3 * N / rec["launches"][dev_label]["ms_median"]}
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
