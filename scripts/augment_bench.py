"""Times the batched augmentation pool (dram_amd/augment.py) against the box's measured copy rate, and the same work done the
reference's way: numpy / scipy on the host, one chunk at a time, followed by the host-to-device copy.

    python scripts/augment_bench.py [--out FILE] [--shapes 64x128,10x80] [--reps 10]

Device times: HIP events around the launches on the launch stream, one warm-up, median and minimum of --reps.  A transform's
traffic is counted as one read plus one write of the tensor (8 bytes per voxel; mask-out and noise read it once more for their
min / max pre-pass, reported separately), and its rate is given as a fraction of the copy rate measured in the same process
the way bench.py measures `ceilings_measured.hbm_copy_tbs`.  A 10 x 80^3 batch (20 MB) fits the 256 MB Infinity Cache, so its
rates are cache rates, not HBM rates.  Prints one JSON line.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "bodyct-dram_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


# ------------------------------------------------------------------------------------------------ the host restatement
def host_chain(chunk, names, rng_seed):
    """The five pool elements in numpy / scipy on one chunk, with the pool's parameter ranges (written for this script)."""
    from scipy import ndimage
    rng = np.random.RandomState(rng_seed)
    x = chunk
    for name in names:
        if name == "GaussianBlur":
            x = ndimage.gaussian_filter(x.astype(np.float32), rng.uniform(0.3, 0.5))
        elif name == "RandomMaskOut":
            lo, hi, y = x.min(), x.max(), x.copy()
            for _ in range(5):
                c = [int(d * rng.uniform(0.2, 0.8)) for d in x.shape]
                s = [int(rng.uniform(0.01, 0.05) * d) for d in x.shape]
                y[tuple(slice(max(0, ci - si // 2), min(ci + (si - si // 2), d)) for ci, si, d in zip(c, s, x.shape))] = \
                    rng.uniform(lo, hi)
            x = y
        elif name == "RandomFlip":
            x = np.flip(x, axis=-1 - rng.randint(3)).copy()
        elif name == "RandomRotate90":
            axes = [(-1, -2), (-1, -3), (-2, -3)][rng.randint(3)]
            x = np.rot90(x, k=rng.randint(4), axes=axes).copy()
        else:
            sigma = rng.uniform(0.01, 0.02)
            lo, hi = x.min(), x.max()
            r = (x.astype(np.float32) - lo) / float(hi - lo + np.float32(1e-7))
            r += rng.normal(0, sigma, size=x.shape)
            np.clip(r, 0.0, 1.0, out=r)
            x = r * (hi - lo) + lo
    return np.ascontiguousarray(x, dtype=np.float32)


POOL = ["GaussianBlur", "RandomMaskOut", "RandomFlip", "RandomRotate90", "GaussianAddictive"]


def time_host(images, chains, threads):
    t0 = time.perf_counter()
    if threads == 1:
        out = [host_chain(images[i], chains[i], i) for i in range(len(chains))]
    else:
        with ThreadPoolExecutor(threads) as ex:
            out = list(ex.map(lambda i: host_chain(images[i], chains[i], i), range(len(chains))))
    return time.perf_counter() - t0, out


# --------------------------------------------------------------------------------------------------------------- device
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="64x128,10x80")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-serial-chunks", type=int, default=8, help="chunks timed on one thread (scaled to the batch)")
    args = ap.parse_args()
    import torch
    from dram_amd import _lib
    from dram_amd import augment as A
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench: needs a GPU (times measured anywhere else say nothing)")
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
        host_images = np.random.default_rng(0).random((N,) + shape, dtype=np.float32)
        x = torch.from_numpy(host_images).to(dev).unsqueeze(1)
        nbytes = 2.0 * x.numel() * 4
        ideal_ms = nbytes / (copy_tbs * 1e12) * 1e3
        rec = {"voxels": x.numel(), "one_read_one_write_at_copy_rate_ms": ideal_ms, "transforms": {}}
        ens = A.EnsembleScanAugmentation(1.0)
        flags = torch.ones(N, dtype=torch.int32, device=dev)
        y = torch.empty_like(x)
        mm = A.sample_minmax(x)
        rec["transforms"]["minmax_prepass"] = dict(timed(lambda: A.sample_minmax(x, out=mm)), bytes_per_voxel=4)
        for t in ens.transform_pool:
            tables = t._tables(t.draw(N, shape), shape, dev)
            if isinstance(t, (A.RandomMaskOut, A.GaussianAddictive)):
                r = timed(lambda: t._launch(x, tables, flags, out=y, minmax=mm))       # the kernel alone
                r["with_minmax_ms_median"] = timed(lambda: t._launch(x, tables, flags, out=y))["ms_median"]
            else:
                r = timed(lambda: t._launch(x, tables, flags, out=y))
            r["fraction_of_copy_rate"] = ideal_ms / r["ms_median"]
            r["tbs"] = nbytes / (r["ms_median"] * 1e-3) / 1e12
            rec["transforms"][type(t).__name__] = r
        sample = {"#image": x}
        chains = ens.draw(N, shape)
        r = timed(lambda: ens.apply(sample, chains), max(3, args.reps // 2))          # table uploads included
        r["fraction_of_copy_rate_5_transforms"] = 5 * ideal_ms / r["ms_median"]
        t0 = time.perf_counter()
        for _ in range(3):
            ens.apply(sample, ens.draw(N, shape))
        torch.cuda.synchronize()
        r["wall_ms_with_draws"] = (time.perf_counter() - t0) / 3 * 1e3
        rec["ensemble_ratio_1"] = r
        del y
        # the reference's way
        names = A.EnsembleScanAugmentation.chain_names(chains)
        k = min(N, args.host_serial_chunks)
        serial_s, _ = time_host(host_images, names[:k], 1)
        threads = min(16, os.cpu_count() or 1)
        pool_s, out = time_host(host_images, names, threads)
        stacked = np.stack(out)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        torch.from_numpy(stacked).to(dev)
        torch.cuda.synchronize()
        h2d_s = time.perf_counter() - t0
        rec["host"] = {"one_thread_ms_per_chunk": serial_s / k * 1e3, "one_thread_ms_batch_extrapolated": serial_s / k * N * 1e3,
                       "threads": threads, "threads_ms_batch": pool_s * 1e3, "h2d_copy_ms": h2d_s * 1e3,
                       "how": "numpy/scipy restatement of the pool, one chunk at a time, all five transforms per chunk in the "
                              "order the device run drew; pageable host-to-device copy of the finished batch"}
        result["shapes"][spec] = rec
        del x, sample
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
