"""Times the device chunk loader (dram_amd/preprocess.py, csrc/prep.hip) against the box's measured copy rate, and the same work
done the reference's way: the oracle's numpy restatements on the host, one chunk at a time.

    python scripts/preprocess_bench.py [--out FILE] [--shapes 64x128,10x80] [--reps 10]

Chunks: synthetic, ragged, every axis drawn from 150..220 voxels, int16 HU with an ellipsoid lobe and a random vessel mask.
Device times: HIP events around the launches on the launch stream, one warm-up per shape, median and minimum of --reps.  Bytes
moved are counted from the shapes: every source array read once (2 + 1 bytes per source voxel for the histogram; 2 + 1 + 1 for
the prepare launch with vessels) plus the outputs written (4 x 4 bytes per output voxel); the prepare launch gathers, so what
it really fetches is at most that.  Rates are given as a fraction of the copy rate measured in the same process the way
bench.py measures `ceilings_measured.hbm_copy_tbs`.  The 10-chunk batch's sources (~100 MB) fit the 256 MB Infinity Cache, so
its rates are cache rates.  The pack (host copies into pinned buffers + upload) is timed with a host clock.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "bodyct-dram_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

WINDOW, PSEUDO_WINDOW, PSEUDO_SCALER = (-1000, -300), (-1150, 350), 0.75


def make_chunks(n, seed):
    rng = np.random.default_rng(seed)
    chunks = []
    for _ in range(n):
        shape = tuple(int(v) for v in rng.integers(150, 221, 3))
        scan = rng.normal(-700, 300, size=shape).clip(-2048, 1500).astype(np.int16)
        grid = np.meshgrid(*[np.arange(s, dtype=np.float32) for s in shape], indexing="ij", sparse=True)
        lobe = (sum(((g - (s - 1) / 2) / (0.45 * s)) ** 2 for g, s in zip(grid, shape)) < 1.0).astype(np.uint8)
        vessel = (rng.random(shape, dtype=np.float32) > 0.9).astype(np.uint8)
        chunks.append({"#image": scan, "#lobe_reference": lobe, "#vessel_reference": vessel,
                       "meta": {"spacing": tuple(float(v) for v in rng.uniform(0.6, 1.4, 3))}})
    return chunks


def host_one(chunk, size):
    """One chunk the reference's way (dataset.py:460-463, Windowing, Resample('fixed_size')) with the oracle's restatements."""
    from dram_amd.preprocess import resample_plan
    from oracle import dram_oracle as O
    scan, lobe, spacing = chunk["#image"], chunk["#lobe_reference"], chunk["meta"]["spacing"]
    w_scan = O.windowing(scan, from_span=PSEUDO_WINDOW, to_span=(0, 1))
    _, th = O.binary_cam(w_scan[lobe > 0], PSEUDO_SCALER)
    lesion = ((w_scan > th) & (lobe > 0)).astype(np.uint8)
    vessel = np.logical_and(chunk["#vessel_reference"] > 0, lobe > 0).astype(np.uint8)
    image = O.windowing(scan.astype(np.float32), from_span=WINDOW, to_span=(0, 1))
    req, new_size = resample_plan("fixed_size", None, (size,) * 3, np.asarray(spacing), scan.shape)
    out = [O.resample_itk(image, spacing, req, new_size, "linear")]
    out += [O.resample_itk(m, spacing, req, new_size, "nearest").astype(np.float32) for m in (lobe, lesion, vessel)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="64x128,10x80")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-serial-chunks", type=int, default=2, help="chunks timed on one thread (scaled to the batch)")
    ap.add_argument("--host-pool-chunks", type=int, default=16, help="chunks timed on the thread pool (scaled to the batch)")
    args = ap.parse_args()
    import torch
    from dram_amd import _lib
    from dram_amd.preprocess import ChunkLoader
    if not torch.cuda.is_available():
        raise SystemExit("preprocess_bench: needs a GPU (times measured anywhere else say nothing)")
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
        chunks = make_chunks(N, seed=N)
        loader = ChunkLoader(size, WINDOW, PSEUDO_WINDOW, PSEUDO_SCALER)
        t0 = time.perf_counter()
        packed = loader.pack(chunks)
        torch.cuda.synchronize()
        pack_first_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        packed = loader.pack(chunks)
        torch.cuda.synchronize()
        pack_ms = (time.perf_counter() - t0) * 1e3
        src_vox, out_vox = packed.scans.numel(), N * size ** 3
        rec = {"source_voxels": src_vox, "output_voxels": out_vox, "pack_and_upload_ms": pack_ms,
               "pack_and_upload_first_ms": pack_first_ms, "entry_points": {}}
        hist = torch.empty((N, 256), dtype=torch.int64, device=dev)
        th = torch.empty(N, dtype=torch.float64, device=dev)
        outs = [torch.empty((N, 1, size, size, size), dtype=torch.float32, device=dev) for _ in range(4)]
        s, l, v, t = (x.data_ptr() for x in (packed.d_scans, packed.d_lobes, packed.d_vessels, packed.d_table))

        def note(name, r, nbytes):
            ideal = nbytes / (copy_tbs * 1e12) * 1e3
            r.update(bytes=nbytes, at_copy_rate_ms=ideal, fraction_of_copy_rate=ideal / r["ms_median"],
                     tbs=nbytes / (r["ms_median"] * 1e-3) / 1e12)
            rec["entry_points"][name] = r

        note("dram_chunk_hist256", timed(lambda: _lib.call("dram_chunk_hist256", s, l, t, N, hist.data_ptr(), *PSEUDO_WINDOW, st)),
             3.0 * src_vox + N * 2048)
        note("dram_otsu256", timed(lambda: _lib.call("dram_otsu256", hist.data_ptr(), N, PSEUDO_SCALER, th.data_ptr(), st)),
             N * 2048 + N * 8)
        prep = lambda ves: _lib.call("dram_chunk_prepare", s, l, v if ves else None, t, th.data_ptr(), N, size, size, size,
                                     float(WINDOW[0]), float(WINDOW[1]), *PSEUDO_WINDOW, outs[0].data_ptr(), outs[1].data_ptr(),
                                     outs[2].data_ptr(), outs[3].data_ptr() if ves else None, st)
        note("dram_chunk_prepare", timed(lambda: prep(True)), 4.0 * src_vox + 16.0 * out_vox)
        note("dram_chunk_prepare_no_vessel", timed(lambda: prep(False)), 3.0 * src_vox + 12.0 * out_vox)
        del outs
        note("ChunkLoader.__call__", timed(lambda: loader(packed)), 7.0 * src_vox + 16.0 * out_vox + 2 * N * 2048)
        # the reference's way, on the same chunks
        k1 = min(N, args.host_serial_chunks)
        t0 = time.perf_counter()
        for c in chunks[:k1]:
            host_one(c, size)
        serial_s = time.perf_counter() - t0
        threads = min(16, os.cpu_count() or 1)
        kp = min(N, args.host_pool_chunks)
        t0 = time.perf_counter()
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(lambda c: host_one(c, size), chunks[:kp]))
        pool_s = time.perf_counter() - t0
        rec["host"] = {"one_thread_ms_per_chunk": serial_s / k1 * 1e3, "one_thread_ms_batch_extrapolated": serial_s / k1 * N * 1e3,
                       "threads": threads, "threads_chunks_timed": kp, "threads_ms_batch_extrapolated": pool_s / kp * N * 1e3,
                       "how": "oracle.windowing / binary_cam / resample_itk composed as the reference composes them, one chunk "
                              "at a time (numpy; the reference itself calls SimpleITK and skimage, absent here)"}
        result["shapes"][spec] = rec
        del packed, hist, th
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
