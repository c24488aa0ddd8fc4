"""Times the surface-distance kernels (csrc/distance.hip) on the lesion mask of inference.synthetic_ct() at 300x512x512 -- its
lesions thresholded directly, no model -- against the copy rate measured in the same process and against
scipy.ndimage.distance_transform_edt on the host.

    python scripts/surface_bench.py [--out FILE] [--shape 300,512,512] [--reps 10] [--no-scipy]

Timed: dram_mask_surface on the mask, dram_edt on that surface (what surface_distances feeds it), dram_surface_gather of the
result over the surface of the mask moved by (1, 2, 3) voxels, and dram_amd.surface_distances of the mask against the moved mask
as a whole (host clock around the call, which ends in a read-back; it includes the two torch sorts).  HIP events around each
call on the launch stream, one warm-up, median and minimum of --reps.  Floors are the bytes a call must at least move, at the
copy rate: the surface 1 byte read + 1 written per voxel, the transform 1 read + 4 written, the gather 1 read (the few surface
voxels not counted).  The three passes of dram_edt are one call here; their split comes from a kernel trace of this script
(rocprofv3 --kernel-trace --stats -- python scripts/surface_bench.py --reps 3 --no-scipy), in a run of its own: edt_x_kernel,
edt_axis_kernel<int, double> (y) and edt_axis_kernel<double, float> (z).  scipy runs once on at most 16 host threads (it uses
one); where scipy does not import the figure is null.  Prints a table, then one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "bodyct-dram_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", default="300,512,512")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-scipy", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from dram_amd import _lib
    from dram_amd.inference import synthetic_ct
    from dram_amd.surface import surface_distances
    if not torch.cuda.is_available():
        raise SystemExit("surface_bench: needs a GPU (times measured anywhere else say nothing)")
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    dev = torch.device("cuda")
    st = torch.cuda.current_stream().cuda_stream
    shape = tuple(int(v) for v in args.shape.split(","))

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

    scan, lobe, spacing = synthetic_ct(shape)
    spacing = [float(s) for s in spacing]
    mask = ((scan > -575) & (lobe > 0)).astype(np.uint8)        # between the parenchyma (-850 +- 60) and the lesions (-300 +- 80)
    moved = np.roll(mask, (1, 2, 3), axis=(0, 1, 2))
    D, H, W = shape
    nvox = mask.size
    mask_d, moved_d = torch.from_numpy(mask).to(dev), torch.from_numpy(moved).to(dev)
    surf, surf_moved = torch.empty_like(mask_d), torch.empty_like(mask_d)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    dist = torch.empty(shape, dtype=torch.float32, device=dev)
    ws_bytes = _lib.lib.dram_edt_ws_bytes(D, H, W)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    result = {"device": torch.cuda.get_device_name(0), "shape": list(shape), "spacing": spacing, "set_voxels": int(mask.sum()),
              "hbm_copy_tbs": copy_tbs, "edt_ws_bytes": ws_bytes, "calls": {}}

    def floor_ms(bytes_per_voxel):
        return bytes_per_voxel * nvox / (copy_tbs * 1e12) * 1e3

    def record(name, t, bytes_per_voxel, scipy_s=None):
        t.update(floor_ms=floor_ms(bytes_per_voxel), over_floor=t["ms_median"] / floor_ms(bytes_per_voxel), scipy_s=scipy_s,
                 scipy_over_gpu=None if scipy_s is None else scipy_s * 1e3 / t["ms_median"])
        result["calls"][name] = t

    _lib.call("dram_mask_surface", moved_d.data_ptr(), surf_moved.data_ptr(), count.data_ptr(), D, H, W, st)
    n_moved = int(count.item())
    record("mask_surface", timed(lambda: _lib.call("dram_mask_surface", mask_d.data_ptr(), surf.data_ptr(), count.data_ptr(), D, H, W,
                                                   st)), 2)
    result["surface_voxels"] = int(count.item())

    t = timed(lambda: _lib.call("dram_edt", surf.data_ptr(), dist.data_ptr(), *spacing, D, H, W, ws.data_ptr(), ws_bytes, st))
    scipy_s = None
    if not args.no_scipy:
        try:
            from scipy import ndimage
        except ImportError:
            ndimage = None
        if ndimage is not None:
            feature = surf.cpu().numpy()
            t0 = time.perf_counter()
            ref = ndimage.distance_transform_edt(feature == 0, sampling=spacing)
            scipy_s = time.perf_counter() - t0
            got = dist.cpu().numpy().astype(np.float64)
            t["max_rel_diff_to_scipy"] = float(np.max(np.abs(got - ref) / np.maximum(ref, 1e-300)))     # float32 against fp64
            del ref, got, feature
    record("edt", t, 5, scipy_s)

    out = torch.empty(n_moved, dtype=torch.float32, device=dev)
    cursor = torch.empty(1, dtype=torch.int64, device=dev)
    record("surface_gather", timed(lambda: _lib.call("dram_surface_gather", surf_moved.data_ptr(), dist.data_ptr(), out.data_ptr(),
                                                     cursor.data_ptr(), n_moved, nvox, st)), 1)
    assert int(cursor.item()) == n_moved

    def whole():
        result["metrics"] = surface_distances(mask_d, moved_d, spacing, tolerances_mm=(1.0, 2.0))
    whole()
    torch.cuda.synchronize()
    s = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        whole()
        s.append((time.perf_counter() - t0) * 1e3)
    record("surface_distances", {"ms_median": statistics.median(s), "ms_min": min(s), "ms_max": max(s)}, 2 * (2 + 5 + 1))

    print(f"{result['device']}: {shape}, {result['set_voxels']} set voxels, {result['surface_voxels']} on the surface, "
          f"copy rate {copy_tbs:.2f} TB/s")
    for name, t in result["calls"].items():
        extra = "" if t["scipy_s"] is None else f", scipy {t['scipy_s']:.2f} s = {t['scipy_over_gpu']:.0f} x"
        print(f"  {name:18s} median {t['ms_median']:8.3f} ms (min {t['ms_min']:.3f}), floor {t['floor_ms']:.3f} ms, "
              f"{t['over_floor']:.1f} x the floor{extra}")
    print(f"  metrics: {result['metrics']}")
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
