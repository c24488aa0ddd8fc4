"""Times the pseudo-vessel mask (csrc/vessel.hip, dram_amd/vessels.py) on the scan of inference.synthetic_ct() at 300x512x512,
spacing (1.0, 0.7, 0.7), default scales (1, 1.5, 2, 3 mm), against the copy rate measured in the same process and against
the fp64 scipy restatement (tests/vessel_restatement.py) on the host.

    python scripts/vessel_bench.py [--out FILE] [--shape 300,512,512] [--reps 10] [--scipy-depth 24]

Timed per scale: dram_hessian (x, y and z passes in one call), dram_hessian_norm_max, dram_vesselness; once: dram_vessel_mask;
and dram_amd.pseudo_vessel_mask as a whole (host clock around the call; it ends in no read-back, so a synchronise closes it;
it includes the bounding-box read-back, the crop copies and the allocations, and works on the lobes' bounding box only, so
its floor is taken over the box).  HIP events around each call on the launch stream, one warm-up, median and minimum of
--reps.  Floors are the bytes a call must at least move, at the copy rate, with every intermediate materialised as the
kernels do: Hessian 2 in + 12 out (x), 12 + 24 (y), 24 + 24 (z) = 98 B per voxel; norm maximum 24 (+ 1 lobe; it skips the
Hessian of voxels outside the lobes, so it can fall below that); vesselness 24 in + 4 in + 4 out; mask 4 + 1 + 1.  The split of
dram_hessian into its passes comes from a kernel trace of this script in a run of its own (rocprofv3 --kernel-trace --stats --
python scripts/vessel_bench.py --reps 3 --scipy-depth 0).  The restatement runs once, on the first --scipy-depth slices only
(all four scales, c given): at full depth its fp64 intermediates need tens of GB; the figure is seconds per voxel, and the
whole-scan time printed beside it is that rate times the voxel count, an extrapolation.  0 skips it.  Prints a table, then one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "bodyct-dram_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", default="300,512,512")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scipy-depth", type=int, default=24)
    args = ap.parse_args()
    import numpy as np
    import torch
    from dram_amd import _lib, vessels
    from dram_amd.inference import synthetic_ct
    if not torch.cuda.is_available():
        raise SystemExit("vessel_bench: needs a GPU (times measured anywhere else say nothing)")
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

    scan, lobe, spacing = synthetic_ct(shape, (1.0, 0.7, 0.7))
    spacing = [float(s) for s in spacing]
    sigmas = vessels.DEFAULT_SIGMAS_MM
    D, H, W = shape
    S = D * H * W
    scan_d, lobe_d = torch.from_numpy(scan).to(dev), torch.from_numpy(lobe).to(dev)
    h6 = torch.empty((6, D, H, W), dtype=torch.float32, device=dev)
    ws = torch.empty(_lib.lib.dram_hessian_ws_bytes(D, H, W) // 4, dtype=torch.float32, device=dev)
    vmax = torch.zeros(shape, dtype=torch.float32, device=dev)
    mask = torch.empty(shape, dtype=torch.uint8, device=dev)
    c_dev = torch.ones(1, dtype=torch.float32, device=dev)
    result = {"device": torch.cuda.get_device_name(0), "shape": list(shape), "spacing": spacing, "sigmas_mm": list(sigmas),
              "hbm_copy_tbs": copy_tbs, "lobe_voxels": int((lobe > 0).sum()), "calls": {}}

    def record(name, t, bytes_per_voxel, nvox=S):
        floor = bytes_per_voxel * nvox / (copy_tbs * 1e12) * 1e3
        t.update(floor_ms=floor, over_floor=t["ms_median"] / floor)
        result["calls"][name] = t

    clip = vessels.DEFAULT_CLIP
    for k, s in enumerate(sigmas):
        tables = vessels._scale_tables(spacing, s, "vessel_bench")
        record(f"hessian {s} mm (radius {tables[1]})", timed(lambda: vessels._hessian_into(scan_d, tables, clip, h6, ws)), 98)
        record(f"hessian_norm_max {s} mm", timed(lambda: _lib.call("dram_hessian_norm_max", h6.data_ptr(), lobe_d.data_ptr(), S,
                                                                   c_dev.data_ptr(), st)), 25)
        record(f"vesselness {s} mm", timed(lambda: _lib.call("dram_vesselness", h6.data_ptr(), S, 0.5, 0.5, c_dev.data_ptr(),
                                                             vmax.data_ptr(), 1, None, st)), 32)
    record("vessel_mask", timed(lambda: _lib.call("dram_vessel_mask", vmax.data_ptr(), lobe_d.data_ptr(), 0.5, mask.data_ptr(), S, st)), 6)
    del h6, ws
    torch.cuda.empty_cache()

    def whole():
        result["mask_voxels"] = vessels.pseudo_vessel_mask(scan_d, lobe_d, spacing)
        torch.cuda.synchronize()
    whole()
    ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        whole()
        ms.append((time.perf_counter() - t0) * 1e3)
    result["mask_voxels"] = int(result["mask_voxels"].sum().item())
    # the whole call works on the lobes' bounding box grown by the largest radius per axis
    radii = [vessels._scale_tables(spacing, s, "vessel_bench")[1] for s in sigmas]
    box = vessels._lobe_box(lobe_d, [max(r[a] for r in radii) for a in range(3)])
    result["box"] = [b.stop - b.start for b in box]
    record("pseudo_vessel_mask as a whole (on the box)", {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)},
           len(sigmas) * (98 + 25 + 32) + 6, result["box"][0] * result["box"][1] * result["box"][2])

    result["scipy"] = None
    if args.scipy_depth > 0:
        import vessel_restatement as VR
        depth = min(D, args.scipy_depth)
        t0 = time.perf_counter()
        VR.vesselness(scan[:depth], spacing, sigmas, c=100.0)
        per_voxel = (time.perf_counter() - t0) / (depth * H * W)
        result["scipy"] = {"depth": depth, "s_per_voxel": per_voxel, "whole_scan_s_extrapolated": per_voxel * S}

    print(f"{result['device']}: {shape}, {result['lobe_voxels']} lobe voxels, {result['mask_voxels']} in the mask, box {result['box']}, "
          f"copy rate {copy_tbs:.2f} TB/s")
    for name, t in result["calls"].items():
        print(f"  {name:42s} median {t['ms_median']:9.3f} ms (min {t['ms_min']:.3f}), floor {t['floor_ms']:.3f} ms, "
              f"{t['over_floor']:.1f} x the floor")
    if result["scipy"]:
        print(f"  scipy restatement on {result['scipy']['depth']} slices: {result['scipy']['s_per_voxel'] * 1e6:.2f} us per voxel, "
              f"{result['scipy']['whole_scan_s_extrapolated']:.0f} s for the whole scan (extrapolated)")
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
