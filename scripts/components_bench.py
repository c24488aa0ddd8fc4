"""Times the lesion-wise report kernels (csrc/components.hip) on the lesion mask of inference.synthetic_ct() at 300x512x512 --
its lesions thresholded directly, no model -- against the copy rate measured in the same process and against
scipy.ndimage.label on the host.

    python scripts/components_bench.py [--out FILE] [--shape 300,512,512] [--reps 10] [--no-scipy]

Timed: dram_cc_label at connectivity 1 and 3, dram_cc_stats (with the `other` mask), dram_lobe_burden.  HIP events around each
call on the launch stream, one warm-up, median and minimum of --reps.  Floors are the bytes a call must at least move, at the
copy rate: labelling 1 byte read + 4 written per voxel, the statistics 5 bytes read, the burden 2 bytes read.  The six launches
of dram_cc_label are one call here; their split comes from a kernel trace of this script (rocprofv3 --kernel-trace --stats --
python scripts/components_bench.py --reps 3 --no-scipy), in a run of its own.  scipy runs once per connectivity on at most 16
host threads (it uses one); where scipy does not import the figure is null.  Prints a table, then one JSON line.
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
    if not torch.cuda.is_available():
        raise SystemExit("components_bench: needs a GPU (times measured anywhere else say nothing)")
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
    mask = ((scan > -575) & (lobe > 0)).astype(np.uint8)        # between the parenchyma (-850 +- 60) and the lesions (-300 +- 80)
    D, H, W = shape
    nvox = mask.size
    mask_d, lobe_d = torch.from_numpy(mask).to(dev), torch.from_numpy(lobe).to(dev)
    labels = torch.empty(shape, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    ws_bytes = _lib.lib.dram_cc_ws_bytes(D, H, W)
    ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=dev)
    result = {"device": torch.cuda.get_device_name(0), "shape": list(shape), "set_voxels": int(mask.sum()), "hbm_copy_tbs": copy_tbs,
              "calls": {}}

    def floor_ms(bytes_per_voxel):
        return bytes_per_voxel * nvox / (copy_tbs * 1e12) * 1e3

    def record(name, t, bytes_per_voxel, scipy_s=None):
        t.update(floor_ms=floor_ms(bytes_per_voxel), over_floor=t["ms_median"] / floor_ms(bytes_per_voxel), scipy_s=scipy_s,
                 scipy_over_gpu=None if scipy_s is None else scipy_s * 1e3 / t["ms_median"])
        result["calls"][name] = t

    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    if args.no_scipy:
        ndimage = None
    for c in (1, 3):
        label = lambda: _lib.call("dram_cc_label", mask_d.data_ptr(), labels.data_ptr(), count.data_ptr(), c, D, H, W, ws.data_ptr(),
                                  ws_bytes, st)
        t = timed(label)
        t["components"] = int(count.item())
        scipy_s = None
        if ndimage is not None:
            t0 = time.perf_counter()
            ref, n_ref = ndimage.label(mask, structure=ndimage.generate_binary_structure(3, c))
            scipy_s = time.perf_counter() - t0
            t["equal_to_scipy"] = bool(n_ref == t["components"] and np.array_equal(labels.cpu().numpy(), ref))
            del ref
        record(f"cc_label_c{c}", t, 5, scipy_s)
    n_comp = result["calls"]["cc_label_c3"]["components"]
    voxels = torch.empty(n_comp, dtype=torch.int64, device=dev)
    hits = torch.empty(n_comp, dtype=torch.int64, device=dev)
    bbox = torch.empty((n_comp, 6), dtype=torch.int32, device=dev)
    record("cc_stats", timed(lambda: _lib.call("dram_cc_stats", labels.data_ptr(), mask_d.data_ptr(), n_comp, voxels.data_ptr(),
                                               bbox.data_ptr(), hits.data_ptr(), D, H, W, st)), 5)
    assert int(voxels.sum()) == result["set_voxels"] and torch.equal(voxels, hits)
    counts = torch.empty((256, 2), dtype=torch.int64, device=dev)
    record("lobe_burden", timed(lambda: _lib.call("dram_lobe_burden", mask_d.data_ptr(), lobe_d.data_ptr(), counts.data_ptr(), nvox, st)), 2)
    assert int(counts[:, 0].sum()) == nvox and int(counts[:, 1].sum()) == result["set_voxels"]

    print(f"{result['device']}: {shape}, {result['set_voxels']} set voxels, copy rate {copy_tbs:.2f} TB/s")
    for name, t in result["calls"].items():
        extra = "" if t["scipy_s"] is None else f", scipy {t['scipy_s']:.2f} s = {t['scipy_over_gpu']:.0f} x"
        print(f"  {name:14s} median {t['ms_median']:8.3f} ms (min {t['ms_min']:.3f}), floor {t['floor_ms']:.3f} ms, "
              f"{t['over_floor']:.1f} x the floor{extra}" + (f", {t['components']} components" if "components" in t else ""))
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
