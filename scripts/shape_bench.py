"""Times the lesion shape kernel (csrc/shape.hip) on the scan of inference.synthetic_ct() at 300x512x512: its lobe map (uint8) and
the components of its lesion mask (int32) -- the lesions thresholded directly, no model -- each with its own n and with n forced
into the other plan, against the copy rate measured in the same process, against dram_label_density without a histogram on the
same labels (a pass that reads the same label bytes once) and, with --host, against the numpy restatement of the tests.

    python scripts/shape_bench.py [--out FILE] [--shape 300,512,512] [--reps 10] [--host]

HIP events around each call on the launch stream, one warm-up, median and minimum of --reps.  The floor is the label bytes at the
copy rate: 1 or 4 bytes per voxel.  With --host every device table is compared with the restatement.  Prints a table, then one
JSON line.
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
    ap.add_argument("--host", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from dram_amd import _lib
    from dram_amd.inference import synthetic_ct
    from dram_amd.lesions import label_components
    if not torch.cuda.is_available():
        raise SystemExit("shape_bench: needs a GPU (times measured anywhere else say nothing)")
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

    scan, lobe, _ = synthetic_ct(shape)
    mask = ((scan > -575) & (lobe > 0)).astype(np.uint8)
    nvox = mask.size
    scan_d, lobe_d, mask_d = torch.from_numpy(scan).to(dev), torch.from_numpy(lobe).to(dev), torch.from_numpy(mask).to(dev)
    labels_d, n_comp = label_components(mask_d, 1)
    n_comp, n_lobe = max(n_comp, 1), int(lobe.max())
    result = {"device": torch.cuda.get_device_name(0), "shape": list(shape), "set_voxels": int(mask.sum()), "components": n_comp,
              "lobes": n_lobe, "hbm_copy_tbs": copy_tbs, "calls": {}}
    calls = result["calls"]

    def record(name, t, bytes_per_voxel, **extra):
        floor = bytes_per_voxel * nvox / (copy_tbs * 1e12) * 1e3
        t.update(floor_ms=floor, over_floor=t["ms_median"] / floor, **extra)
        calls[name] = t

    def shape_call(labels_t, kind, n_lab):
        buf = torch.empty(n_lab * 266, dtype=torch.int64, device=dev)
        t = timed(lambda: _lib.call("dram_label_shape", labels_t.data_ptr(), kind, n_lab, buf[:n_lab * 256].data_ptr(),
                                    buf[n_lab * 256:].data_ptr(), *shape, st))
        t["plan"] = _lib.lib.dram_label_shape_plan(kind, n_lab)
        return t, buf

    def density_call(labels_t, kind, n_lab):
        count, total, sumsq = (torch.empty(n_lab, dtype=torch.int64, device=dev) for _ in range(3))
        vmin, vmax = (torch.empty(n_lab, dtype=torch.int32, device=dev) for _ in range(2))
        t = timed(lambda: _lib.call("dram_label_density", scan_d.data_ptr(), labels_t.data_ptr(), kind, None, n_lab, count.data_ptr(),
                                    total.data_ptr(), sumsq.data_ptr(), vmin.data_ptr(), vmax.data_ptr(), None, -1024, 1, 0, nvox, st))
        t["plan"] = _lib.lib.dram_label_density_plan(kind, n_lab, 0)
        return t

    def other_plan(kind, n_lab):
        """The nearest n at or above n_lab that the wave plan takes (None where the label kind has none)."""
        m = n_lab
        while _lib.lib.dram_label_shape_plan(kind, m) == 0:
            m += 1
        return m if _lib.lib.dram_label_shape_plan(kind, m) == 1 else None

    ratios = {}
    for tag, labels_t, labels_h, kind, n_lab, bpv in (("lobes_u8", lobe_d, lobe, 0, n_lobe, 1), ("components_i32", labels_d, None, 1, n_comp, 4)):
        settings = [(tag, n_lab)]
        m = other_plan(kind, n_lab)
        if m is not None and m != n_lab:
            settings.append((tag + "_wave", m))
        elif _lib.lib.dram_label_shape_plan(kind, n_lab) == 1:
            settings.append((tag + "_lds", 1))                                  # plan 0 on the same volume: only label 1 counts
        for name, n_use in settings:
            t, buf = shape_call(labels_t, kind, n_use)
            if args.host:
                import shape_restatement as SR
                h = labels_h if labels_h is not None else labels_t.cpu().numpy()
                t0 = time.perf_counter()
                ref = SR.tables(h, n_use)
                t["numpy_s"] = time.perf_counter() - t0
                got = buf.cpu().numpy()
                t["equal_to_numpy"] = bool(np.array_equal(got[:n_use * 256].reshape(n_use, 256), ref["cfg"])
                                           and np.array_equal(got[n_use * 256:].reshape(n_use, 10), ref["mom"]))
                t["numpy_over_gpu"] = t["numpy_s"] * 1e3 / t["ms_median"]
            record("shape_" + name, t, bpv, n=n_use)
            d = density_call(labels_t, kind, n_use)
            record("density_" + name, d, bpv + 2, n=n_use)
            ratios[name] = t["ms_median"] / d["ms_median"]
    result["shape_over_density"] = ratios

    print(f"{result['device']}: {shape}, {n_comp} components of {result['set_voxels']} set voxels, {n_lobe} lobes, copy rate {copy_tbs:.2f} TB/s")
    for name, t in calls.items():
        extra = "" if "numpy_s" not in t else f", numpy {t['numpy_s']:.2f} s = {t['numpy_over_gpu']:.0f} x, equal: {t['equal_to_numpy']}"
        print(f"  {name:34s} n {t['n']:6d} plan {t['plan']} median {t['ms_median']:8.3f} ms (min {t['ms_min']:.3f}), floor {t['floor_ms']:.3f} ms, "
              f"{t['over_floor']:.1f} x the floor{extra}")
    print("  shape / density (no histogram): " + ", ".join(f"{k} {v:.2f} x" for k, v in ratios.items()))
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
