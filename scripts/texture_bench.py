"""Times the lesion texture kernel (csrc/texture.hip) on the scan of inference.synthetic_ct() at 300x512x512: its lobe map (uint8)
at 16 levels, and 32 component labels of its lesion mask (int32) -- the lesions thresholded directly, no model, the components
folded onto 32 labels -- at 16 and 32 levels, each with its own n and, where the arguments allow it, with n forced into the other
plan; against the copy rate measured in the same process, against dram_label_density without a histogram and dram_label_shape on
the same labels and, with --host, against the numpy restatement of the tests.

    python scripts/texture_bench.py [--out FILE] [--shape 300,512,512] [--reps 10] [--host]

HIP events around each call on the launch stream, one warm-up, median and minimum of --reps.  The floor is one read of scan plus
labels at the copy rate: 3 or 6 bytes per voxel.  With --host every device table is compared with the restatement.  Prints a
table, then one JSON line.
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

LO, WIDTH = -1000, 75


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
        raise SystemExit("texture_bench: needs a GPU (times measured anywhere else say nothing)")
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
    comp_d, n_comp = label_components(mask_d, 1)
    comp32_d = torch.where(comp_d > 0, (comp_d - 1) % 32 + 1, comp_d).to(torch.int32).contiguous()    # 32 labels, every lesion kept
    n_lobe = int(lobe.max())
    result = {"device": torch.cuda.get_device_name(0), "shape": list(shape), "set_voxels": int(mask.sum()), "components": n_comp,
              "lobes": n_lobe, "hbm_copy_tbs": copy_tbs, "calls": {}}
    calls = result["calls"]

    def record(name, t, bytes_per_voxel, **extra):
        floor = bytes_per_voxel * nvox / (copy_tbs * 1e12) * 1e3
        t.update(floor_ms=floor, over_floor=t["ms_median"] / floor, **extra)
        calls[name] = t

    def glcm_call(labels_t, kind, n_lab, levels):
        out = torch.empty((n_lab, 13, levels, levels), dtype=torch.int64, device=dev)
        t = timed(lambda: _lib.call("dram_label_glcm", scan_d.data_ptr(), labels_t.data_ptr(), kind, None, n_lab, LO, WIDTH, levels, 1,
                                    out.data_ptr(), *shape, st))
        t["plan"] = _lib.lib.dram_label_glcm_plan(kind, n_lab, levels, 1)
        return t, out

    def density_call(labels_t, kind, n_lab):
        count, total, sumsq = (torch.empty(n_lab, dtype=torch.int64, device=dev) for _ in range(3))
        vmin, vmax = (torch.empty(n_lab, dtype=torch.int32, device=dev) for _ in range(2))
        t = timed(lambda: _lib.call("dram_label_density", scan_d.data_ptr(), labels_t.data_ptr(), kind, None, n_lab, count.data_ptr(),
                                    total.data_ptr(), sumsq.data_ptr(), vmin.data_ptr(), vmax.data_ptr(), None, -1024, 1, 0, nvox, st))
        t["plan"] = _lib.lib.dram_label_density_plan(kind, n_lab, 0)
        return t

    def shape_call(labels_t, kind, n_lab):
        buf = torch.empty(n_lab * 266, dtype=torch.int64, device=dev)
        t = timed(lambda: _lib.call("dram_label_shape", labels_t.data_ptr(), kind, n_lab, buf[:n_lab * 256].data_ptr(),
                                    buf[n_lab * 256:].data_ptr(), *shape, st))
        t["plan"] = _lib.lib.dram_label_shape_plan(kind, n_lab)
        return t

    def other_plan(kind, n_lab, levels):
        """An n that the other plan takes: the nearest above n_lab for the wave plan (labels above n_lab do not occur, so the work
        is the same), the largest below it for the LDS plan (the labels above it then belong to nobody); None where there is
        none."""
        own = _lib.lib.dram_label_glcm_plan(kind, n_lab, levels, 1)
        m = n_lab
        while m >= 1 and _lib.lib.dram_label_glcm_plan(kind, m, levels, 1) == own:
            m += 1 if own == 0 else -1
        return m if m >= 1 and _lib.lib.dram_label_glcm_plan(kind, m, levels, 1) == 1 - own else None

    ratios = {}
    cases = (("lobes_u8_16", lobe_d, lobe, 0, n_lobe, 16, 1), ("components32_i32_16", comp32_d, None, 1, 32, 16, 4),
             ("components32_i32_32", comp32_d, None, 1, 32, 32, 4))
    for tag, labels_t, labels_h, kind, n_lab, levels, bpv in cases:
        settings = [(tag, n_lab)]
        m = other_plan(kind, n_lab, levels)
        if m is not None:
            settings.append((f"{tag}_plan{_lib.lib.dram_label_glcm_plan(kind, m, levels, 1)}_n{m}", m))
        for name, n_use in settings:
            t, out = glcm_call(labels_t, kind, n_use, levels)
            if args.host:
                import texture_restatement as TR
                h = labels_h if labels_h is not None else labels_t.cpu().numpy()
                t0 = time.perf_counter()
                ref = TR.glcm(scan, h, n_use, None, levels, LO, WIDTH, 1)
                t["numpy_s"] = time.perf_counter() - t0
                t["equal_to_numpy"] = bool(np.array_equal(out.cpu().numpy(), ref))
                t["numpy_over_gpu"] = t["numpy_s"] * 1e3 / t["ms_median"]
            t["pairs"] = int(out.sum().item())
            record("glcm_" + name, t, bpv + 2, n=n_use, levels=levels)
            if levels == 16:
                d, s = density_call(labels_t, kind, n_use), shape_call(labels_t, kind, n_use)
                record("density_" + name, d, bpv + 2, n=n_use)
                record("shape_" + name, s, bpv, n=n_use)
                ratios[name] = {"over_density": t["ms_median"] / d["ms_median"], "over_shape": t["ms_median"] / s["ms_median"]}
    result["glcm_ratios"] = ratios

    print(f"{result['device']}: {shape}, {n_comp} components of {result['set_voxels']} set voxels, {n_lobe} lobes, copy rate {copy_tbs:.2f} TB/s")
    for name, t in calls.items():
        extra = "" if "numpy_s" not in t else f", numpy {t['numpy_s']:.2f} s = {t['numpy_over_gpu']:.0f} x, equal: {t['equal_to_numpy']}"
        print(f"  {name:44s} n {t['n']:4d} plan {t['plan']} median {t['ms_median']:8.3f} ms (min {t['ms_min']:.3f}), floor {t['floor_ms']:.3f} ms, "
              f"{t['over_floor']:.1f} x the floor{extra}")
    print("  glcm / density (no histogram), glcm / shape: " + ", ".join(f"{k} {v['over_density']:.2f} x, {v['over_shape']:.2f} x" for k, v in ratios.items()))
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
