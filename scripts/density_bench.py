"""Times the lesion density kernels (csrc/density.hip) on the scan of inference.synthetic_ct() at 300x512x512, its lobe map and
the components of its lesion mask -- the lesions thresholded directly, no model -- against the copy rate measured in the same
process and against scipy.ndimage on the host.

    python scripts/density_bench.py [--out FILE] [--shape 300,512,512] [--reps 10] [--no-scipy]

Timed: dram_label_density in both regimes (the lobe map, uint8 labels in LDS, with and without the 4096-bin histogram; the
component labels, int32, with and without it -- a few dozen components without a histogram still fit in LDS, so the wave regime
is also timed on the same labels with n raised past the LDS regime), dram_hist_summary over the lobes' histograms, and
lesions.lesion_report with and without `scan=` (host clock around the call, which ends in a read-back).  HIP events around each
kernel call on the launch stream, one warm-up, median and minimum of --reps.  Floors are the bytes a call must at least read, at
the copy rate: 2 (scan) + 1 or 4 (labels) bytes per voxel.  Every device result is compared with numpy on the host.  scipy
(sum_labels, minimum, maximum, histogram over the same labels) runs once on at most 16 host threads (it uses one); where scipy
does not import the figure is null.  Prints a table, then one JSON line.
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
    from dram_amd.density import HIST_RANGE, hist_summary
    from dram_amd.inference import synthetic_ct
    from dram_amd.lesions import label_components, lesion_report
    if not torch.cuda.is_available():
        raise SystemExit("density_bench: needs a GPU (times measured anywhere else say nothing)")
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

    def host_timed(fn, reps=3):
        fn()
        torch.cuda.synchronize()
        s = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            s.append((time.perf_counter() - t0) * 1e3)
        return {"ms_median": statistics.median(s), "ms_min": min(s), "ms_max": max(s)}

    n = 1 << 30
    src, dst = torch.zeros(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    copy = timed(lambda: _lib.call("dram_calibrate_hbm_copy", src.data_ptr(), dst.data_ptr(), n, st), 5)
    copy_tbs = 2.0 * n / (copy["ms_min"] * 1e-3) / 1e12
    del src, dst
    torch.cuda.empty_cache()

    scan, lobe, spacing = synthetic_ct(shape)
    mask = ((scan > -575) & (lobe > 0)).astype(np.uint8)        # between the parenchyma (-850 +- 60) and the lesions (-300 +- 80)
    nvox = mask.size
    scan_d, lobe_d, mask_d = torch.from_numpy(scan).to(dev), torch.from_numpy(lobe).to(dev), torch.from_numpy(mask).to(dev)
    labels_d, n_comp = label_components(mask_d, 1)
    n_lobe = int(lobe.max())
    lo, width, nbins = HIST_RANGE
    result = {"device": torch.cuda.get_device_name(0), "shape": list(shape), "set_voxels": int(mask.sum()), "components": n_comp,
              "lobes": n_lobe, "hbm_copy_tbs": copy_tbs, "calls": {}}

    def record(name, t, bytes_per_voxel=None, **extra):
        if bytes_per_voxel is not None:
            floor = bytes_per_voxel * nvox / (copy_tbs * 1e12) * 1e3
            t.update(floor_ms=floor, over_floor=t["ms_median"] / floor, share_of_copy_rate=floor / t["ms_median"])
        t.update(extra)
        result["calls"][name] = t

    def density(labels_t, kind, n_lab, with_hist):
        count, total, sumsq = (torch.empty(n_lab, dtype=torch.int64, device=dev) for _ in range(3))
        vmin, vmax = (torch.empty(n_lab, dtype=torch.int32, device=dev) for _ in range(2))
        hist = torch.empty((n_lab, nbins + 2), dtype=torch.int64, device=dev) if with_hist else None
        t = timed(lambda: _lib.call("dram_label_density", scan_d.data_ptr(), labels_t.data_ptr(), kind, None, n_lab, count.data_ptr(),
                                    total.data_ptr(), sumsq.data_ptr(), vmin.data_ptr(), vmax.data_ptr(),
                                    None if hist is None else hist.data_ptr(), lo, width, nbins if with_hist else 0, nvox, st))
        t["regime"] = _lib.lib.dram_label_density_plan(kind, n_lab, nbins if with_hist else 0)
        return t, (count, total, sumsq, vmin, vmax, hist)

    def check(out, labels_h, n_lab):
        """The device tables against numpy on the host (bincount over the labelled voxels)."""
        sel = labels_h.reshape(-1) > 0
        k, v = labels_h.reshape(-1)[sel].astype(np.int64) - 1, scan.reshape(-1)[sel].astype(np.int64)
        ok = np.array_equal(out[0].cpu().numpy(), np.bincount(k, minlength=n_lab))
        ok &= np.array_equal(out[1].cpu().numpy(), np.bincount(k, weights=v, minlength=n_lab).astype(np.int64))
        ok &= np.array_equal(out[2].cpu().numpy(), np.bincount(k, weights=v * v, minlength=n_lab).astype(np.int64))
        if out[5] is not None:
            b = np.where(v < lo, 0, np.where(v < lo + nbins * width, 1 + (v - lo) // width, nbins + 1))
            ok &= np.array_equal(out[5].cpu().numpy().reshape(-1), np.bincount(k * (nbins + 2) + b, minlength=n_lab * (nbins + 2)))
        return bool(ok)

    labels_h = labels_d.cpu().numpy()
    lobe_hist = None
    for name, lab_t, lab_h, kind, n_lab, bpv in (("lobes", lobe_d, lobe, 0, n_lobe, 3), ("components", labels_d, labels_h, 1, max(n_comp, 1), 6)):
        for with_hist in (False, True):
            t, out = density(lab_t, kind, n_lab, with_hist)
            t["equal_to_numpy"] = check(out, lab_h, n_lab)
            record(f"density_{name}" + ("_hist" if with_hist else ""), t, bpv)
            if name == "lobes" and with_hist:
                lobe_hist = out[5]

    # the same component labels with n raised past what the LDS regime takes without a histogram (the labels above n_comp stay
    # empty): the wave regime on its own, as a scan with thousands of components would take it
    n_wave = max(n_comp, 1)
    while _lib.lib.dram_label_density_plan(1, n_wave, 0) == 0:
        n_wave *= 2
    t, out = density(labels_d, 1, n_wave, False)
    t["equal_to_numpy"] = check(out, labels_h, n_wave)
    record("density_components_wave", t, 6, n=n_wave)

    q = np.array([150, 500, 850], dtype=np.int32)
    edges = np.array([-950, -750, -300], dtype=np.int32)
    pct = torch.empty((n_lobe, 3), dtype=torch.int32, device=dev)
    bands = torch.empty((n_lobe, 4), dtype=torch.int64, device=dev)
    record("hist_summary_lobes", timed(lambda: _lib.call("dram_hist_summary", lobe_hist.data_ptr(), n_lobe, lo, width, nbins, q.ctypes.data, 3,
                                                         edges.ctypes.data, 3, pct.data_ptr(), bands.data_ptr(), st)))
    p_host, _ = hist_summary(lobe_hist, HIST_RANGE, q, edges)
    result["perc15_hu_per_lobe"] = p_host[:, 0].tolist()

    record("lesion_report", host_timed(lambda: lesion_report(mask_d, lobe_d, spacing)))
    record("lesion_report_with_scan", host_timed(lambda: lesion_report(mask_d, lobe_d, spacing, scan=scan_d)))

    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    if args.no_scipy:
        ndimage = None
    if ndimage is not None:
        for name, lab_h, n_lab in (("lobes", lobe, n_lobe), ("components", labels_h, max(n_comp, 1))):
            index = np.arange(1, n_lab + 1)
            t0 = time.perf_counter()
            ndimage.sum_labels(scan, lab_h, index)
            ndimage.minimum(scan, lab_h, index)
            ndimage.maximum(scan, lab_h, index)
            t1 = time.perf_counter()
            ndimage.histogram(scan, lo, lo + nbins * width, nbins, lab_h, index)
            t2 = time.perf_counter()
            for key, s in ((f"density_{name}", t1 - t0), (f"density_{name}_hist", t2 - t0)):
                result["calls"][key].update(scipy_s=s, scipy_over_gpu=s * 1e3 / result["calls"][key]["ms_median"])

    print(f"{result['device']}: {shape}, {n_comp} components of {result['set_voxels']} set voxels, {n_lobe} lobes, "
          f"copy rate {copy_tbs:.2f} TB/s")
    for name, t in result["calls"].items():
        floor = "" if "floor_ms" not in t else (f", floor {t['floor_ms']:.3f} ms, {100 * t['share_of_copy_rate']:.0f} % of the copy rate, "
                                                f"regime {t['regime']}, equal to numpy: {t['equal_to_numpy']}")
        extra = "" if t.get("scipy_s") is None else f", scipy {t['scipy_s']:.2f} s = {t['scipy_over_gpu']:.0f} x"
        print(f"  {name:26s} median {t['ms_median']:8.3f} ms (min {t['ms_min']:.3f}){floor}{extra}")
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
