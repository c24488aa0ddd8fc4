"""Times the lesion distribution kernels (csrc/distribution.hip, with csrc/distance.hip for the depth map) on the scan of
inference.synthetic_ct() at 300x512x512, its lobe map and the components of its lesion mask -- the lesions thresholded directly,
no model -- against the copy rate measured in the same process, against dram_label_density on the same label volumes and
against scipy.ndimage on the host.

    python scripts/distribution_bench.py [--out FILE] [--shape 300,512,512] [--reps 10] [--no-scipy]

Timed: lung_depth on its own; dram_label_depth over the lobe map (uint8 labels, table in LDS) with the report's histogram and
zones, without a mask and with the lesion mask; dram_label_depth over the component labels (int32, zones, no histogram) as the
report calls it and with n raised past the LDS regime (the wave regime on its own); dram_label_density on the same label volumes
with and without its histogram; and the whole lesion_distribution call (host clock around the call, which ends in a read-back).
HIP events around each kernel call on the launch stream, one warm-up, median and minimum of --reps.  Floors are the bytes a call
must at least read, at the copy rate: 4 (depth) + 1 or 4 (labels) + 1 (mask) bytes per voxel.  Every device table is compared
with numpy on the host.  scipy (distance_transform_edt over the lobe map, then sum_labels, minimum and center_of_mass over the
same labels) runs once; where scipy does not import the figure is null.  Prints a table, then one JSON line.
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
    from dram_amd.distribution import BINS_PER_MM, NBINS, ZONES, lesion_distribution, lung_depth
    from dram_amd.inference import synthetic_ct
    from dram_amd.lesions import label_components
    if not torch.cuda.is_available():
        raise SystemExit("distribution_bench: needs a GPU (times measured anywhere else say nothing)")
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
    n_comp = max(n_comp, 1)
    n_lobe = int(lobe.max())
    idx = np.argwhere(lobe > 0)
    box = np.array([v for a in range(3) for v in (idx[:, a].min(), idx[:, a].max() + 1)], dtype=np.int32)
    nzt = ZONES[0] * ZONES[1] * ZONES[2]
    result = {"device": torch.cuda.get_device_name(0), "shape": list(shape), "lung_voxels": int((lobe > 0).sum()),
              "set_voxels": int(mask.sum()), "components": n_comp, "lobes": n_lobe, "hbm_copy_tbs": copy_tbs, "calls": {}}

    def record(name, t, bytes_per_voxel=None, **extra):
        if bytes_per_voxel is not None:
            floor = bytes_per_voxel * nvox / (copy_tbs * 1e12) * 1e3
            t.update(floor_ms=floor, over_floor=t["ms_median"] / floor, share_of_copy_rate=floor / t["ms_median"])
        t.update(extra)
        result["calls"][name] = t

    record("lung_depth", timed(lambda: lung_depth(lobe_d, spacing)))
    depth_d = lung_depth(lobe_d, spacing)
    depth = depth_d.cpu().numpy()

    def label_depth(labels_t, kind, n_lab, mask_t, nbins, zones):
        count, qsum, possum = (torch.empty(s, dtype=torch.int64, device=dev) for s in (n_lab, n_lab, 3 * n_lab))
        dmin, dmax = (torch.empty(n_lab, dtype=torch.int32, device=dev) for _ in range(2))
        hist = torch.empty((n_lab, nbins + 2), dtype=torch.int64, device=dev) if nbins else None
        zt = torch.empty((n_lab, nzt), dtype=torch.int64, device=dev) if zones else None
        nz = ZONES if zones else (1, 1, 1)
        t = timed(lambda: _lib.call("dram_label_depth", depth_d.data_ptr(), labels_t.data_ptr(), kind, None if mask_t is None else mask_t.data_ptr(),
                                    n_lab, count.data_ptr(), qsum.data_ptr(), dmin.data_ptr(), dmax.data_ptr(), possum.data_ptr(),
                                    None if hist is None else hist.data_ptr(), BINS_PER_MM, nbins, None if zt is None else zt.data_ptr(),
                                    box.ctypes.data if zones else None, *nz, *shape, st))
        t["regime"] = _lib.lib.dram_label_depth_plan(kind, n_lab, nbins, nzt if zones else 0)
        return t, (count, qsum, possum, hist, zt)

    def check(out, labels_h, mask_h, n_lab, nbins):
        """The device tables against numpy on the host (bincount over the contributing voxels)."""
        lab = labels_h.reshape(-1)
        sel = lab > 0
        if mask_h is not None:
            sel &= mask_h.reshape(-1) != 0
        v = np.nonzero(sel)[0]
        k, d = lab[v].astype(np.int64) - 1, depth.reshape(-1)[v]
        q = (np.minimum(d, np.float32(2097152.0)) * np.float32(1024.0)).astype(np.int64)
        ok = np.array_equal(out[0].cpu().numpy(), np.bincount(k, minlength=n_lab))
        ok &= np.array_equal(out[1].cpu().numpy(), np.bincount(k, weights=q, minlength=n_lab).astype(np.int64))
        z, y, x = np.unravel_index(v, shape)
        pos = np.stack([np.bincount(k, weights=a, minlength=n_lab).astype(np.int64) for a in (z, y, x)], axis=1)
        ok &= np.array_equal(out[2].cpu().numpy().reshape(n_lab, 3), pos)
        if out[3] is not None:
            b = d * np.float32(BINS_PER_MM)
            e = np.where(b >= np.float32(nbins), nbins + 1, 1 + np.minimum(b, nbins).astype(np.int64))
            ok &= np.array_equal(out[3].cpu().numpy().reshape(-1), np.bincount(k * (nbins + 2) + e, minlength=n_lab * (nbins + 2)))
        if out[4] is not None:
            zone = 0
            for a, (i, nza) in enumerate(zip((z, y, x), ZONES)):
                a0, a1 = int(box[2 * a]), int(box[2 * a + 1])
                zone = zone * nza + ((np.clip(i, a0, a1 - 1) - a0) * nza) // (a1 - a0)
            ok &= np.array_equal(out[4].cpu().numpy().reshape(-1), np.bincount(k * nzt + zone, minlength=n_lab * nzt))
        return bool(ok)

    def density(labels_t, kind, n_lab, with_hist):
        count, total, sumsq = (torch.empty(n_lab, dtype=torch.int64, device=dev) for _ in range(3))
        vmin, vmax = (torch.empty(n_lab, dtype=torch.int32, device=dev) for _ in range(2))
        hist = torch.empty((n_lab, 4098), dtype=torch.int64, device=dev) if with_hist else None
        t = timed(lambda: _lib.call("dram_label_density", scan_d.data_ptr(), labels_t.data_ptr(), kind, None, n_lab, count.data_ptr(),
                                    total.data_ptr(), sumsq.data_ptr(), vmin.data_ptr(), vmax.data_ptr(),
                                    None if hist is None else hist.data_ptr(), -1024, 1, 4096 if with_hist else 0, nvox, st))
        t["regime"] = _lib.lib.dram_label_density_plan(kind, n_lab, 4096 if with_hist else 0)
        return t

    labels_h = labels_d.cpu().numpy()
    for name, mask_t, mask_h, bpv in (("depth_lobes_hist_zones", None, None, 5), ("depth_lobes_hist_zones_masked", mask_d, mask, 6)):
        t, out = label_depth(lobe_d, 0, n_lobe, mask_t, NBINS, True)
        t["equal_to_numpy"] = check(out, lobe, mask_h, n_lobe, NBINS)
        record(name, t, bpv)
    t, out = label_depth(lobe_d, 0, n_lobe, None, 0, False)
    t["equal_to_numpy"] = check(out, lobe, None, n_lobe, 0)
    record("depth_lobes_moments_only", t, 5)
    t, out = label_depth(labels_d, 1, n_comp, None, 0, True)
    t["equal_to_numpy"] = check(out, labels_h, None, n_comp, 0)
    record("depth_components_zones", t, 8)
    n_wave = n_comp
    while _lib.lib.dram_label_depth_plan(1, n_wave, 0, nzt) == 0:
        n_wave *= 2
    t, out = label_depth(labels_d, 1, n_wave, None, 0, True)
    t["equal_to_numpy"] = check(out, labels_h, None, n_wave, 0)
    record("depth_components_zones_wave", t, 8, n=n_wave)

    # the yardstick: dram_label_density on the same label volumes (2-byte scan in place of the 4-byte depth)
    record("density_lobes", density(lobe_d, 0, n_lobe, False), 3)
    record("density_lobes_hist", density(lobe_d, 0, n_lobe, True), 3)
    record("density_components", density(labels_d, 1, n_comp, False), 6)
    n_dw = n_comp
    while _lib.lib.dram_label_density_plan(1, n_dw, 0) == 0:
        n_dw *= 2
    record("density_components_wave", density(labels_d, 1, n_dw, False), 6, n=n_dw)
    calls = result["calls"]
    result["depth_over_density"] = {"lobes_hist": calls["depth_lobes_hist_zones"]["ms_median"] / calls["density_lobes_hist"]["ms_median"],
                                    "lobes": calls["depth_lobes_moments_only"]["ms_median"] / calls["density_lobes"]["ms_median"],
                                    "components": calls["depth_components_zones"]["ms_median"] / calls["density_components"]["ms_median"],
                                    "components_wave": calls["depth_components_zones_wave"]["ms_median"] / calls["density_components_wave"]["ms_median"]}

    record("lesion_distribution_given_depth", host_timed(lambda: lesion_distribution(mask_d, lobe_d, spacing, labels=labels_d, n=n_comp, depth=depth_d)))
    record("lesion_distribution", host_timed(lambda: lesion_distribution(mask_d, lobe_d, spacing, labels=labels_d, n=n_comp)))
    rep = lesion_distribution(mask_d, lobe_d, spacing, labels=labels_d, n=n_comp, depth=depth_d)
    result["peripheral_share_per_lobe"] = {str(v): e["peripheral_share"] for v, e in rep["lobes"].items()}
    result["subpleural_lesions"] = int(rep["lesions"]["subpleural"].sum())

    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    if args.no_scipy:
        ndimage = None
    if ndimage is not None:
        t0 = time.perf_counter()
        ref = ndimage.distance_transform_edt(lobe > 0, sampling=spacing)
        t1 = time.perf_counter()
        result["edt_max_abs_diff_mm"] = float(np.abs(ref - depth).max())
        calls["lung_depth"].update(scipy_s=t1 - t0, scipy_over_gpu=(t1 - t0) * 1e3 / calls["lung_depth"]["ms_median"])
        total = t1 - t0
        for name, lab_h, n_lab in (("depth_lobes_moments_only", lobe, n_lobe), ("depth_components_zones", labels_h, n_comp)):
            index = np.arange(1, n_lab + 1)
            t0 = time.perf_counter()
            ndimage.sum_labels(ref, lab_h, index)
            ndimage.minimum(ref, lab_h, index)
            ndimage.center_of_mass(lab_h > 0, lab_h, index)
            s = time.perf_counter() - t0
            total += s
            calls[name].update(scipy_s=s, scipy_over_gpu=s * 1e3 / calls[name]["ms_median"])
        calls["lesion_distribution"].update(scipy_s=total, scipy_over_gpu=total * 1e3 / calls["lesion_distribution"]["ms_median"])

    print(f"{result['device']}: {shape}, {n_comp} components of {result['set_voxels']} set voxels, {n_lobe} lobes of "
          f"{result['lung_voxels']} voxels, copy rate {copy_tbs:.2f} TB/s")
    for name, t in calls.items():
        floor = "" if "floor_ms" not in t else (f", floor {t['floor_ms']:.3f} ms, {100 * t['share_of_copy_rate']:.0f} % of the copy rate, regime {t['regime']}"
                                                + ("" if "equal_to_numpy" not in t else f", equal to numpy: {t['equal_to_numpy']}"))
        extra = "" if t.get("scipy_s") is None else f", scipy {t['scipy_s']:.2f} s = {t['scipy_over_gpu']:.0f} x"
        print(f"  {name:34s} median {t['ms_median']:8.3f} ms (min {t['ms_min']:.3f}){floor}{extra}")
    print("  depth / density: " + ", ".join(f"{k} {v:.2f} x" for k, v in result["depth_over_density"].items()))
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
