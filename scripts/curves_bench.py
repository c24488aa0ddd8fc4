"""Times the heat-map curve kernel (csrc/curves.hip) on the scan of inference.synthetic_ct() at 300x512x512 through LobeInference
(He-initialised reference-width model: the heat map a real run of this project gives, not a trained one), against the copy rate
and dram_lung_hist256 measured in the same process and against sklearn on the host.

    python scripts/curves_bench.py [--out FILE] [--shape 300,512,512] [--reps 10] [--no-sklearn]

Timed: dram_score_hist over the lobe map with and without gate / conf at 256, 1024 and 4096 bins on three maps -- the heat map
of the run ("real"), a uniform random map inside the lungs ("uniform": no two neighbours share a bin, so nothing aggregates) and
a map that sits in a handful of low bins with a thin tail ("peaked": what a trained sigmoid head gives, the worst case for the
per-bin atomics) --, dram_lung_hist256 on the same map and lobe volume, and dram_calibrate_hbm_copy.  HIP events around each call
on the launch stream, one warm-up, median and minimum of --reps.  The floor of a call is 6 bytes per voxel (score, reference,
region; 7 with a gate) over all voxels at the copy rate -- more than the kernel reads, which skips score, reference and gate
where 16 region bytes are zero; each call is also given as a multiple of dram_lung_hist256 on the same map and of the same call
on the uniform map.  Every device table is compared with numpy on the host.  sklearn (roc_auc_score + precision_recall_curve on
the lung voxels of the real map) runs once; where sklearn does not import the figure is null.  Prints a table, then one JSON line.
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
    ap.add_argument("--no-sklearn", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    import models
    from dram_amd import _lib
    from dram_amd.configs import ST_DRAM_REF_MODEL
    from dram_amd.curves import curves_from_tables
    from dram_amd.inference import LobeInference, synthetic_ct
    if not torch.cuda.is_available():
        raise SystemExit("curves_bench: needs a GPU (times measured anywhere else say nothing)")
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
    lesion = ((scan > -575) & (lobe > 0)).astype(np.uint8)      # between the parenchyma (-850 +- 60) and the lesions (-300 +- 80)
    torch.manual_seed(0)
    model = models.DC3D(**ST_DRAM_REF_MODEL)
    model.init(models.HeNorm(mode="fan_in"))
    inf = LobeInference(model.cuda().eval())
    scan_d, lobe_d, lesion_d = torch.from_numpy(scan).to(dev), torch.from_numpy(lobe).to(dev), torch.from_numpy(lesion).to(dev)
    res = inf.run(scan_d, lobe_d, spacing, lesion=lesion_d)
    gate_d = torch.empty(shape, dtype=torch.uint8, device=dev)
    _lib.call("dram_lesion_post", res["htp"].data_ptr(), scan_d.data_ptr(), None, None, gate_d.data_ptr(), float("-inf"),
              inf.post_window[0], inf.post_window[1], float(res["threshold_scan"]), scan_d.numel(), st)
    nvox, n_lobe = lobe.size, int(lobe.max())
    lung = lobe_d > 0
    n_lung = int(lung.sum())
    g = torch.Generator(device=dev).manual_seed(1)
    uniform = torch.rand(shape, generator=g, device=dev) * lung
    peaked = (0.02 + 0.002 * torch.randn(shape, generator=g, device=dev)).clamp_(0.0, 1.0)
    tail = torch.rand(shape, generator=g, device=dev) < 0.03
    peaked = torch.where(tail, torch.rand(shape, generator=g, device=dev), peaked) * lung
    maps = {"real": res["htp"], "uniform": uniform.contiguous(), "peaked": peaked.contiguous()}
    del tail
    result = {"device": torch.cuda.get_device_name(0), "shape": list(shape), "lung_voxels": n_lung, "lobes": n_lobe,
              "hbm_copy_tbs": copy_tbs, "threshold": res["threshold"], "calls": {}, "maps": {}}

    hist256 = torch.empty(256, dtype=torch.int64, device=dev)
    ssum = torch.empty(1, dtype=torch.float64, device=dev)
    for name, m in maps.items():
        t = timed(lambda: _lib.call("dram_lung_hist256", m.data_ptr(), lobe_d.data_ptr(), hist256.data_ptr(), ssum.data_ptr(), nvox, st))
        result["calls"][f"lung_hist256/{name}"] = t

    lobe_h = lobe.reshape(-1)
    sel = lobe_h > 0
    row_h = (lobe_h[sel].astype(np.int64) - 1) * 2 + (lesion.reshape(-1)[sel] != 0)

    def check(m_h, gate_h, nbins, hist, conf):
        """The device tables against numpy on the host (bincount over the lung voxels)."""
        s = m_h[sel]
        b = np.where(s >= 1.0, nbins, 1 + np.floor(s.astype(np.float64) * nbins).astype(np.int64))
        b = np.where(s >= 0.0, b, 0)
        if gate_h is not None:
            b = np.where(gate_h[sel] != 0, b, 0)
        flat = row_h * (nbins + 1) + b
        ok = np.array_equal(hist.cpu().numpy().reshape(-1), np.bincount(flat, minlength=n_lobe * 2 * (nbins + 1)))
        if conf is not None:
            q = np.where(b > 0, np.floor(np.minimum(s, 1.0).astype(np.float64) * 16777216.0), 0.0)
            ok &= np.array_equal(conf.cpu().numpy().reshape(-1),
                                 np.bincount(flat, weights=q, minlength=n_lobe * 2 * (nbins + 1)).astype(np.int64))
        return bool(ok)

    gate_h = gate_d.cpu().numpy().reshape(-1)
    for name, m in maps.items():
        m_h = m.cpu().numpy().reshape(-1)
        occupied = np.sort(np.bincount(np.floor(np.clip(m_h[sel], 0, 1) * 1024).astype(np.int64), minlength=1025))[::-1]
        result["maps"][name] = {"bins_of_1024_holding_90_percent": int(np.searchsorted(np.cumsum(occupied), 0.9 * occupied.sum()) + 1)}
        for nbins in (256, 1024, 4096):
            print(f"curves_bench: {name} map, {nbins} bins", file=sys.stderr, flush=True)
            for with_gate, with_conf in ((False, False), (True, False), (False, True), (True, True)):
                hist = torch.empty((n_lobe, 2, nbins + 1), dtype=torch.int64, device=dev)
                conf = torch.empty_like(hist) if with_conf else None
                t = timed(lambda: _lib.call("dram_score_hist", m.data_ptr(), lesion_d.data_ptr(), lobe_d.data_ptr(),
                                            gate_d.data_ptr() if with_gate else None, n_lobe, nbins, hist.data_ptr(),
                                            None if conf is None else conf.data_ptr(), nvox, st))
                bpv = 6 + int(with_gate)
                floor = bpv * nvox / (copy_tbs * 1e12) * 1e3
                base = result["calls"][f"lung_hist256/{name}"]["ms_median"]
                t.update(path=_lib.lib.dram_score_hist_plan(n_lobe, nbins, int(with_conf)), bytes_per_voxel=bpv, floor_ms=floor,
                         over_floor=t["ms_median"] / floor, over_lung_hist256=t["ms_median"] / base,
                         equal_to_numpy=check(m_h, gate_h if with_gate else None, nbins, hist, conf))
                result["calls"][f"score_hist/{name}/{nbins}" + ("/gate" if with_gate else "") + ("/conf" if with_conf else "")] = t
                if name == "real" and nbins == 1024 and with_conf and not with_gate:
                    c = curves_from_tables(hist.cpu().numpy(), conf.cpu().numpy())
                    result["real_map"] = {"auc_roc": float(c["auc_roc"][-1]), "average_precision": float(c["average_precision"][-1]),
                                          "best_dice": float(c["best_dice"][-1]), "best_dice_threshold": float(c["best_dice_threshold"][-1]),
                                          "dice_at_otsu": float(res["dice"]), "ece": float(c["ece"][-1])}
    for nbins in (256, 1024, 4096):
        for tail_ in ("", "/gate", "/conf", "/gate/conf"):
            a, b = result["calls"][f"score_hist/real/{nbins}{tail_}"], result["calls"][f"score_hist/uniform/{nbins}{tail_}"]
            a["over_uniform_map"] = a["ms_median"] / b["ms_median"]
            p = result["calls"][f"score_hist/peaked/{nbins}{tail_}"]
            p["over_uniform_map"] = p["ms_median"] / b["ms_median"]

    try:
        from sklearn import metrics
    except ImportError:
        metrics = None
    if args.no_sklearn:
        metrics = None
    result["sklearn_s"] = None
    if metrics is not None:
        t0 = time.perf_counter()
        s_h, y_h = res["htp"].cpu().numpy().reshape(-1)[sel], lesion.reshape(-1)[sel]          # the pull to the host is part of the route
        auc = metrics.roc_auc_score(y_h, s_h)
        metrics.precision_recall_curve(y_h, s_h)
        result["sklearn_s"] = time.perf_counter() - t0
        result["sklearn_auc_roc"] = float(auc)

    print(f"{result['device']}: {shape}, {n_lung} lung voxels in {n_lobe} lobes, copy rate {copy_tbs:.2f} TB/s")
    for name, t in result["calls"].items():
        extra = "" if "floor_ms" not in t else (f", path {t['path']}, {t['over_floor']:.2f} x the {t['bytes_per_voxel']} B/voxel floor "
                                                f"({t['floor_ms']:.3f} ms), {t['over_lung_hist256']:.2f} x lung_hist256"
                                                + (f", {t['over_uniform_map']:.2f} x the uniform map" if "over_uniform_map" in t else "")
                                                + f", equal to numpy: {t['equal_to_numpy']}")
        print(f"  {name:36s} median {t['ms_median']:8.3f} ms (min {t['ms_min']:.3f}){extra}")
    print(f"  maps: {result['maps']}")
    print(f"  real map at 1024 bins: {result.get('real_map')}")
    if result["sklearn_s"] is not None:
        print(f"  sklearn roc_auc_score + precision_recall_curve on the lung voxels: {result['sklearn_s']:.2f} s (AUC {result['sklearn_auc_roc']:.6f})")
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
