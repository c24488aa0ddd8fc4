"""Times the heat-map refinement (csrc/guided.hip, dram_amd/refine.py) on the scan of inference.synthetic_ct() at 300x512x512,
spacing (1.0, 0.7, 0.7), against the copy rate measured in the same process, against the floor and against the numpy / scipy
restatement on the host.

    python scripts/refine_bench.py [--out FILE] [--shape 300,512,512] [--reps 5] [--host-depth 24] [--only-run] [--tree DIR]

Timed: dram_guided_filter at radius 2, 4 and the cap (isotropic, in voxels), with the int16 scan and with a float32 volume as
the guide, on the whole volume and on the bounding box of the lobes (x widened to multiples of 4, as refine_heatmap cuts it);
HIP events around each call on the launch stream, one warm-up, median of --reps.  The floor is the bytes the DEFINITION must
move, at the copy rate: G (2 or 4) + P (4) + M (1) in, q (4) out = 11 B per voxel with the int16 guide, 13 B with a float32
one (ab = NULL) -- not the bytes of the six passes, which materialise fp64 intermediates: 9 + 40, 40 + 40, 41 + 24, 16 + 16,
16 + 16, 16 + 8 + 1 + 2 + 4 = 289 B per voxel with the int16 guide before the halo re-reads.  Then LobeInference.run as a whole
with refine=None and refine=True (the full-width model, host clock around calls closed by a synchronise), and the restatement
(tests/guided_restatement.py, direct sums; and the scipy uniform_filter route) on the first --host-depth slices, given as seconds
per voxel with the whole-scan time extrapolated from it.  0 skips it.
--only-run times run(refine=None) alone and needs nothing of this change; with --tree DIR the package and the library are taken
from another checkout (built there), which is how the untouched path is compared against the parent commit: the two commands
alternated in one session.  Prints a table, then one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", default="300,512,512")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-depth", type=int, default=24)
    ap.add_argument("--only-run", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    for p in (tree, os.path.join(tree, "bodyct-dram_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import numpy as np
    import torch
    import models
    from dram_amd import _lib
    from dram_amd.configs import ST_DRAM_REF_MODEL
    from dram_amd.inference import LobeInference, synthetic_ct
    if not torch.cuda.is_available():
        raise SystemExit("refine_bench: needs a GPU (times measured anywhere else say nothing)")
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    dev = torch.device("cuda")
    st = torch.cuda.current_stream().cuda_stream
    shape = tuple(int(v) for v in args.shape.split(","))
    D, H, W = shape
    S = D * H * W
    scan, lobe, spacing = synthetic_ct(shape, (1.0, 0.7, 0.7))
    spacing = [float(s) for s in spacing]
    scan_d, lobe_d = torch.from_numpy(scan).to(dev), torch.from_numpy(lobe).to(dev)
    result = {"device": torch.cuda.get_device_name(0), "tree": os.path.relpath(tree, ROOT), "shape": list(shape), "spacing": spacing,
              "lobe_voxels": int((lobe > 0).sum()), "calls": {}, "run": {}}

    torch.manual_seed(0)
    model = models.DC3D(**ST_DRAM_REF_MODEL)
    model.init(models.HeNorm(mode="fan_in"))
    model = model.cuda().eval()

    def time_run(tag, **kw):
        inf = LobeInference(model, **kw)
        res = inf.run(scan_d, lobe_d, spacing)
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            res = inf.run(scan_d, lobe_d, spacing)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        result["run"][tag] = {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}
        return res

    res = time_run("refine=None")
    if not args.only_run:
        res = time_run("refine=True", refine=True)
        htp = res["htp"]
        del res

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
        copy = timed(lambda: _lib.call("dram_calibrate_hbm_copy", src.data_ptr(), dst.data_ptr(), n, st))
        copy_tbs = 2.0 * n / (copy["ms_min"] * 1e-3) / 1e12
        result["hbm_copy_tbs"] = copy_tbs
        del src, dst
        torch.cuda.empty_cache()

        from dram_amd import refine, vessels
        cap = _lib.lib.dram_guided_max_radius()
        box = vessels._lobe_box(lobe_d, (0, 0, 0))
        result["box"] = [b.stop - b.start for b in box]
        guide_f = ((scan_d.float() + 1150.0) / 1500.0).clamp_(0.0, 1.0)
        for where, cut in (("whole", tuple(slice(0, n) for n in shape)), ("box", box)):
            p, m = htp[cut].contiguous(), lobe_d[cut].contiguous()
            q = torch.empty_like(p)
            ws = refine._workspace(p.shape, dev)
            nvox = p.numel()
            for kind, g, window, floor_b in (("int16", scan_d[cut].contiguous(), refine.DEFAULT_WINDOW, 11),
                                             ("float32", guide_f[cut].contiguous(), None, 13)):
                for r in (2, 4, cap):
                    t = timed(lambda: refine._filter_into(p, g, m, [r, r, r], 1e-3, window, q, None, ws))
                    floor = floor_b * nvox / (copy_tbs * 1e12) * 1e3
                    t.update(voxels=nvox, floor_ms=floor, over_floor=t["ms_median"] / floor)
                    result["calls"][f"guided_filter {where} {kind} r={r}"] = t
            del p, m, q, ws
            torch.cuda.empty_cache()

        result["host"] = None
        if args.host_depth > 0:
            import guided_restatement as GR
            from scipy.ndimage import uniform_filter
            z0 = box[0].start
            depth = min(box[0].stop - z0, args.host_depth)
            sl = slice(z0, z0 + depth)
            hp = htp[sl].cpu().numpy()
            t0 = time.perf_counter()
            GR.guided_filter(scan[sl], hp, lobe[sl], (4, 4, 4), 1e-3, refine.DEFAULT_WINDOW)
            direct = (time.perf_counter() - t0) / (depth * H * W)
            t0 = time.perf_counter()
            mk = (lobe[sl] > 0).astype(np.float64)
            g = GR.guide_values(scan[sl], refine.DEFAULT_WINDOW) * mk
            pp = hp.astype(np.float64) * mk
            f = lambda v: uniform_filter(v, size=9, mode="constant")
            nn = np.maximum(f(mk), 0.5 / 729.0)                    # the mean of the mask over 9^3: N / 729, at least one voxel
            mg, mp = f(g) / nn, f(pp) / nn
            a = (f(g * pp) / nn - mg * mp) / ((f(g * g) / nn - mg * mg) + 1e-3) * mk
            b = (mp - a * mg) * mk
            _ = (f(a) / nn * g + f(b) / nn) * mk
            uni = (time.perf_counter() - t0) / (depth * H * W)
            result["host"] = {"depth": depth, "radius": 4, "direct_s_per_voxel": direct, "uniform_filter_s_per_voxel": uni,
                              "direct_whole_scan_s_extrapolated": direct * S, "uniform_filter_whole_scan_s_extrapolated": uni * S}

    print(f"{result['device']} [{result['tree']}]: {shape}, {result['lobe_voxels']} lobe voxels"
          + (f", box {result['box']}, copy rate {result['hbm_copy_tbs']:.2f} TB/s" if "box" in result else ""))
    for name, t in result["run"].items():
        print(f"  run({name}) median {t['ms_median']:9.2f} ms (min {t['ms_min']:.2f}, max {t['ms_max']:.2f})")
    for name, t in result["calls"].items():
        print(f"  {name:38s} median {t['ms_median']:9.3f} ms (min {t['ms_min']:.3f}), floor {t['floor_ms']:.3f} ms, "
              f"{t['over_floor']:.1f} x the floor")
    if result.get("host"):
        h = result["host"]
        print(f"  host, radius 4, {h['depth']} slices: direct sums {h['direct_s_per_voxel'] * 1e6:.2f} us per voxel "
              f"({h['direct_whole_scan_s_extrapolated']:.0f} s for the scan, extrapolated), uniform_filter "
              f"{h['uniform_filter_s_per_voxel'] * 1e6:.2f} us per voxel ({h['uniform_filter_whole_scan_s_extrapolated']:.0f} s)")
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
