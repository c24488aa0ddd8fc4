"""The result contact sheet on the synthetic 300x512x512 CT of scripts/infer_bench.py, 1 GPU (HIP events, median of --reps):
the occupancy pass per coord axis against the copy rate over the bytes it must read and over the whole masks, the render, a
whole LobeInference.sheet, and (--host) the reference's recipe on the host: scipy.ndimage.zoom of the six whole volumes."""
import argparse, os, sys, time
import numpy as np, torch
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bodyct-dram_amd")]
from dram_amd import _lib
from dram_amd.inference import LobeInference, synthetic_ct
from dram_amd.sheet import pick_slices, result_sheet, sheet_occupancy, zoomed_extents

ap = argparse.ArgumentParser(); ap.add_argument("--shape", default="300,512,512"); ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--host", action="store_true", help="also time the host recipe (seconds of CPU time)")
args = ap.parse_args()
shape = tuple(int(v) for v in args.shape.split(","))
scan, lobe, spacing = synthetic_ct(shape, (1.0, 0.7, 0.7), seed=7)
dev = "cuda:0"
g = np.random.default_rng(3)
htp = np.where(lobe > 0, g.random(size=shape, dtype=np.float32) ** 4, 0).astype(np.float32)
pred, ref = (htp > 0.6).astype(np.uint8), ((scan > -600) & (lobe > 0)).astype(np.uint8)
post = (pred & (scan > -700)).astype(np.uint8)
d = lambda v: torch.from_numpy(v).to(dev)
scan_d, htp_d, pred_d, post_d, ref_d = d(scan), d(htp), d(pred), d(post), d(ref)


def timed(fn, reps=args.reps):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


n = int(np.prod(shape))
src, dst = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
t_copy = timed(lambda: _lib.call("dram_calibrate_hbm_copy", src.data_ptr(), dst.data_ptr(), n, torch.cuda.current_stream().cuda_stream))
rate = 2 * n / t_copy / 1e9                                      # TB/s: bytes read + written per ms / 1e9
print(f"copy rate over {n / 1e6:.1f} MB: {rate:.2f} TB/s", flush=True)
for ca in range(3):
    za, zb = zoomed_extents(shape, 360, ca)
    a, b = [k for k in range(3) if k != ca]
    zn = {a: za, b: zb}
    rows = int(np.prod([shape[k] if k == ca else min(zn[k], shape[k]) for k in (0, 1)]))      # rows (z, y) that the zoom samples
    must = 2 * rows * shape[2]                                   # two masks, whole rows of the sampled (z, y)
    t = timed(lambda: sheet_occupancy([pred_d, ref_d], 0, 360, ca))
    print(f"occupancy coord_axis {ca}: {t:.3f} ms; rows it must read {must / 1e6:.1f} MB -> {must / t / 1e9 / (rate / 2):.2f} of the read "
          f"rate, whole masks {2 * n / 1e6:.1f} MB -> {2 * n / t / 1e9 / (rate / 2):.2f}", flush=True)
rows4 = [[pred_d], [post_d], [ref_d], [htp_d]]
t = timed(lambda: result_sheet(scan_d, rows4, [pred_d, ref_d]))
out = result_sheet(scan_d, rows4, [pred_d, ref_d])
print(f"result_sheet (occupancy + read-back + render, 4 rows): {t:.3f} ms; slices {out['slice_ids']}, sheet {tuple(out['sheet'].shape)}", flush=True)
from dram_amd import sheet as sheet_mod
ids = out["slice_ids"]
real_pick = sheet_mod.pick_slices
sheet_mod.sheet_occupancy, keep = (lambda *a, **k: None), sheet_mod.sheet_occupancy
sheet_mod.pick_slices = lambda flags, num: ids                   # the render alone: the slice ids are given
t = timed(lambda: result_sheet(scan_d, rows4, [pred_d, ref_d]))
sheet_mod.sheet_occupancy, sheet_mod.pick_slices = keep, real_pick
nbytes = out["sheet"].numel()
print(f"render alone: {t:.3f} ms for {nbytes / 1e6:.1f} MB of sheet ({nbytes / t / 1e9 / (rate / 2):.3f} of the write rate)", flush=True)

res = {"htp": htp_d, "mask": pred_d, "mask_post": post_d}
inf = LobeInference(None)
t = timed(lambda: inf.sheet(res, scan_d, ref_d))
t0 = time.perf_counter(); inf.sheet(res, scan_d, ref_d)["sheet"].cpu(); t_wall = (time.perf_counter() - t0) * 1e3
print(f"LobeInference.sheet: {t:.3f} ms (HIP events), {t_wall:.2f} ms host clock with the sheet copied to the host", flush=True)

if args.host:
    from scipy import ndimage
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ratio = [360 / 512, 1.0, 360 / 512]
    vols = [np.flip(v, 0) for v in ((np.clip(scan, -1150, 350) + 1150) / 1500.0 * 255).astype(np.uint8)[None]] + \
        [np.flip(v, 0) for v in (pred * 255, post * 255, ref * 255, (np.clip(htp, 0, 1) * 255).astype(np.uint8), (pred > 0) | (ref > 0))]
    zoomed = [ndimage.zoom(v, ratio, order=1 if i == 0 else 0) for i, v in enumerate(vols)]
    found = ndimage.find_objects(zoomed[5].astype(np.uint8))[0][1]
    t_host = time.perf_counter() - t0
    print(f"host recipe (flip + ndimage.zoom of six volumes + find_objects; drawing not included): {t_host:.2f} s; planes {found.start}..{found.stop}; "
          f"device slices {pick_slices(sheet_occupancy([pred_d, ref_d], 0, 360, 1), 5)}")
