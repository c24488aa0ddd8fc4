"""Times the general max-pool (dram_maxpool3d_fwd / _bwd) against the copy rate measured in the same process, and beside it the
dedicated 2x2x2 kernels (dram_maxpool3d_2_fwd / _bwd) on the same tensor: the yardstick for the 2 / 2 / 0 geometry.

    python scripts/pool_bench.py [--out FILE] [--shapes 16x64x128,10x64x80] [--reps 10]

HIP events around the launches on the launch stream, one warm-up, median and minimum of --reps.  Bytes moved are the
algorithm's: forward = the input once + 5 bytes per output (value and uint8 index); backward = 5 bytes per output + the input
gradient once (overlapping windows re-read outputs, but from cache: each is counted once).  16 x 64 x 128^3 is the first
pool of the benchmark network at the per-GPU micro-batch.  Prints one JSON line, then a table.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "bodyct-dram_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

GEOMETRIES = {"k122_s122_p0": ((1, 2, 2), (1, 2, 2), (0, 0, 0)), "k3_s2_p1": ((3, 3, 3), (2, 2, 2), (1, 1, 1)),
              "k2_s2_p0": ((2, 2, 2), (2, 2, 2), (0, 0, 0))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="16x64x128,10x64x80")
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch
    from dram_amd import _lib
    from dram_amd import functional as HF
    if not torch.cuda.is_available():
        raise SystemExit("pool_bench: needs a GPU (times measured anywhere else say nothing)")
    dev = torch.device("cuda")
    st = torch.cuda.current_stream().cuda_stream

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
    result = {"device": torch.cuda.get_device_name(0), "hbm_copy_tbs": copy_tbs, "shapes": {}}

    for spec in args.shapes.split(","):
        N, C, size = (int(v) for v in spec.split("x"))
        shape = (N, C, size, size, size)
        x = torch.randn(shape, device=dev)
        dx = torch.empty_like(x)
        rec = {"elements": x.numel()}
        for name, (k, s, p) in GEOMETRIES.items():
            osz = HF.max_pool3d_geometry(shape, k, s, p)[3]
            out = torch.empty((N, C) + osz, device=dev)
            idx = torch.empty(out.shape, dtype=torch.uint8, device=dev)
            gy = torch.randn(out.shape, device=dev)
            nbytes = 4.0 * x.numel() + 5.0 * out.numel()          # the same for both directions
            ideal_ms = nbytes / (copy_tbs * 1e12) * 1e3

            def finish(r):
                r["bytes"] = nbytes
                r["gbs"] = nbytes / (r["ms_median"] * 1e-3) / 1e9
                r["fraction_of_copy_rate"] = ideal_ms / r["ms_median"]
                return r
            geom = (N, C, size, size, size, *k, *s, *p)
            g = {"output": list(osz), "at_copy_rate_ms": ideal_ms}
            g["general_fwd"] = finish(timed(lambda: _lib.call("dram_maxpool3d_fwd", x.data_ptr(), out.data_ptr(), idx.data_ptr(),
                                                              *geom, st)))
            g["general_bwd"] = finish(timed(lambda: _lib.call("dram_maxpool3d_bwd", gy.data_ptr(), idx.data_ptr(), dx.data_ptr(),
                                                              *geom, st)))
            if name == "k2_s2_p0":      # the dedicated kernels on the same tensors, alternating with the general ones above
                ref_out, ref_dx = out.clone(), dx.clone()
                g["dedicated_fwd"] = finish(timed(lambda: _lib.call("dram_maxpool3d_2_fwd", x.data_ptr(), out.data_ptr(),
                                                                    idx.data_ptr(), N, C, size, size, size, st)))
                g["dedicated_bwd"] = finish(timed(lambda: _lib.call("dram_maxpool3d_2_bwd", gy.data_ptr(), idx.data_ptr(),
                                                                    dx.data_ptr(), N, C, size, size, size, st)))
                g["same_values"] = bool(torch.equal(ref_out, out)) and bool(torch.equal(ref_dx, dx))
                g["general_fwd_again"] = finish(timed(lambda: _lib.call("dram_maxpool3d_fwd", x.data_ptr(), out.data_ptr(),
                                                                        idx.data_ptr(), *geom, st)))
                g["general_bwd_again"] = finish(timed(lambda: _lib.call("dram_maxpool3d_bwd", gy.data_ptr(), idx.data_ptr(),
                                                                        dx.data_ptr(), *geom, st)))
                g["general_over_dedicated_fwd"] = g["general_fwd"]["ms_median"] / g["dedicated_fwd"]["ms_median"]
                g["general_over_dedicated_bwd"] = g["general_bwd"]["ms_median"] / g["dedicated_bwd"]["ms_median"]
            rec[name] = g
            del out, idx, gy
        result["shapes"][spec] = rec
        del x, dx
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line, flush=True)
    for spec, rec in result["shapes"].items():
        for name in GEOMETRIES:
            for k, r in rec[name].items():
                if isinstance(r, dict):
                    print(f"{spec:>12} {name:<13} {k:<18} {r['ms_median']:8.3f} ms (min {r['ms_min']:.3f}, max {r['ms_max']:.3f})  "
                          f"{r['bytes'] / 1e9:6.2f} GB  {r['gbs']:8.1f} GB/s  {r['fraction_of_copy_rate']:.3f} of the copy rate "
                          f"({copy_tbs * 1e3:.0f} GB/s)", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
