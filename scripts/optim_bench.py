"""Times one optimiser step of dram_amd.optim.Adam against torch.optim.Adam on the parameter set of the reference model.

    python scripts/optim_bench.py [--out FILE] [--reps 10]

Parameters: every parameter of models.DC3D(**ST_DRAM_REF_MODEL) (16.3 M elements, 86 tensors) with random gradients, in two
layouts: gradients as separate tensors, and gradients as views into 32 MB flat buckets filled in reverse parameter order, as
DataParallelTrainer leaves them.  step() is timed by HIP events on the launch stream: one warm-up, median, minimum and maximum
of --reps.  Beside it: torch.optim.Adam with its defaults, torch.optim.Adam(fused=True) where the installed torch has it, and
the time 28 bytes per element (16 read, 12 written) take at the copy rate dram_calibrate_hbm_copy reaches in the same process.
Global-norm clipping (max_norm 1.0, the 2-norm; the random gradients have norm ~ 40, so every step clips) is timed the same way
beside them: the clipped fused step (set_grad_clip), dram_amd.optim.clip_grad_norm_ followed by the plain step, and
torch.nn.utils.clip_grad_norm_ followed by torch.optim.Adam.step().  Clipping in place shrinks the gradients from repetition
to repetition; none of the kernels' work depends on their values.
dram_amd.optim.RAdam and AdaBound are timed in the same process, plain and clipped: they move the same 28 bytes per element as
Adam, so the Adam time of the same run is what they are held against (`*_over_adam`), beside torch.optim.RAdam with its
defaults and with foreach=True.  AdaBound has no torch counterpart.  Every optimiser is stepped 6 times before it is timed,
so that RAdam is timed in its rectified branch (the one with the root and the quotient).
Prints one JSON line.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch
    import models
    from dram_amd import _lib, optim
    from dram_amd.configs import ST_DRAM_REF_MODEL
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench: needs a GPU (times measured anywhere else say nothing)")
    dev = torch.device("cuda")
    st = torch.cuda.current_stream().cuda_stream

    def timed(fn, reps=args.reps, warm=1):
        for _ in range(warm):
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

    torch.manual_seed(0)
    shapes = [tuple(p.shape) for p in models.DC3D(**ST_DRAM_REF_MODEL).parameters()]
    elements = sum(torch.Size(s).numel() for s in shapes)
    ideal_ms = 28.0 * elements / (copy_tbs * 1e12) * 1e3
    result = {"device": torch.cuda.get_device_name(0), "hbm_copy_tbs": copy_tbs, "tensors": len(shapes), "elements": elements,
              "adam_28_bytes_per_element_at_copy_rate_ms": ideal_ms, "table_capacity": optim.TABLE_CAPACITY, "layouts": {}}

    def grads(layout):
        if layout == "separate":
            return [torch.randn(s, device=dev) * 0.01 for s in shapes]
        out, cap, cur = [None] * len(shapes), 32 << 20, []
        order = list(reversed(range(len(shapes))))
        buckets, size = [], 0
        for i in order:
            cur.append(i)
            size += torch.Size(shapes[i]).numel() * 4
            if size >= cap:
                buckets.append(cur)
                cur, size = [], 0
        if cur:
            buckets.append(cur)
        for b in buckets:
            flat = torch.randn(sum(torch.Size(shapes[i]).numel() for i in b), device=dev) * 0.01
            off = 0
            for i in b:
                k = torch.Size(shapes[i]).numel()
                out[i] = flat[off:off + k].view(shapes[i])
                off += k
        return out

    def fused_clip(ps, cls=optim.Adam, **kw):
        opt = cls(ps, lr=1e-4, **kw)
        opt.set_grad_clip(1.0)
        return opt

    class ClipThenStep:
        def __init__(self, clip, opt, ps):
            self.clip, self.opt, self.ps = clip, opt, ps

        def step(self):
            self.clip(self.ps, 1.0)
            self.opt.step()

    makers = {"dram_amd.optim.Adam": lambda ps: optim.Adam(ps, lr=1e-4),
              "torch.optim.Adam": lambda ps: torch.optim.Adam(ps, lr=1e-4),
              "dram_amd.optim.Adam + set_grad_clip": fused_clip,
              "dram_amd clip_grad_norm_ + Adam": lambda ps: ClipThenStep(optim.clip_grad_norm_, optim.Adam(ps, lr=1e-4), ps),
              "torch clip_grad_norm_ + Adam": lambda ps: ClipThenStep(torch.nn.utils.clip_grad_norm_,
                                                                      torch.optim.Adam(ps, lr=1e-4), ps)}
    makers.update({"dram_amd.optim.RAdam": lambda ps: optim.RAdam(ps, lr=1e-4),
                   "dram_amd.optim.RAdam + set_grad_clip": lambda ps: fused_clip(ps, optim.RAdam),
                   "torch.optim.RAdam": lambda ps: torch.optim.RAdam(ps, lr=1e-4),
                   "torch.optim.RAdam(foreach=True)": lambda ps: torch.optim.RAdam(ps, lr=1e-4, foreach=True),
                   "dram_amd.optim.AdaBound": lambda ps: optim.AdaBound(ps, lr=1e-4, final_lr=0.01),
                   "dram_amd.optim.AdaBound + set_grad_clip": lambda ps: fused_clip(ps, optim.AdaBound, final_lr=0.01)})
    try:
        torch.optim.Adam([torch.zeros(1, device=dev, requires_grad=True)], fused=True)
        makers["torch.optim.Adam(fused=True)"] = lambda ps: torch.optim.Adam(ps, lr=1e-4, fused=True)
    except (RuntimeError, TypeError, ValueError) as e:
        result["torch_fused_unavailable"] = str(e)

    for layout in ("separate", "buckets_32mb"):
        rec = {}
        for name, make in makers.items():
            gs = grads(layout)                           # fresh ones: the clipping lines scale them in place
            rec["gradients_16_byte_aligned"] = sum(g.data_ptr() % 16 == 0 for g in gs)
            ps = [torch.randn(s, device=dev).mul_(0.1).requires_grad_() for s in shapes]
            for p, g in zip(ps, gs):
                p.grad = g
            opt = make(ps)
            r = timed(opt.step, warm=6)
            r["fraction_of_copy_rate"] = ideal_ms / r["ms_median"]
            rec[name] = r
            del opt, ps, gs
        ours, ref = rec["dram_amd.optim.Adam"], rec["torch.optim.Adam"]
        rec["ours_over_torch_default"] = ours["ms_median"] / ref["ms_median"]
        rec["no_slower_than_torch_default_within_spread"] = ours["ms_median"] <= ref["ms_median"] + max(
            ours["ms_max"] - ours["ms_min"], ref["ms_max"] - ref["ms_min"])
        clip, two, tclip = (rec[k] for k in ("dram_amd.optim.Adam + set_grad_clip", "dram_amd clip_grad_norm_ + Adam",
                                             "torch clip_grad_norm_ + Adam"))
        rec["clipped_over_unclipped"] = clip["ms_median"] / ours["ms_median"]
        rec["clipped_minus_unclipped_ms"] = clip["ms_median"] - ours["ms_median"]
        rec["clipped_over_clip_then_step"] = clip["ms_median"] / two["ms_median"]
        rec["clipped_over_torch_clip_then_step"] = clip["ms_median"] / tclip["ms_median"]
        rec["clipped_no_slower_than_torch_clip_then_step_within_spread"] = clip["ms_median"] <= tclip["ms_median"] + max(
            clip["ms_max"] - clip["ms_min"], tclip["ms_max"] - tclip["ms_min"])
        for k in ("RAdam", "AdaBound"):
            plain, clipped = rec[f"dram_amd.optim.{k}"], rec[f"dram_amd.optim.{k} + set_grad_clip"]
            rec[f"{k.lower()}_over_adam"] = plain["ms_median"] / ours["ms_median"]
            rec[f"{k.lower()}_clipped_over_adam_clipped"] = clipped["ms_median"] / clip["ms_median"]
        rec["radam_over_torch_default"] = rec["dram_amd.optim.RAdam"]["ms_median"] / rec["torch.optim.RAdam"]["ms_median"]
        rec["radam_over_torch_foreach"] = (rec["dram_amd.optim.RAdam"]["ms_median"]
                                           / rec["torch.optim.RAdam(foreach=True)"]["ms_median"])
        result["layouts"][layout] = rec
    line = json.dumps(result)
    print(line, flush=True)
    for layout, rec in result["layouts"].items():
        for name in makers:
            r = rec[name]
            print(f"{layout:>13} {name:<40} {r['ms_median']:7.3f} ms (min {r['ms_min']:.3f}, max {r['ms_max']:.3f})  "
                  f"{r['fraction_of_copy_rate']:.3f} of 28 B/element at the copy rate ({ideal_ms:.3f} ms)", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
