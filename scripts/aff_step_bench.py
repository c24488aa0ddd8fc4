"""Step time of the reference's headline recipe on one GPU: DeviceIntRegAffRefineLoss around DC3DATGeneric(st_dram_ref_att)
at TRAIN_BATCH_SIZE 10 chunks of RESAMPLE_SIZE 80^3 -- two forward passes (the batch and its transformed copy) per backward.
    python scripts/aff_step_bench.py [--mode trainer|by-hand] [--n 10] [--size 80] [--micro M] [--steps 5]
--mode trainer   DataParallelTrainer.step with the loss as loss_fn (one transform per step, targets of the copy on the device)
--mode by-hand   loss(model, batch), the weighted sum, backward(), opt.step(): the only way to run this loss on a tree whose
                 trainer does not take it, so the same script times both sides of a comparison
The model returns (dense, refined); the loss wants a third, class-map output, which no shipped model has: the refined map
stands in for it (one more transform and one more masked smooth-L1 over a 1-channel map, as a real one would cost).
`random` / `numpy.random` are re-seeded before every step, so every step -- warm-up, timed, either mode -- draws the same T.
Prints one dict: ms per step (best and spread of --steps steps, device events on the stream), peak GB, and -- where the
library has it -- the regression-target kernels alone against their floor, the time the copy kernel's rate needs to read
the two masks once (they are HBM-bound: 8 B/voxel read, nothing written but 4 floats per sample)."""
import argparse
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bodyct-dram_amd")]
FACTORS = [2.0, 1.0, 0.5, 0.5]          # LOSS_FACTORS, st_dram_ref_att.py:45


class ThreeOut(torch.nn.Module):
    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, imgs, lbs):
        dense, refined = self.net(imgs, lbs)
        return dense, refined, refined


def _best_ms(fn, reps, inner=1):
    """Best and worst of `reps` timings of `inner` calls each, device events on the current stream."""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / inner)
    return min(out), max(out)


def targets_alone(batch):
    """(ms of dram_intreg_targets on the batch's masks, ms the copy kernel's rate needs for the same bytes read once)."""
    from dram_amd import _lib, functional as HF
    if not hasattr(HF, "intreg_targets"):
        return None
    ctss = batch.ctss_device()
    freq = [1.0 / 6] * 6
    run = lambda: HF.intreg_targets(batch.lobes, batch.lesions, ctss, freq, 5e-2)
    nbytes = 2 * batch.lobes.numel() * 4
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda").zero_()
    dst = torch.empty_like(src)
    st = torch.cuda.current_stream().cuda_stream
    copy = lambda: _lib.call("dram_calibrate_hbm_copy", dst.data_ptr(), src.data_ptr(), nbytes, st)
    for _ in range(3):
        run()
        copy()
    t_tgt, _ = _best_ms(run, 5, inner=20)
    t_copy, _ = _best_ms(copy, 5, inner=20)
    floor = t_copy / 2.0                 # the copy moves every byte twice (read + write); the targets read them once
    return {"targets_ms": t_tgt, "copy_ms_same_bytes": t_copy, "copy_gb_s": 2 * nbytes / t_copy / 1e6,
            "floor_ms": floor, "floor_over_targets": floor / t_tgt, "mask_bytes": nbytes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["trainer", "by-hand"], default="trainer")
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--size", type=int, default=80)
    ap.add_argument("--micro", type=int, default=0, help="micro-batch of the trainer (0: the whole batch)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--slim", action="store_true", help="DC3DATGeneric(SLIM_ATT): a rehearsal size, not a measurement")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is nothing to fall back to"
    import models
    from dram_amd.configs import SLIM_ATT, ST_DRAM_REF_ATT_MODEL
    from dram_amd.train_step import DataParallelTrainer, DeviceIntRegAffRefineLoss, synthetic_batch
    torch.manual_seed(0)
    net = models.DC3DATGeneric(**(SLIM_ATT if a.slim else ST_DRAM_REF_ATT_MODEL))
    net.init(models.HeNorm(mode="fan_in"))
    m = ThreeOut(net).cuda().train()
    pool = [a.size - a.size // 5, a.size - a.size // 10, a.size]          # 64, 72, 80 at the reference's size
    loss = DeviceIntRegAffRefineLoss(rescale_jitter=pool, band_width=5e-2, smoothing=0.05)
    opt = torch.optim.Adam(m.parameters(), lr=1e-4)
    batch = synthetic_batch(a.n, a.size, 100, torch.device("cuda"))
    drawn = []

    def reseed():
        random.seed(a.seed)
        np.random.seed(a.seed)

    if a.mode == "trainer":
        tr = DataParallelTrainer(m, opt, loss_fn=loss, loss_factors=FACTORS)
        orig = loss.draw

        def draw():
            T = orig()
            drawn.append([(type(t).__name__, getattr(t, "scale_factor", None)) for t in T.p])
            return T
        loss.draw = draw

        def step():
            reseed()
            return tr.step(batch, micro_batch=a.micro or None)
    else:
        def step():
            reseed()
            opt.zero_grad(set_to_none=True)
            terms = loss(m, batch)
            sum(f * t for f, t in zip(FACTORS, terms)).backward()
            opt.step()
            return tuple(t.detach() for t in terms)

    for _ in range(a.warmup):
        terms = step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    times = []
    for _ in range(a.steps):
        lo, _ = _best_ms(lambda: step(), 1)
        times.append(lo)
    terms = step()
    torch.cuda.synchronize()
    out = {"model": "DC3DATGeneric(%s) + refined as the third output" % ("SLIM_ATT" if a.slim else "st_dram_ref_att"),
           "loss": "DeviceIntRegAffRefineLoss", "mode": a.mode, "chunks": a.n, "size": a.size, "micro_batch": a.micro or a.n,
           "rescale_pool": pool, "transform": drawn[-1] if drawn else "seed %d" % a.seed,
           "ms_per_step_best": min(times), "ms_per_step_worst": max(times), "ms_per_step_all": [round(t, 2) for t in times],
           "peak_gb": torch.cuda.max_memory_allocated() / 2 ** 30, "terms": [float(t) for t in terms]}
    alone = targets_alone(batch)
    if alone is not None:
        out["targets_kernel"] = alone
    print(out)


if __name__ == "__main__":
    main()
