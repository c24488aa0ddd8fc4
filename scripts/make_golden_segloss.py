"""Writes tests/golden/segloss.npz: the reference's BootBinCrossEntropy and BinaryCrossEntropySmooth (dram/metrics.py:10-72)
run on the CPU in fp64 and in fp32, with torch autograd for the gradient with respect to the probabilities.

Needs the reference checkout (see oracle/make_golden.py for where it is expected and how it is imported); nothing of it is
copied: the fixture holds inputs, loss values and gradients.

    python scripts/make_golden_segloss.py

Per case `c` of CASES: c/p, c/t, c/voi (fp64 inputs; p strictly inside (0, 1), some elements beyond both clamps),
c/smoothing, c/boot, c/gboot (fp64 run), c/boot32, c/gboot32 (the same inputs rounded to fp32), c/smooth,
c/bce, c/gbce, c/bce32, c/gbce32 (BinaryCrossEntropySmooth on p, t).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import make_golden as MG  # noqa: E402

SHAPE = (2, 1, 5, 6, 7)
# (case, seed, smoothing, smooth, share of voi, share of t inside voi): t rare, t common (both alpha clamps), no inside
CASES = (("mixed", 1, 0.1, 1.0, 0.6, 0.5), ("rare", 2, 0.3, 0.5, 0.5, 0.05), ("common", 3, 0.0, 2.0, 0.7, 0.95),
         ("noinside", 4, 0.1, 1.0, 0.0, 0.0))


def inputs(seed, voi_share, t_share):
    g = torch.Generator().manual_seed(seed)
    p = torch.sigmoid(torch.randn(SHAPE, generator=g, dtype=torch.float64) * 3.0)
    flat = p.view(-1)
    flat[3], flat[4], flat[5], flat[6] = 1e-9, 1.0 - 1e-9, 3e-7, 1.0 - 3e-7        # beyond either loss's clamps, both sides
    voi = (torch.rand(SHAPE, generator=g, dtype=torch.float64) < voi_share).double()
    t = ((torch.rand(SHAPE, generator=g, dtype=torch.float64) < t_share) & (voi > 0)).double()
    return p, t, voi


def run(fn, p, *rest):
    p = p.clone().requires_grad_(True)
    loss = fn(p, *rest)
    loss.backward()
    return np.array(loss.item()), MG._np(p.grad)


def main():
    torch.set_num_threads(4)
    MG._import_reference()
    import metrics
    arrs = {}
    for case, seed, smoothing, smooth, voi_share, t_share in CASES:
        p, t, voi = inputs(seed, voi_share, t_share)
        boot, bce = metrics.BootBinCrossEntropy(smoothing), metrics.BinaryCrossEntropySmooth(smooth)
        arrs.update({f"{case}/p": MG._np(p), f"{case}/t": MG._np(t), f"{case}/voi": MG._np(voi),
                     f"{case}/smoothing": np.array(smoothing), f"{case}/smooth": np.array(smooth)})
        arrs[f"{case}/boot"], arrs[f"{case}/gboot"] = run(boot, p, t, voi)
        arrs[f"{case}/boot32"], arrs[f"{case}/gboot32"] = run(boot, p.float(), t.float(), voi.float())
        arrs[f"{case}/bce"], arrs[f"{case}/gbce"] = run(bce, p, t)
        arrs[f"{case}/bce32"], arrs[f"{case}/gbce32"] = run(bce, p.float(), t.float())
        print(case, "boot", arrs[f"{case}/boot"], arrs[f"{case}/boot32"], "bce", arrs[f"{case}/bce"], arrs[f"{case}/bce32"],
              "inside", int(voi.sum()), "t", int(t.sum()))
    assert float(arrs["noinside/voi"].sum()) == 0 and all(float(arrs[f"{c}/voi"].sum()) > 0 for c in ("mixed", "rare", "common"))
    MG._save("segloss", cases=np.array([c[0] for c in CASES]), **arrs)


if __name__ == "__main__":
    main()
