"""Writes tests/golden/intreg.npz and tests/golden/intregaff.npz: the reference's IntRegLoss and IntRegAffLoss
(dram/metrics.py:75-308) run on the CPU, the affine cases under fixed `random` / `numpy.random` seeds.

Needs the reference checkout (see oracle/make_golden.py for where it is expected and how it is imported); nothing of it is
copied: the fixtures hold inputs, the drawn transform chains, loss values and gradients.

    python scripts/make_golden_intreg.py

intreg.npz     images, lobes, lesions, ctss, dense (the logits the stand-in model returns as its second output), reg, enc,
               gdense = d(2 reg + 1 enc) / d dense.  band_width 5e-2, frequency map 1/6.
intregaff.npz  images, lobes, lesions, ctss, theta (parameters of the closed-form stand-in model of
               oracle/make_golden.py:gen_affloss), and per case: seed, T ("|"-joined class names of the drawn chain),
               chain (one int row per transform, see `_chain_rows`), out = (reg, aff, enc), gtheta =
               d(2 reg + 0.5 aff + 1 enc) / d theta.
"""
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import make_golden as MG  # noqa: E402

BAND_WIDTH = 5e-2
RESCALE_JITTER = [8, 10, 12, 14]
SATURATION = 17.4       # fp32 sigmoid(d) rounds to exactly 1 from about d = 17.33 on
# (case, seed): chosen so that every transform occurs, the kept chains have 0..3 members and one chain is empty
CASES_AFF = (("all3", 0), ("all3b", 18), ("fliprot", 4), ("rescale", 5), ("rotrescale", 10), ("none", 14))


class Obj:
    ctss_frequency_map = {k: 1.0 / 6 for k in range(6)}
    debug_path = os.path.join(os.sep, "tmp", "_dram_golden_dbg")
    epoch_n = 0


def _sphere_batch(N, S, seed):
    g = torch.Generator().manual_seed(seed)
    zz, yy, xx = np.meshgrid(*[np.arange(S)] * 3, indexing="ij")
    lobe = (((zz - S / 2 + .5) ** 2 + (yy - S / 2 + .5) ** 2 + (xx - S / 2 + .5) ** 2) < (0.45 * S) ** 2)
    lobes = torch.from_numpy(lobe.astype(np.float32))[None, None].repeat(N, 1, 1, 1, 1)
    images = torch.rand(N, 1, S, S, S, generator=g) * lobes
    lesions = ((images > 0.7) & (lobes > 0)).float()
    return g, images, lobes, lesions


def gen_intreg(metrics):
    N, S = 6, 12
    g, images, lobes, lesions = _sphere_batch(N, S, 78)
    ctss = [float(n % 6) for n in range(N)]
    dense = torch.randn(N, 1, S, S, S, generator=g) * 2.0
    dense[3] -= 1.6                                   # lesion ratio ~0.3, ctss 3: a lobe mean near 0.3 sits inside the band
    flat = dense.view(N, -1)
    flat[:, ::37] *= 12.0                             # a spread of logits far beyond fp32 sigmoid saturation, both signs
    flat[:, 5] = torch.tensor([18.0, -18.0, 30.0, -30.0, 95.0, -95.0])
    flat[:, 6] = torch.tensor([17.0, -17.0, 16.0, -16.0, 88.0, -104.0])
    dense = dense.clone().requires_grad_(True)
    decoy = torch.randn(N, 1, S, S, S, generator=g)   # first and third outputs: IntRegLoss must not look at them

    def model(imgs, lbs):
        return decoy, dense, decoy
    model.trace_path = None
    loss_fn = metrics.IntRegLoss(band_width=BAND_WIDTH)
    reg, enc = loss_fn(model, images, lobes, lesions, ctss, obj=Obj(), metas=None)
    (2.0 * reg + 1.0 * enc).backward()

    # the fixture must exercise what the tests claim
    assert all(float(l.sum()) > 0 for l in lobes), "every sample needs lobe voxels"
    assert sorted(set(int(c) for c in ctss)) == [0, 1, 2, 3, 4, 5]
    per_sample = [loss_fn.compute_reg_loss_with_probs(torch.sigmoid(dense[n:n + 1]).detach(), lobes[n:n + 1], lesions[n:n + 1],
                                                      ctss[n:n + 1], obj=Obj()).item() for n in range(N)]
    assert any(v > 0 for v in per_sample) and any(v == 0 for v in per_sample), per_sample
    d = dense.detach()
    p = torch.sigmoid(d)
    assert (d.abs() < SATURATION).any() and (d > SATURATION).any() and (d < -SATURATION).any()
    assert (p == 1).any() and (p == 0).any() and ((p > 0) & (p < 1)).any()
    assert torch.isfinite(reg) and torch.isfinite(enc) and torch.isfinite(dense.grad).all()
    print("intreg", reg.item(), enc.item(), "per-sample reg", per_sample)
    MG._save("intreg", images=MG._np(images), lobes=MG._np(lobes), lesions=MG._np(lesions), ctss=np.array(ctss),
             dense=MG._np(dense), reg=np.array(reg.item()), enc=np.array(enc.item()), gdense=MG._np(dense.grad))


def _chain_rows(chain):
    """One int row per transform: Flip3DOneShot (0, f2, f3, f4) with f_k = 1 when axis k is mirrored; Rotate903DOneShot
    (1, times, a, b); Rescale3DOneShot (2, d, h, w)."""
    rows = []
    for t in chain:
        name = type(t).__name__
        if name == "Flip3DOneShot":
            axes = {int(a) % 5 for a in t.flip_axis}
            rows.append([0] + [int(k in axes) for k in (2, 3, 4)])
        elif name == "Rotate903DOneShot":
            rows.append([1, int(t.rotate_times)] + [int(a) % 5 for a in t.rotate_axis])
        elif name == "Rescale3DOneShot":
            assert t.mode == "size"
            rows.append([2] + [int(v) for v in t.scale_factor])
        else:
            raise AssertionError(name)
    return np.array(rows, dtype=np.int64).reshape(-1, 4)


def draw_chain(metrics, seed):
    random.seed(seed)
    np.random.seed(seed)
    return metrics.IntRegAffLoss(rescale_jitter=RESCALE_JITTER, band_width=BAND_WIDTH).get_affine_transform().p


def gen_intregaff(metrics):
    N, S = 4, 12
    g, images, lobes, lesions = _sphere_batch(N, S, 92)
    ctss = [float(1 + n % 5) for n in range(N)]
    theta = torch.tensor([1.5, -0.4, 0.8], requires_grad=True)

    def model(imgs, lbs):      # the stand-in of oracle/make_golden.py:gen_affloss; IntRegAffLoss takes its first output
        a, b, c = theta[0], theta[1], theta[2]
        D, H, W = imgs.shape[-3:]
        rz = torch.linspace(0.0, 1.0, D).view(1, 1, D, 1, 1)
        rx = torch.linspace(0.0, 1.0, W).view(1, 1, 1, 1, W)
        dense = a * (imgs - 0.5) * 4.0 + b + 0.6 * c * rx - 0.4 * rz
        refined = 0.7 * dense - c * imgs
        cls = torch.cat([a * imgs + rz, imgs * imgs + b * c * rx], dim=1)
        return dense, refined, cls
    model.trace_path = None
    arrs, seen, lengths = {}, set(), set()
    for case, seed in CASES_AFF:
        random.seed(seed)
        np.random.seed(seed)
        loss_fn = metrics.IntRegAffLoss(rescale_jitter=RESCALE_JITTER, band_width=BAND_WIDTH)
        holder = {}
        orig = loss_fn.get_affine_transform

        def spy():
            holder["T"] = orig()
            return holder["T"]
        loss_fn.get_affine_transform = spy
        theta.grad = None
        reg, aff, enc = loss_fn(model, images, lobes, lesions, ctss, obj=Obj(), metas=None)
        (2.0 * reg + 0.5 * aff + 1.0 * enc).backward()
        names = [type(t).__name__ for t in holder["T"].p]
        seen.update(names)
        lengths.add(len(names))
        print("intregaff", case, seed, names, _chain_rows(holder["T"].p).tolist(), reg.item(), aff.item(), enc.item(),
              theta.grad.tolist())
        assert all(torch.isfinite(v) for v in (reg, aff, enc))
        arrs[f"{case}/seed"] = np.array(seed)
        arrs[f"{case}/T"] = np.array("|".join(names))
        arrs[f"{case}/chain"] = _chain_rows(holder["T"].p)
        arrs[f"{case}/out"] = np.array([reg.item(), aff.item(), enc.item()])
        arrs[f"{case}/gtheta"] = MG._np(theta.grad)
    assert seen == {"Flip3DOneShot", "Rotate903DOneShot", "Rescale3DOneShot"}, seen
    assert 0 in lengths, "one case needs an empty chain"
    assert all(float(l.sum()) > 0 for l in lobes)
    MG._save("intregaff", images=MG._np(images), lobes=MG._np(lobes), lesions=MG._np(lesions), ctss=np.array(ctss),
             theta=MG._np(theta), cases=np.array([c for c, _ in CASES_AFF]), **arrs)


def main():
    torch.set_num_threads(8)
    MG._import_reference()
    torch.Tensor.cuda = lambda self, *a, **k: self     # this process only (metrics.py:136,173 hard-code .cuda())
    import metrics
    if sys.argv[1:2] == ["scan"]:                      # list the chain each seed draws (to choose CASES_AFF)
        for seed in range(int(sys.argv[2]) if len(sys.argv) > 2 else 64):
            print(seed, [type(t).__name__ for t in draw_chain(metrics, seed)])
        return
    gen_intreg(metrics)
    gen_intregaff(metrics)


if __name__ == "__main__":
    main()
