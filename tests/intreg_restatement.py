"""Restatement of the reference's IntRegLoss and IntRegAffLoss (dram/metrics.py:75-308) with torch ops, in whatever
precision its inputs have (the tests run it in fp64).  tests/test_intreg_loss_cpu.py pins it to the reference's own
results (tests/golden/intreg.npz, intregaff.npz); tests/test_gpu_intreg_loss.py then leans on it at other shapes.

The interval hinge and the OneShot transforms are the oracle's (O.reg_loss_with_probs, O.oneshot_chain), which
tests/test_oracle_golden.py pins; the entropy term and the way the two losses combine their parts are stated here."""
import torch
import torch.nn.functional as F

from oracle import dram_oracle as O

EPS = 1e-7


def enc_loss(p):
    """compute_enc_loss (metrics.py:154-156)."""
    return (-p * torch.log(p + EPS) + (p - 1.0) * torch.log(1.0 - p + EPS)).mean()


def int_reg_loss(dense, lobes, lesions, ctsses, freq_map, band_width=5e-2):
    """IntRegLoss.__call__ (metrics.py:204-210) given the logits it uses (the model's second output).  Returns (reg, enc)."""
    probs = torch.sigmoid(dense)
    return O.reg_loss_with_probs(probs, lobes, lesions, ctsses, freq_map, band_width), enc_loss(probs)


def chain_from_rows(rows):
    """intregaff.npz `<case>/chain` (scripts/make_golden_intreg.py:_chain_rows) -> the chain format of O.oneshot_chain."""
    chain = []
    for kind, a, b, c in (tuple(int(v) for v in r) for r in rows):
        if kind == 0:
            chain.append(("flip", tuple(ax for ax, on in zip((2, 3, 4), (a, b, c)) if on)))
        elif kind == 1:
            chain.append(("rot90", a, (b, c)))
        elif kind == 2:
            chain.append(("rescale", (a, b, c)))
        else:
            raise ValueError(f"unknown chain row {(kind, a, b, c)}")
    return chain


CHAIN_CLASS = {"flip": "Flip3DOneShot", "rot90": "Rotate903DOneShot", "rescale": "Rescale3DOneShot"}


def int_reg_aff_loss(model, chain, images, lobes, lesions, ctsses, freq_map, band_width=5e-2):
    """IntRegAffLoss.__call__ (metrics.py:245-308) for a GIVEN transform chain.  `model(images, lobes)` returns three
    outputs, the first is used.  Returns (reg, aff, enc)."""
    T = lambda key, x: O.oneshot_chain(chain, key, x)
    aff_images = T("#image", images)
    aff_lobes = T("#reference", lobes).contiguous()
    aff_lesions = T("#reference", lesions).contiguous()
    probs = torch.sigmoid(model(images, lobes)[0])
    reg = O.reg_loss_with_probs(probs, lobes, lesions, ctsses, freq_map, band_width)
    enc = enc_loss(probs)
    probs_T = T("#image", probs)
    aff_probs = torch.sigmoid(model(aff_images, aff_lobes)[0])
    aff_reg = O.reg_loss_with_probs(aff_probs, aff_lobes, aff_lesions, ctsses, freq_map, band_width)
    m = aff_lobes.expand_as(probs_T) > 0
    aff = F.smooth_l1_loss(probs_T[m], aff_probs[m])
    return (reg + aff_reg) / 2.0, aff, enc


def aff_standin(theta):
    """The closed-form 3-output stand-in model of the affine fixtures (scripts/make_golden_intreg.py, the one of
    oracle/make_golden.py:gen_affloss): smooth, position-dependent functions of the input and three scalar parameters.
    Test scaffolding written with torch ops, on whatever device and in whatever precision `theta` has."""
    def model(imgs, lbs):
        a, b, c = theta[0], theta[1], theta[2]
        D, H, W = imgs.shape[-3:]
        rz = torch.linspace(0.0, 1.0, D, dtype=imgs.dtype, device=imgs.device).view(1, 1, D, 1, 1)
        rx = torch.linspace(0.0, 1.0, W, dtype=imgs.dtype, device=imgs.device).view(1, 1, 1, 1, W)
        dense = a * (imgs - 0.5) * 4.0 + b + 0.6 * c * rx - 0.4 * rz
        refined = 0.7 * dense - c * imgs
        cls = torch.cat([a * imgs + rz, imgs * imgs + b * c * rx], dim=1)
        return dense, refined, cls
    return model
