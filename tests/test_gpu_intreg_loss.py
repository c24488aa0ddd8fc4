"""GPU parity of the losses without the pseudo-label refinement, DeviceIntRegLoss and DeviceIntRegAffLoss
(dram_amd/train_step.py; kernels dram_intreg_enc_loss_* of csrc/loss.hip): against the reference's own results
(tests/golden/intreg.npz, intregaff.npz), against the fp64 restatement that tests/test_intreg_loss_cpu.py pins to the same
files, and inside one DataParallelTrainer step of the slim DC3D.  The bounds are those tests/test_gpu_train_step.py holds
the Refine losses to."""
import os
import random

import numpy as np
import pytest
import torch

from intreg_restatement import aff_standin, int_reg_loss
from oracle import dram_oracle as O
from dram_amd.configs import SLIM

pytestmark = pytest.mark.gpu
FREQ = {k: 1.0 / 6 for k in range(6)}
BAND = 5e-2
AFF_CASES = ["all3", "all3b", "fliprot", "rescale", "rotrescale", "none"]


def _random_case(n, shape, scale, seed=11):
    g = torch.Generator().manual_seed(seed)
    dense = torch.randn((n, 1) + shape, generator=g) * scale
    lobes = (torch.rand((n, 1) + shape, generator=g) > 0.4).float()
    lobes.view(n, -1)[:, 0] = 1.0          # every sample has an inside ...
    lobes.view(n, -1)[:, -1] = 0.0         # ... and an outside voxel
    lesions = ((torch.rand((n, 1) + shape, generator=g) > 0.5) & (lobes > 0)).float()
    images = torch.rand((n, 1) + shape, generator=g)
    ctss = [float(i % 6) for i in range(n)]
    return dense, lobes, lesions, images, ctss


def test_intreg_loss_matches_reference_golden(golden_dir):
    """tests/golden/intreg.npz was produced by the reference's IntRegLoss (scripts/make_golden_intreg.py); its logits reach
    far beyond fp32 sigmoid saturation on both sides."""
    from dram_amd.train_step import Batch, DeviceIntRegLoss
    z = np.load(os.path.join(golden_dir, "intreg.npz"))
    t = lambda k: torch.from_numpy(z[k]).cuda()
    batch = Batch(t("images"), t("lobes"), t("lesions"), list(z["ctss"]), FREQ, band_width=BAND)
    dense = t("dense").requires_grad_(True)
    reg, enc = DeviceIntRegLoss(BAND)(dense, batch)
    print("reg", reg.item(), float(z["reg"]), "enc", enc.item(), float(z["enc"]))
    assert abs(reg.item() - float(z["reg"])) <= 1e-5 * max(1.0, abs(float(z["reg"])))
    assert abs(enc.item() - float(z["enc"])) <= 1e-5 * max(1.0, abs(float(z["enc"])))
    (2.0 * reg + 1.0 * enc).backward()
    ref = z["gdense"]
    err = np.abs(dense.grad.cpu().numpy() - ref).max() / np.abs(ref).max()
    print("gdense rel err", err)
    assert np.isfinite(dense.grad.cpu().numpy()).all()
    assert err <= 1e-4


# (n, shape, scale): S odd (the one-float path), S a multiple of 4 (16-byte loads), one row of 7; then shapes whose samples
# span many blocks: 336 blocks per sample in one step each; S odd with more steps than the 1024 blocks a sample gets; and
# twelve samples whose 171 blocks each take two steps of 16-byte loads, the second one only partly filled
FP64_CASES = [(3, (9, 17, 23), 3.0), (5, (32, 32, 32), 1.0), (2, (1, 1, 7), 3.0), (2, (96, 112, 128), 1.0),
              (2, (97, 113, 127), 1.0), (12, (96, 96, 96), 2.0)]


@pytest.mark.parametrize("n,shape,scale", FP64_CASES)
def test_intreg_loss_matches_fp64_restatement(n, shape, scale):
    from dram_amd.train_step import Batch, DeviceIntRegLoss
    dense, lobes, lesions, images, ctss = _random_case(n, shape, scale)
    d64 = dense.double().requires_grad_(True)
    reg_r, enc_r = int_reg_loss(d64, lobes.double(), lesions.double(), ctss, FREQ, BAND)
    (2.0 * reg_r + enc_r).backward()
    batch = Batch(images.cuda(), lobes.cuda(), lesions.cuda(), ctss, FREQ, band_width=BAND)
    dg = dense.cuda().requires_grad_(True)
    reg, enc = DeviceIntRegLoss(BAND)(dg, batch)
    (2.0 * reg + enc).backward()
    ref = d64.grad.float().numpy()
    err = np.abs(dg.grad.cpu().numpy() - ref).max() / np.abs(ref).max()
    print((n, shape, scale), "reg", reg.item(), reg_r.item(), "enc", enc.item(), enc_r.item(), "grad rel err", err)
    assert reg_r.item() > 0
    assert abs(reg.item() - reg_r.item()) <= 2e-5 * max(1.0, abs(reg_r.item()))
    assert abs(enc.item() - enc_r.item()) <= 2e-5 * max(1.0, abs(enc_r.item()))
    assert err <= 1e-4
    # deterministic: a second evaluation gives the same bits, values and gradient
    d2 = dense.cuda().requires_grad_(True)
    reg2, enc2 = DeviceIntRegLoss(BAND)(d2, batch)
    (2.0 * reg2 + enc2).backward()
    assert reg2.item() == reg.item() and enc2.item() == enc.item()
    assert torch.equal(d2.grad, dg.grad)


@pytest.mark.parametrize("n,shape", [(3, (9, 17, 23)), (2, (16, 16, 32)), (2, (1, 1, 7))])
def test_intreg_loss_saturated_logits(n, shape):
    """Logits scaled far into saturation (randn * 30, plus the largest finite float of either sign): nothing non-finite
    comes out, and the values agree with the reference's expression evaluated by torch in fp32 on the CPU
    (compute_enc_loss's order of operations: 1 - p from the rounded p).  An fp64 evaluation is no yardstick here: where
    fp32 rounds p to 1 its gradient is exactly 0.  The gradient is compared too where a sample has a thousand voxels or
    more: two fp32 sigmoids may differ by one ulp, which next to saturation moves p (1 - p) by 6e-8 times d loss / d p, and
    in a lobe of three voxels d reg / d p is of order 1 while the largest gradient element is of order 1e-4, so the 1e-4
    bound would there measure the sigmoids' last bit and not the kernel."""
    from dram_amd.train_step import Batch, DeviceIntRegLoss
    dense, lobes, lesions, images, ctss = _random_case(n, shape, 30.0)
    dense.view(n, -1)[:, 1] = torch.finfo(torch.float32).max
    dense.view(n, -1)[:, 2] = -torch.finfo(torch.float32).max
    batch = Batch(images.cuda(), lobes.cuda(), lesions.cuda(), ctss, FREQ, band_width=BAND)
    dg = dense.cuda().requires_grad_(True)
    reg, enc = DeviceIntRegLoss(BAND)(dg, batch)
    (2.0 * reg + enc).backward()
    got = dg.grad.cpu()
    assert np.isfinite(reg.item()) and np.isfinite(enc.item()) and torch.isfinite(got).all()
    d32 = dense.clone().requires_grad_(True)
    reg_r, enc_r = int_reg_loss(d32, lobes, lesions, ctss, FREQ, BAND)
    (2.0 * reg_r + enc_r).backward()
    ref = d32.grad
    assert torch.isfinite(ref).all()
    print((n, shape), "reg", reg.item(), reg_r.item(), "enc", enc.item(), enc_r.item(),
          "grad abs err", (got - ref).abs().max().item(), "max|ref|", ref.abs().max().item())
    assert abs(reg.item() - reg_r.item()) <= 2e-5 * max(1.0, abs(reg_r.item()))
    assert abs(enc.item() - enc_r.item()) <= 2e-5 * max(1.0, abs(enc_r.item()))
    if dense[0].numel() >= 1000:
        assert (got - ref).abs().max().item() <= 1e-4 * ref.abs().max().item()


# 9x17x23 = 3519 voxels; 21x23x19 = 9177, an odd count past 8192: nine blocks per sample, the last one partly filled
@pytest.mark.parametrize("shape", [(9, 17, 23), (21, 23, 19)], ids=["9x17x23", "21x23x19"])
def test_intreg_loss_uses_refined_when_given(shape):
    """The reference takes the model's second output for both terms (metrics.py:206-209): with `refined` given, both follow
    it and `dense` gets no gradient."""
    from dram_amd.train_step import Batch, DeviceIntRegLoss
    dense, lobes, lesions, images, ctss = _random_case(3, shape, 2.0)
    refined = torch.randn(dense.shape, generator=torch.Generator().manual_seed(3)) * 2.0
    batch = Batch(images.cuda(), lobes.cuda(), lesions.cuda(), ctss, FREQ, band_width=BAND)
    r64 = refined.double().requires_grad_(True)
    reg_r, enc_r = int_reg_loss(r64, lobes.double(), lesions.double(), ctss, FREQ, BAND)
    (2.0 * reg_r + enc_r).backward()
    dg, rg = dense.cuda().requires_grad_(True), refined.cuda().requires_grad_(True)
    reg, enc = DeviceIntRegLoss(BAND)(dg, batch, refined=rg)
    (2.0 * reg + enc).backward()
    assert abs(reg.item() - reg_r.item()) <= 2e-5 * max(1.0, abs(reg_r.item()))
    assert abs(enc.item() - enc_r.item()) <= 2e-5 * max(1.0, abs(enc_r.item()))
    ref = r64.grad.float().numpy()
    assert np.abs(rg.grad.cpu().numpy() - ref).max() <= 1e-4 * np.abs(ref).max()
    assert dg.grad is None
    alone = DeviceIntRegLoss(BAND)(rg.detach(), batch)
    assert alone[0].item() == reg.item() and alone[1].item() == enc.item()


def test_trainer_step_with_intreg_loss_matches_oracle(golden_dir):
    """One optimisation step (forward, fused loss, backward, SGD) of the slim DC3D with loss_fn=DeviceIntRegLoss(), whole
    batch and as two micro-batches, against the oracle's forward and torch autograd on the CPU in fp64; built like
    test_trainer_step_matches_oracle.  'ln' normalises per sample and `enc` is a plain mean, so the two micro-batches must
    reproduce the whole-batch losses AND the whole-batch update."""
    import models
    from dram_amd.train_step import Batch, DataParallelTrainer, DeviceIntRegLoss
    z = np.load(os.path.join(golden_dir, "intreg.npz"))
    torch.manual_seed(5)
    m = models.DC3D(**SLIM, norm_method="ln")
    m.init(models.HeNorm(mode="fan_in"))
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    params, buffers = O.split_state_dict({k: v.double() for k, v in sd.items()})
    for p in params.values():
        p.requires_grad_(True)
    t = lambda k: torch.from_numpy(z[k])
    x = torch.zeros((6, 1, 16, 16, 16))
    x[..., 2:14, 2:14, 2:14] = t("images")
    lobes, lesions = torch.zeros_like(x), torch.zeros_like(x)
    lobes[..., 2:14, 2:14, 2:14] = t("lobes")
    lesions[..., 2:14, 2:14, 2:14] = t("lesions")
    ctss = list(z["ctss"])
    out = O.dc3d_forward(SLIM, params, buffers, x.double(), training=True, norm_method="ln")
    dense = out[0] if isinstance(out, (tuple, list)) else out
    reg_r, enc_r = int_reg_loss(dense, lobes.double(), lesions.double(), ctss, FREQ, BAND)
    (2.0 * reg_r + enc_r).backward()
    lr = 0.5
    expect = {k: (p.detach() - lr * p.grad).float() for k, p in params.items()}
    for micro in (None, 3):
        m.load_state_dict(sd)
        mg = m.cuda().train()
        tr = DataParallelTrainer(mg, torch.optim.SGD(mg.parameters(), lr=lr), loss_fn=DeviceIntRegLoss(BAND))
        batch = Batch(x.cuda(), lobes.cuda(), lesions.cuda(), ctss, FREQ, band_width=BAND)
        reg, enc = tr.step(batch, micro_batch=micro)
        print("micro", micro, "reg", reg.item(), reg_r.item(), "enc", enc.item(), enc_r.item())
        assert abs(reg.item() - reg_r.item()) <= 1e-4 * max(1.0, abs(reg_r.item()))
        assert abs(enc.item() - enc_r.item()) <= 1e-4 * max(1.0, abs(enc_r.item()))
        got = {k: v.detach().cpu() for k, v in mg.named_parameters()}
        for k, e in expect.items():
            step_ref = (e - sd[k]).abs().max().item()
            err = (got[k] - e).abs().max().item()
            assert err <= 2e-3 * step_ref + 1e-9, (micro, k, err, step_ref)
        m = m.cpu()


@pytest.mark.parametrize("case", AFF_CASES)
def test_intreg_aff_loss_matches_reference_golden(golden_dir, case):
    """DeviceIntRegAffLoss against the reference's IntRegAffLoss (tests/golden/intregaff.npz): the same `random` /
    `numpy.random` seeds draw the same chain (names checked), then the three values and the gradients of the stand-in
    model's parameters, at the bounds of test_affine_consistency_loss_matches_reference_golden.  The stand-in is torch-op
    scaffolding; the OneShot transforms, the sigmoid, the hinge + entropy kernel and the masked smooth-L1 are the product's."""
    from dram_amd.train_step import Batch, DeviceIntRegAffLoss
    z = np.load(os.path.join(golden_dir, "intregaff.npz"))
    t = lambda k: torch.from_numpy(z[k]).cuda()
    batch = Batch(t("images"), t("lobes"), t("lesions"), list(z["ctss"]), FREQ, band_width=BAND)
    theta = t("theta").requires_grad_(True)
    seed = int(z[f"{case}/seed"])
    random.seed(seed)
    np.random.seed(seed)
    loss = DeviceIntRegAffLoss(rescale_jitter=[8, 10, 12, 14], band_width=BAND, freq_map=FREQ)
    drawn = {}
    orig = loss.get_affine_transform

    def spy():
        drawn["T"] = orig()
        return drawn["T"]
    loss.get_affine_transform = spy
    reg, aff, enc = loss(aff_standin(theta), batch)
    got_T = [type(x).__name__ for x in drawn["T"].p]
    want_T = [d for d in str(z[f"{case}/T"]).split("|") if d]
    assert got_T == want_T, (got_T, want_T)
    ref = z[f"{case}/out"]
    for name, g_, r_ in zip(("reg", "aff", "enc"), (reg, aff, enc), ref):
        assert abs(float(g_) - float(r_)) <= 2e-5 * max(1.0, abs(float(r_))), (case, name, float(g_), float(r_))
    (2.0 * reg + 0.5 * aff + 1.0 * enc).backward()
    gref = z[f"{case}/gtheta"]
    err = np.abs(theta.grad.cpu().numpy() - gref).max() / np.abs(gref).max()
    assert err <= 1e-4, (case, err, theta.grad.tolist(), gref.tolist())
