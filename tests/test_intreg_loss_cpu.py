"""The fp64 restatement of IntRegLoss / IntRegAffLoss (tests/intreg_restatement.py) against the reference's own results
(tests/golden/intreg.npz, intregaff.npz; scripts/make_golden_intreg.py), and the properties of those fixtures that keep the
comparisons from passing vacuously.  No GPU needed; tests/test_gpu_intreg_loss.py holds the device losses to the same files
and, at other shapes, to this restatement."""
import os

import numpy as np
import pytest
import torch

from intreg_restatement import CHAIN_CLASS, aff_standin, chain_from_rows, int_reg_aff_loss, int_reg_loss
from oracle import dram_oracle as O

FREQ = {k: 1.0 / 6 for k in range(6)}
BAND = 5e-2
AFF_CASES = ["all3", "all3b", "fliprot", "rescale", "rotrescale", "none"]


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"))


def test_intreg_fixture_is_not_vacuous(golden_dir):
    """What scripts/make_golden_intreg.py asserts when it writes intreg.npz, checked on the committed file: lobe voxels in
    every sample, ctss 0..5, hinges active and inactive, logits on both sides of fp32 sigmoid saturation."""
    z = _load(golden_dir, "intreg")
    t = lambda k: torch.from_numpy(z[k])
    lobes, dense, ctss = t("lobes"), t("dense"), list(z["ctss"])
    N = dense.shape[0]
    assert all(float(lobes[n].sum()) > 0 for n in range(N))
    assert sorted(set(int(c) for c in ctss)) == [0, 1, 2, 3, 4, 5]
    per_sample = [O.reg_loss_with_probs(torch.sigmoid(dense[n:n + 1].double()), lobes[n:n + 1].double(), t("lesions")[n:n + 1].double(),
                                        ctss[n:n + 1], FREQ, BAND).item() for n in range(N)]
    assert any(v > 0 for v in per_sample) and any(v == 0 for v in per_sample), per_sample
    p = torch.sigmoid(dense)                # fp32
    assert (p == 1).any() and (p == 0).any() and ((p > 0) & (p < 1)).any()
    assert (dense > 17.4).any() and (dense < -17.4).any() and (dense.abs() < 17.4).any()
    assert np.isfinite(z["reg"]) and np.isfinite(z["enc"]) and np.isfinite(z["gdense"]).all()


def test_intregaff_fixture_is_not_vacuous(golden_dir):
    z = _load(golden_dir, "intregaff")
    assert list(z["cases"]) == AFF_CASES
    names = [[d for d in str(z[f"{c}/T"]).split("|") if d] for c in AFF_CASES]
    assert {n for chain in names for n in chain} == set(CHAIN_CLASS.values())
    assert [] in names
    for c, chain in zip(AFF_CASES, names):       # the two records of the chain agree
        assert [CHAIN_CLASS[op[0]] for op in chain_from_rows(z[f"{c}/chain"])] == chain
    assert all(float(l.sum()) > 0 for l in torch.from_numpy(z["lobes"]))


def test_restated_intreg_matches_reference_golden(golden_dir):
    """(reg, enc) and d(2 reg + enc)/d dense in fp64 against the reference's fp32 run.  Measured here: |reg - golden| 1.4e-7,
    |enc - golden| 4.3e-10, gradient 3.1e-7 of max|golden| -- far inside the project's bounds for the Refine loss
    (1e-5 max(1, |v|) and 1e-4 of max|ref|) although the fixture holds logits that saturate the fp32 sigmoid: the entropy
    term needs no looser bound."""
    z = _load(golden_dir, "intreg")
    t = lambda k: torch.from_numpy(z[k]).double()
    dense = t("dense").requires_grad_(True)
    reg, enc = int_reg_loss(dense, t("lobes"), t("lesions"), list(z["ctss"]), FREQ, BAND)
    print("reg", reg.item(), float(z["reg"]), "enc", enc.item(), float(z["enc"]))
    assert abs(reg.item() - float(z["reg"])) <= 1e-5 * max(1.0, abs(float(z["reg"])))
    assert abs(enc.item() - float(z["enc"])) <= 1e-5 * max(1.0, abs(float(z["enc"])))
    (2.0 * reg + 1.0 * enc).backward()
    ref = z["gdense"]
    err = np.abs(dense.grad.numpy() - ref).max() / np.abs(ref).max()
    print("gdense rel err", err)
    assert err <= 1e-4


@pytest.mark.parametrize("case", AFF_CASES)
def test_restated_intregaff_matches_reference_golden(golden_dir, case):
    """(reg, aff, enc) and the stand-in model's parameter gradients with the chain the reference drew, at the bounds of
    test_affine_consistency_oracle_matches_reference_golden."""
    z = _load(golden_dir, "intregaff")
    chain = chain_from_rows(z[f"{case}/chain"])
    t = lambda k: torch.from_numpy(z[k]).double()
    theta = t("theta").requires_grad_(True)
    reg, aff, enc = int_reg_aff_loss(aff_standin(theta), chain, t("images"), t("lobes"), t("lesions"), list(z["ctss"]), FREQ, BAND)
    for name, g_, r_ in zip(("reg", "aff", "enc"), (reg, aff, enc), z[f"{case}/out"]):
        assert abs(g_.item() - float(r_)) <= 2e-5 * max(1.0, abs(float(r_))), (case, name, g_.item(), float(r_))
    (2.0 * reg + 0.5 * aff + 1.0 * enc).backward()
    gref = z[f"{case}/gtheta"]
    err = np.abs(theta.grad.numpy() - gref).max() / np.abs(gref).max()
    assert err <= 1e-4, (case, err, theta.grad.tolist(), gref.tolist())


def test_device_intreg_losses_refuse_cpu_tensors(golden_dir):
    """No CPU / PyTorch fallback: the new losses raise on host tensors like every other op of the path."""
    from dram_amd.train_step import Batch, DeviceIntRegAffLoss, DeviceIntRegLoss
    z = _load(golden_dir, "intreg")
    t = lambda k: torch.from_numpy(z[k])
    batch = Batch(t("images"), t("lobes"), t("lesions"), list(z["ctss"]), FREQ, band_width=BAND)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DeviceIntRegLoss()(t("dense"), batch)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DeviceIntRegAffLoss([8, 10, 12, 14], freq_map=FREQ)(lambda im, lb: (t("dense"), None, None), batch)
