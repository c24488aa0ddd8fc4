"""CPU checks of the fp64 restatement of BootBinCrossEntropy and BinaryCrossEntropySmooth (tests/seg_loss_restatement.py),
which the GPU tests hold the kernels to: against torch's fp64 evaluation of oracle.dram_oracle.boot_bce, against a direct
torch transcription of BinaryCrossEntropySmooth, against the reference's own classes (tests/golden/segloss.npz, written by
scripts/make_golden_segloss.py), and the derivation the one-pass kernels rest on."""
import os

import numpy as np
import pytest
import torch

import seg_loss_restatement as R
from seg_loss_restatement import torch_bce_smooth
from oracle import dram_oracle as O

CASES = ["mixed", "rare", "common", "noinside"]


def _case(seed, n=997, voi_share=0.6, t_share=0.4, binary=True):
    g = torch.Generator().manual_seed(seed)
    p = torch.sigmoid(torch.randn(n, generator=g, dtype=torch.float64) * 3.0)
    p[:4] = torch.tensor([1e-9, 1.0 - 1e-9, 3e-7, 1.0 - 3e-7], dtype=torch.float64)
    voi = (torch.rand(n, generator=g, dtype=torch.float64) < voi_share).double()
    t = torch.rand(n, generator=g, dtype=torch.float64)
    t = ((t < t_share).double() if binary else t) * voi
    return p, t, voi


def _autograd(fn, p, *rest):
    p = p.clone().requires_grad_(True)
    loss = fn(p, *rest)
    loss.backward()
    return loss.item(), p.grad.numpy()


@pytest.mark.parametrize("seed,voi_share,t_share,smoothing", [(1, 0.6, 0.4, 0.1), (2, 0.5, 0.02, 0.3), (3, 0.7, 0.97, 0.0),
                                                              (4, 0.3, 0.5, 1.0)])
def test_boot_restatement_equals_oracle_fp64(seed, voi_share, t_share, smoothing):
    p, t, voi = _case(seed, voi_share=voi_share, t_share=t_share)
    ref, gref = _autograd(lambda q: O.boot_bce(q, t, voi, smoothing), p)
    got, ggot = R.boot_bce(p, t, voi, smoothing), R.boot_bce_grad(p, t, voi, smoothing)
    assert abs(got - ref) <= 1e-12 * abs(ref)
    assert np.abs(ggot - gref).max() <= 1e-12 * np.abs(gref).max()
    assert ((ggot == 0) == (gref == 0)).all()


@pytest.mark.parametrize("seed,t_share,smooth", [(1, 0.4, 1.0), (2, 0.02, 0.5), (3, 0.97, 2.0)])
def test_bce_smooth_restatement_equals_torch_fp64(seed, t_share, smooth):
    p, t, _ = _case(seed, voi_share=1.0, t_share=t_share)
    ref, gref = _autograd(lambda q: torch_bce_smooth(q, t, smooth), p)
    got, ggot = R.bce_smooth(p, t, smooth), R.bce_smooth_grad(p, t, smooth)
    assert abs(got - ref) <= 1e-12 * abs(ref)
    assert np.abs(ggot - gref).max() <= 1e-12 * np.abs(gref).max()
    assert ((ggot == 0) == (gref == 0)).all() and (ggot[:4] == 0).all() and (ggot[4:] != 0).all()


@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_reference_golden(golden_dir, case):
    """The reference's own classes, run in fp64 by scripts/make_golden_segloss.py."""
    z = np.load(os.path.join(golden_dir, "segloss.npz"))
    p, t, voi = z[f"{case}/p"], z[f"{case}/t"], z[f"{case}/voi"]
    s, sm = float(z[f"{case}/smoothing"]), float(z[f"{case}/smooth"])
    assert abs(R.boot_bce(p, t, voi, s) - float(z[f"{case}/boot"])) <= 1e-12 * abs(float(z[f"{case}/boot"]))
    assert np.abs(R.boot_bce_grad(p, t, voi, s) - z[f"{case}/gboot"]).max() <= 1e-12 * np.abs(z[f"{case}/gboot"]).max()
    assert abs(R.bce_smooth(p, t, sm) - float(z[f"{case}/bce"])) <= 1e-12 * abs(float(z[f"{case}/bce"]))
    assert np.abs(R.bce_smooth_grad(p, t, sm) - z[f"{case}/gbce"]).max() <= 1e-12 * np.abs(z[f"{case}/gbce"]).max()
    # and the oracle's expression agrees with the reference's class on the same inputs
    ref = O.boot_bce(torch.from_numpy(p), torch.from_numpy(t), torch.from_numpy(voi), s).item()
    assert abs(ref - float(z[f"{case}/boot"])) <= 1e-12 * abs(ref)


def test_golden_cases_reach_both_alpha_clamps_and_the_empty_inside(golden_dir):
    z = np.load(os.path.join(golden_dir, "segloss.npz"))
    alphas = {}
    for case in CASES:
        sums = R.boot_bce_sums(z[f"{case}/p"], z[f"{case}/t"], z[f"{case}/voi"])
        alphas[case] = R.boot_bce_from_sums(sums, 0.1)[1] if sums[2] > 0 else None
    assert alphas["rare"] == 0.75 and alphas["common"] == 0.25 and 0.25 < alphas["mixed"] < 0.75 and alphas["noinside"] is None


@pytest.mark.parametrize("seed", [5, 6])
def test_weighted_sum_follows_from_the_sums_for_nonbinary_targets(seed):
    """sum nll w = alpha A + (1 - alpha) B and sum w = alpha T + (1 - alpha)(n_in - T) for any t, binary or not: w is affine
    in t and alpha depends on the sums alone.  This is what lets the forward be ONE pass."""
    p, t, voi = _case(seed, binary=False)
    assert ((t > 0) & (t < 1)).any()
    ins = voi > 0
    pi, ti = p[ins], t[ins]
    alpha = (1.0 - ti.sum() / ins.sum()).clamp(0.25, 0.75)
    w = alpha * ti + (1.0 - alpha) * (1.0 - ti)
    nll = -torch.log((pi * ti + (1.0 - pi) * (1.0 - ti)).clamp(1e-7, 1.0 - 1e-7))
    n_out, s_out, n_in, T, A, B, H = R.boot_bce_sums(p, t, voi)
    assert n_in == ins.sum().item() and n_out == (voi < 1e-7).sum().item()
    assert abs((nll * w).sum().item() - (alpha.item() * A + (1.0 - alpha.item()) * B)) <= 1e-12 * (nll * w).sum().item()
    assert abs(w.sum().item() - (alpha.item() * T + (1.0 - alpha.item()) * (n_in - T))) <= 1e-12 * w.sum().item()
    ref = O.boot_bce(p, t, voi, 0.2).item()
    assert abs(R.boot_bce(p, t, voi, 0.2) - ref) <= 1e-12 * abs(ref)
    _, gref = _autograd(lambda q: O.boot_bce(q, t, voi, 0.2), p)
    assert np.abs(R.boot_bce_grad(p, t, voi, 0.2) - gref).max() <= 1e-12 * np.abs(gref).max()


def test_empty_sets_match_torch():
    p, t, _ = _case(7, n=64)
    ones, zeros = torch.ones_like(p), torch.zeros_like(p)
    # no outside: torch's mean of an empty tensor is nan, the loss is nan, the gradient is the inside part's and finite
    ref, gref = _autograd(lambda q: O.boot_bce(q, t, ones, 0.1), p)
    assert np.isnan(ref) and np.isnan(R.boot_bce(p, t, ones, 0.1))
    got = R.boot_bce_grad(p, t, ones, 0.1)
    assert np.isfinite(gref).all() and np.abs(got - gref).max() <= 1e-12 * np.abs(gref).max()
    # no inside: the outside term alone (t is 0 there in any real call; the formula does not need it)
    t0 = torch.zeros_like(p)
    ref, gref = _autograd(lambda q: O.boot_bce(q, t0, zeros, 0.1), p)
    assert abs(R.boot_bce(p, t0, zeros, 0.1) - ref) <= 1e-12 * abs(ref)
    assert np.abs(R.boot_bce_grad(p, t0, zeros, 0.1) - gref).max() <= 1e-12 * np.abs(gref).max()
    assert abs(ref - (-torch.log((1.0 - p).clamp(1e-7, 1.0 - 1e-7))).mean().item()) <= 1e-12 * abs(ref)
    # nothing at all: nan from both losses
    e = torch.zeros(0, dtype=torch.float64)
    assert np.isnan(O.boot_bce(e, e, e, 0.1).item()) and np.isnan(R.boot_bce(e, e, e, 0.1))
    assert np.isnan(torch_bce_smooth(e, e, 1.0).item()) and np.isnan(R.bce_smooth(e, e, 1.0))


def test_abi_and_interface_without_a_gpu():
    """Signatures, argument errors of the C entry points (nothing is launched), the lazy names and the host-side checks."""
    import dram_amd
    from dram_amd import _lib, losses
    from dram_amd import functional as HF
    assert dram_amd.BootBinCrossEntropy is losses.BootBinCrossEntropy and "BootBinCrossEntropy" in dram_amd.__all__
    assert dram_amd.BinaryCrossEntropySmooth is losses.BinaryCrossEntropySmooth and "BinaryCrossEntropySmooth" in dram_amd.__all__
    assert losses.BootBinCrossEntropy().smoothing == 0.1 and losses.BinaryCrossEntropySmooth(0.5).smooth == 0.5
    chunk = _lib.lib.dram_seg_loss_chunk()
    assert chunk == 4096 and _lib.lib.dram_seg_loss_state_floats() >= 5
    assert _lib.lib.dram_seg_loss_ws_bytes(0) == 0
    assert _lib.lib.dram_seg_loss_ws_bytes(chunk + 1) == (8 + 2 * 7) * 8
    q = 64      # a non-null dummy: every call below must be refused before anything is launched
    fwd = lambda *a: _lib.lib.dram_boot_bce_fwd(*a)
    assert fwd(None, q, q, 2, 2, 10, 0.1, q, q, q, 1 << 20, None) == -1
    assert fwd(q, q, q, 2, 2, 10, 0.1, q, q, None, 1 << 20, None) == -1
    assert fwd(q, q, q, 2, 2, -1, 0.1, q, q, q, 1 << 20, None) == -1
    assert fwd(q, q, q, 1, 2, 10, 0.1, q, q, q, 1 << 20, None) == -1            # int16 is no mask kind
    assert fwd(q, q, q, 2, 2, 10, 0.1, q, q, q, 8, None) == -2                  # workspace too small
    assert fwd(None, None, None, 2, 0, 0, 0.1, None, None, None, 0, None) == 0  # n == 0: nothing to do
    assert _lib.lib.dram_boot_bce_bwd(q, q, None, 2, 2, 10, 0.1, q, q, q, None) == -1
    assert _lib.lib.dram_boot_bce_bwd(q, q, q, 2, 2, -5, 0.1, q, q, q, None) == -1
    assert _lib.lib.dram_bce_smooth_fwd(q, None, 2, 10, 1.0, q, q, q, 1 << 20, None) == -1
    assert _lib.lib.dram_bce_smooth_fwd(q, q, 2, -1, 1.0, q, q, q, 1 << 20, None) == -1
    assert _lib.lib.dram_bce_smooth_bwd(q, q, 2, 10, 1.0, q, q, None, None) == -1
    assert _lib.lib.dram_bce_smooth_bwd(None, None, 0, 0, 1.0, None, None, None, None) == 0
    with pytest.raises(_lib.DramHipError, match="null pointer"):
        _lib.call("dram_bce_smooth_bwd", q, q, 2, 10, 1.0, None, q, q, None)
    x = torch.rand(2, 1, 3, 3, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HF.boot_bce(x, x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        losses.BinaryCrossEntropySmooth(1.0)(x, x)
