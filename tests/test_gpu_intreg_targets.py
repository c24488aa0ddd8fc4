"""Regression targets on the device (csrc/loss.hip, dram_intreg_targets, through Batch.on_device) against the host path
of Batch.__init__ on 0/1 masks: the same bits for targets, weight and keep, in every case of the band logic, for a row
that takes one block and one that takes several, for rows that do and do not allow 16-byte loads."""
import numpy as np
import pytest
import torch

import targets_restatement as R

pytestmark = pytest.mark.gpu
FREQ = {0: 0.05, 1: 0.2, 2: 0.5, 3: 0.8, 4: 0.95, 5: 1.0 / 6}      # below, at, inside, at and above the clamp [0.2, 0.8]


def _masks(shape, ratios, seed):
    """The ellipsoid lobe of synthetic_batch; per sample the first round(ratio * lobe voxels) lobe voxels in a random
    order are lesion, and so is a random fifth of the OUTSIDE (which must not count).  0/1 floats, [N,1,D,H,W] on the device."""
    D, H, W = shape
    g = torch.Generator().manual_seed(seed)
    zz = (torch.arange(D, dtype=torch.float32) - (D - 1) / 2).view(D, 1, 1) / (0.45 * D)
    yy = (torch.arange(H, dtype=torch.float32) - (H - 1) / 2).view(1, H, 1) / (0.45 * H)
    xx = (torch.arange(W, dtype=torch.float32) - (W - 1) / 2).view(1, 1, W) / (0.45 * W)
    lobe = ((zz ** 2 + yy ** 2 + xx ** 2) < 1.0).float().reshape(-1)
    inside = torch.nonzero(lobe > 0).reshape(-1)
    n = len(ratios)
    lesions = torch.zeros((n, lobe.numel()))
    for i, r in enumerate(ratios):
        pick = inside[torch.randperm(inside.numel(), generator=g)[:int(round(r * inside.numel()))]]
        lesions[i, pick] = 1.0
        lesions[i] = torch.maximum(lesions[i], ((torch.rand(lobe.numel(), generator=g) < 0.2) & (lobe == 0)).float())
    lobes = lobe.view(1, 1, D, H, W).expand(n, 1, D, H, W).contiguous()
    images = torch.rand((n, 1, D, H, W), generator=g)
    return images.cuda(), lobes.cuda(), lesions.view(n, 1, D, H, W).cuda()


def _host_branches(lobes, lesions, ctss, band_width):
    s0 = (lesions * lobes).double().flatten(1).sum(1).cpu().numpy()
    s1 = lobes.double().flatten(1).sum(1).cpu().numpy()
    return R.band([int(c) for c in ctss], R.ratio(s0, s1), band_width)


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def _ctss_dev(ctss):
    return torch.tensor([int(c) for c in ctss], dtype=torch.int32).cuda()


CASES = {
    # one sample per score; 512 voxels: one block per row, 16-byte loads
    "n6_8x8x8": ((8, 8, 8), [0.0, 1.0, 2.0, 3.0, 4.0, 5.0], [0.0, 0.5, 0.03, 0.2, 0.1, 0.9], 5e-2),
    # 315 voxels: no multiple of 4, element loads
    "n3_5x7x9": ((5, 7, 9), [1.0, 4.0, 2.0], [0.5, 0.1, 0.02], 1e-2),
    # 64 000 voxels: 16 blocks per row, the partial combine
    "n2_40x40x40": ((40, 40, 40), [3.0, 0.0], [0.2, 0.3], 5e-2),
}


@pytest.mark.parametrize("case", list(CASES))
def test_on_device_equals_the_host_batch(case):
    from dram_amd.train_step import Batch
    shape, ctss, ratios, bw = CASES[case]
    images, lobes, lesions = _masks(shape, ratios, 7)
    want_t, branch = _host_branches(lobes, lesions, ctss, bw)
    if case == "n6_8x8x8":      # every case of the band logic, known on the host side before the device is asked
        assert {R.OVERLAP, R.BELOW, R.ABOVE} == set(branch.tolist()), branch
    else:
        assert len(set(branch.tolist())) >= 2, branch
    host = Batch(images, lobes, lesions, ctss, FREQ, band_width=bw)
    assert np.array_equal(_bits(host.targets), want_t.view(np.int32))        # the restatement describes the host path
    dev = Batch.on_device(images, lobes, lesions, _ctss_dev(ctss), FREQ, band_width=bw, ctss=ctss)
    torch.cuda.synchronize()
    assert dev.targets.shape == host.targets.shape and dev.weight.shape == host.weight.shape and dev.keep.shape == host.keep.shape
    assert dev.targets.dtype == dev.weight.dtype == dev.keep.dtype == torch.float32
    assert torch.equal(dev.targets, host.targets), (dev.targets.tolist(), host.targets.tolist())
    assert torch.equal(dev.weight, host.weight), (dev.weight.tolist(), host.weight.tolist())
    assert torch.equal(dev.keep, host.keep)
    assert dev.ctss == host.ctss and len(dev) == len(host)
    # the lazily uploaded scores of a host-built batch are what on_device takes, and micro-batches slice them
    again = Batch.on_device(images[1:], lobes[1:], lesions[1:], host.ctss_device()[1:], FREQ, band_width=bw, ctss=ctss[1:])
    assert torch.equal(again.targets, host.targets[1:]) and torch.equal(again.weight, host.weight[1:])
    assert host.micro(1, len(host))._ctss_dev.tolist() == [int(c) for c in ctss[1:]]


def test_empty_lobe_gives_nan_targets_for_that_sample_only():
    from dram_amd.train_step import Batch
    ctss = [2.0, 3.0, 4.0]
    images, lobes, lesions = _masks((8, 8, 8), [0.03, 0.2, 0.1], 9)
    lobes[1] = 0.0
    dev = Batch.on_device(images, lobes, lesions, _ctss_dev(ctss), FREQ, band_width=5e-2, ctss=ctss)
    others = [0, 2]
    host = Batch(images[others], lobes[others], lesions[others], [ctss[i] for i in others], FREQ, band_width=5e-2)
    assert torch.isnan(dev.targets[1]).all()
    assert torch.equal(dev.targets[others], host.targets) and torch.isfinite(dev.targets[others]).all()
    w, k = R.weight_keep([int(c) for c in ctss], FREQ)
    assert np.array_equal(_bits(dev.weight), w.view(np.int32)) and dev.keep.flatten().tolist() == k.tolist()


def test_two_launches_give_the_same_bits():
    from dram_amd import functional as HF
    shape, ctss, ratios, bw = CASES["n2_40x40x40"]
    _, lobes, lesions = _masks(shape, ratios, 7)
    c = _ctss_dev(ctss)
    fr = [FREQ[k] for k in range(6)]
    a = HF.intreg_targets(lobes, lesions, c, fr, bw)
    b = HF.intreg_targets(lobes, lesions, c, fr, bw)
    for x, y in zip(a, b):
        assert np.array_equal(_bits(x), _bits(y))
    # rows at an address that rules out 16-byte loads take the element kernel and add up to the same sums
    pad = torch.zeros(lobes.numel() + 1, device="cuda")
    off = lambda t: pad.clone()[1:].copy_(t.reshape(-1)).view_as(t)
    lo, le = off(lobes), off(lesions)
    assert lo.data_ptr() % 16 != 0 and lo.is_contiguous()
    d = HF.intreg_targets(lo, le, c, fr, bw)
    for x, y in zip(a, d):
        assert np.array_equal(_bits(x), _bits(y))
