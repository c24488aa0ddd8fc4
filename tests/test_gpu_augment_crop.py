"""RandomCrop and StandarizeChannel on the device (dram_amd/augment.py over csrc/crop.hip and csrc/augment.hip) against the
reference's own outputs (tests/golden/augment_crop.npz, scripts/make_golden_crop.py).

RandomCrop is bit-exact (np.array_equal): the pad values are minima and copies, the nearest-neighbour resample copies, and the
linear one is the oracle's fp64 lerps in the oracle's order.  StandarizeChannel is compared within a bound measured from the
data (test_standarize_channel)."""
import os
import random

import numpy as np
import pytest
import torch

from dram_amd import augment as A
from oracle import dram_oracle as O

pytestmark = pytest.mark.gpu
KEYS = ("crop_sizes_ratio", "crop_sizes", "offset", "shifted_center", "padding")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "augment_crop.npz"))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _params(gold, i):
    p = {k: gold[f"case{i}/{k}"].tolist() for k in KEYS}
    p["spacing"] = tuple(gold["spacing"].tolist())
    return p


def _batches(gold):
    """The fixture's cases grouped by shape: (case indices, x [N, D, H, W], lobe, parameters), one None entry appended (a copy of
    the first case's input that must come back untouched)."""
    by_shape = {}
    for i in range(int(gold["n_cases"])):
        by_shape.setdefault(tuple(gold[f"case{i}/shape"].tolist()), []).append(i)
    out = []
    for shape, idx in by_shape.items():
        x = np.stack([gold[f"case{i}/x"] for i in idx] + [gold[f"case{idx[0]}/x"]])
        lobe = np.stack([gold[f"case{i}/lobe"] for i in idx] + [gold[f"case{idx[0]}/lobe"]])
        out.append((idx, x, lobe, [_params(gold, i) for i in idx] + [None]))
    assert len(out) == 2
    return out


def _check(gold, idx, x, lobe, out):
    img, lab = out["#image"].cpu().numpy(), out["#lobe_reference"].cpu().numpy()
    img, lab = img.reshape(x.shape), lab.reshape(x.shape)
    assert img.dtype == np.float32 and lab.dtype == np.uint8
    for k, i in enumerate(idx):
        assert np.array_equal(img[k], gold[f"case{i}/out_image"]), i
        assert np.array_equal(lab[k], gold[f"case{i}/out_lobe"]), i
    assert np.array_equal(img[-1], x[-1]) and np.array_equal(lab[-1], lobe[-1])         # the None entry
    assert sum(not np.array_equal(img[k], x[k]) for k in range(len(idx))) >= len(idx) - 1   # all but the identity crop move


def test_equals_reference(gold):
    """Every fixture case with its recorded parameters, one batch per shape, [N, D, H, W] and [N, 1, D, H, W]."""
    aug = A.RandomCrop((0.5,) * 3, (0.4,) * 3)
    for idx, x, lobe, p in _batches(gold):
        meta = {"k": 1}
        out = aug.apply({"#image": dev(x), "#lobe_reference": dev(lobe), "other": 3, "meta": meta}, p)
        assert out["meta"] is meta and out["other"] == 3 and out["#image"].shape == x.shape
        _check(gold, idx, x, lobe, out)
        five = aug.apply({"#image": dev(x).unsqueeze(1), "#lobe_reference": dev(lobe).unsqueeze(1)}, p)
        assert five["#image"].shape == (x.shape[0], 1) + x.shape[1:]
        _check(gold, idx, x, lobe, five)


def test_unaligned_base(gold):
    """Input and output 4 bytes (fp32) or 1 byte (uint8) past a 16-byte boundary: the same bits."""
    aug = A.RandomCrop((0.5,) * 3, (0.4,) * 3)
    for idx, x, lobe, p in _batches(gold):
        got = {}
        for key, src in (("#image", x), ("#lobe_reference", lobe)):
            t = dev(src)
            store = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
            shifted = store[1:].view(t.shape)
            shifted.copy_(t)
            assert shifted.data_ptr() % 16 == t.element_size() and shifted.is_contiguous()
            v = shifted.unsqueeze(1)
            tables, flags = aug._tables(p, x.shape[1:], v.device), A._flags(p, v.device)
            sink = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
            y = sink[1:].view(v.shape)
            assert aug._launch_key(key, v, tables, flags, out=y) is y and y.data_ptr() % 16 == t.element_size()
            got[key] = y
        _check(gold, idx, x, lobe, got)


@pytest.mark.parametrize("mode", ["minimum", "constant", "edge"])
def test_multi_block_against_the_oracle(mode):
    """(33, 40, 47), N = 3, seeded draws with a wide setting (so that windows leave the chunk): several blocks per sample, rows
    that are no multiple of the 16-byte groups.  Reference: oracle.resample_itk of pad_crop, the host restatement that the
    fixture pins at the small shapes."""
    shape, spacing = (33, 40, 47), (1.25, 0.7, 0.8)
    rng = np.random.default_rng(11)
    x = rng.standard_normal((3,) + shape).astype(np.float32)
    w = rng.random((3,) + shape).astype(np.float32)
    lobe = rng.integers(0, 6, (3,) + shape).astype(np.uint8)
    aug = A.RandomCrop((0.9,) * 3, (0.45,) * 3, padding_mode=mode)
    np.random.seed(21)
    p = [dict(q, spacing=spacing) for q in aug.draw(3, shape)]
    windows = [A.crop_window(q, shape) for q in p]
    assert any(st < 0 for s, _ in windows for st in s) and any(st + sz > d for s, z in windows for st, sz, d in zip(s, z, shape))
    out = aug.apply({"#image": dev(x), "#lobe_reference": dev(lobe), "#weight_map": dev(w)}, p)
    for n in range(3):
        size = windows[n][1]
        req = [spacing[a] * (size[a] / shape[a]) for a in range(3)]
        for key, src, how in (("#image", x, "linear"), ("#lobe_reference", lobe, "nearest"), ("#weight_map", w, "nearest")):
            want = O.resample_itk(A.pad_crop(src[n], p[n], mode), spacing, req, shape, how)
            assert np.array_equal(out[key][n].cpu().numpy(), want), (n, key)


def test_ensemble_with_random_crop():
    """2 x 80^3 through the driver, compared with applying each sample's drawn chain to that sample alone."""
    random.seed(4)
    np.random.seed(4)
    rng = np.random.default_rng(6)
    x = dev(rng.random((2, 1, 80, 80, 80)).astype(np.float32))
    m = dev(rng.integers(0, 6, (2, 1, 80, 80, 80)).astype(np.uint8))
    aug = A.EnsembleScanAugmentation(1.0, pool=[A.RandomCrop((0.5,) * 3, (0.4,) * 3), A.RandomFlip(3)])
    chains = aug.draw(2, (80, 80, 80))
    names = aug.chain_names(chains)
    assert all(sorted(n) == ["RandomCrop", "RandomFlip"] for n in names)
    keep, keep_m = x.clone(), m.clone()
    out = aug.apply({"#image": x, "#lobe_reference": m, "meta": {"a": 1}}, chains)
    assert torch.equal(x, keep) and torch.equal(m, keep_m) and out["#lobe_reference"].dtype == torch.uint8
    for i, chain in enumerate(chains):
        one = {"#image": keep[i:i + 1].contiguous(), "#lobe_reference": keep_m[i:i + 1].contiguous()}
        for t, p in chain:
            one = t.apply(one, [p])
        assert not torch.equal(one["#image"], keep[i:i + 1])
        assert torch.equal(out["#image"][i:i + 1], one["#image"]), (i, names[i])
        assert torch.equal(out["#lobe_reference"][i:i + 1], one["#lobe_reference"]), (i, names[i])


def _stand64(a):
    a = a.astype(np.float64)
    return (a - a.mean()) / a.std()


def test_standarize_channel(gold):
    """Against the reference's recorded fp32 outputs.  The bound comes from the data: the largest absolute error of an fp64 numpy
    restatement against the recorded reference output on these inputs is measured here (3.8e-7, on a channel of the 4-d sample;
    2.6e-7 on the 3-d one: one to two fp32 steps at the outputs' magnitude of up to 2.6), and the device gets four times that
    (1.5e-6): the margin covers the reference's fp32 pairwise sums, and the device's fp64 sums land nearer the fp64
    restatement (measured on an MI355X: 2.4e-7 per sample and 4.8e-7 per channel against the reference, 1.9e-7 against fp64)."""
    x3, x4 = gold["stand/x3"], gold["stand/x4"]
    want3, want4 = gold["stand/out3"], gold["stand/out4"]
    ref3, ref4 = _stand64(x3), np.stack([_stand64(c) for c in x4])
    measured = max(np.abs(ref3 - want3).max(), np.abs(ref4 - want4).max())
    bound = 4 * measured
    print(f"fp64 restatement against the reference: {measured:.3e}; bound {bound:.3e}")
    assert 0 < measured < 1e-5
    aug = A.StandarizeChannel(0)
    lobe = dev(np.ones((2,) + x3.shape, dtype=np.uint8))
    # [N, D, H, W] and [N, 1, D, H, W], per sample; a None entry comes back untouched, other keys pass through
    batch = np.stack([x3, x4[1], x3])
    for t in (dev(batch), dev(batch).unsqueeze(1)):
        out = aug.apply({"#image": t, "#lobe_reference": lobe}, [{}, {}, None])
        assert out["#lobe_reference"] is lobe and out["#image"].shape == t.shape and out["#image"].dtype == torch.float32
        got = out["#image"].cpu().numpy().reshape(batch.shape)
        e3, e4 = np.abs(got[0] - want3).max(), np.abs(got[1] - want4[1]).max()
        print(f"device against the reference: {e3:.3e} {e4:.3e}; against fp64: {np.abs(got[0] - ref3).max():.3e}")
        assert e3 <= bound and e4 <= bound
        assert np.array_equal(got[2], x3)
    # [N, C, D, H, W] per (sample, channel)
    two = np.stack([x4, x4[::-1]])
    got = aug(dict({"#image": dev(two)}))["#image"].cpu().numpy()
    err = max(np.abs(got[0] - want4).max(), np.abs(got[1] - want4[::-1]).max())
    print(f"device per channel against the reference: {err:.3e}")
    assert err <= bound
    assert np.array_equal(got[0, 0], got[1, 2])                  # the same row gives the same bits wherever it stands
    with pytest.raises(NotImplementedError):
        A.StandarizeChannel(1).apply({"#image": dev(two)}, [{}, {}])
