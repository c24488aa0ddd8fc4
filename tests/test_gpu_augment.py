"""The training augmentation pool on the device (dram_amd/augment.py over csrc/augment.hip) against the reference's own
outputs (tests/golden/augment.npz, scripts/make_golden_augment.py).  Every case is a batch with different parameters per sample
and one inactive sample, which must come back bit-identical."""
import math
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from dram_amd import augment as A

pytestmark = pytest.mark.gpu
ODD, CUBE = (12, 10, 14), (12, 12, 12)
MASK_KW = dict(times=5, region_size=((0.1, 0.5), (0.1, 0.5), (0.1, 0.5)))
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "augment.npz"))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sample(gold, which, five_d=False):
    x, m = dev(gold[which]), dev(gold[which + "_mask"])
    if five_d:
        x, m = x.unsqueeze(1), m.unsqueeze(1)
    return {"#image": x, "#lobe_reference": m, "meta": {"k": 1}}


def _same(t, a):
    return torch.equal(t.reshape(a.shape).cpu(), torch.from_numpy(np.ascontiguousarray(a)))


# ---------------------------------------------------------------------------------------------------- flip, rotate, mask-out
@pytest.mark.parametrize("five_d", [False, True])
def test_flip_equals_reference(gold, five_d):
    s = _sample(gold, "odd", five_d)
    params = [{"flip_axis": int(a)} for a in gold["flip/flip_axis"]] + [None]
    out = A.RandomFlip(3).apply(s, params)
    assert out["#image"].shape == s["#image"].shape and out["#lobe_reference"].dtype == torch.uint8
    assert out["meta"] is s["meta"]
    for k in range(3):
        assert _same(out["#image"][k], gold["flip/out"][k])
        assert _same(out["#lobe_reference"][k], gold["flip/mask_out"][k])
    assert torch.equal(out["#image"][3], s["#image"][3]) and torch.equal(out["#lobe_reference"][3], s["#lobe_reference"][3])


def test_every_flip_axis(gold):
    x = dev(gold["odd"][0:1]).expand(4, *ODD).contiguous()
    out = A.RandomFlip(3).apply({"#image": x}, [{"flip_axis": -1}, {"flip_axis": -2}, None, {"flip_axis": -3}])["#image"]
    for k, j in ((0, 0), (1, 1), (3, 2)):
        assert _same(out[k], gold["flip_all/out"][j])
    assert torch.equal(out[2], x[2])


@pytest.mark.parametrize("five_d", [False, True])
def test_rotate_equals_reference(gold, five_d):
    s = _sample(gold, "cube", five_d)
    params = [{"rotate_axis": tuple(int(v) for v in a), "rotate_times": int(k)}
              for a, k in zip(gold["rotate/rotate_axis"], gold["rotate/rotate_times"])] + [None]
    out = A.RandomRotate90(3).apply(s, params)
    want_m = gold["rotate/mask_out"] if "rotate/mask_out" in gold.files else gold["cube_mask"]
    for k in range(3):
        assert _same(out["#image"][k], gold["rotate/out"][k])
        assert _same(out["#lobe_reference"][k], want_m[k])
    assert torch.equal(out["#image"][3], s["#image"][3]) and torch.equal(out["#lobe_reference"][3], s["#lobe_reference"][3])


def test_every_quarter_turn(gold):
    n = len(gold["rotate_all/times"])
    x = dev(gold["cube"][0:1]).expand(n + 1, *CUBE).contiguous()
    m = dev(gold["cube_mask"][0:1]).expand(n + 1, *CUBE).contiguous()
    params = [{"rotate_axis": tuple(int(v) for v in a), "rotate_times": int(k)}
              for a, k in zip(gold["rotate_all/axis"], gold["rotate_all/times"])] + [None]
    out = A.RandomRotate90(3).apply({"#image": x, "#m_reference": m}, params)
    for k in range(n):
        assert _same(out["#image"][k], gold["rotate_all/out"][k]), params[k]
        assert _same(out["#m_reference"][k], gold["rotate_all/mask_out"][k]), params[k]
    assert torch.equal(out["#image"][n], x[n]) and torch.equal(out["#m_reference"][n], m[n])


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8])
def test_moves_on_shapes_of_many_tiles(dtype):
    """Shapes that span several tiles with ragged edges, against torch.flip / torch.rot90 on the host."""
    g = torch.Generator().manual_seed(3)
    for shape, params in [
        ((40, 33, 70), [{"flip_axis": -1}, {"flip_axis": -2}, None, {"flip_axis": -3}]),
        ((37, 37, 37), [{"rotate_axis": (-1, -2), "rotate_times": 1}, None, {"rotate_axis": (-1, -3), "rotate_times": 3},
                        {"rotate_axis": (-2, -3), "rotate_times": 1}, {"rotate_axis": (-1, -3), "rotate_times": 2}]),
        ((70, 33, 70), [{"rotate_axis": (-1, -3), "rotate_times": 1}, None, {"rotate_axis": (-1, -3), "rotate_times": 3}]),
    ]:
        n = len(params)
        x = (torch.rand((n, 2) + shape, generator=g) * 200).to(dtype)
        aug = A.RandomFlip(3) if "flip_axis" in params[0] else A.RandomRotate90(3)
        out = aug.apply({"#x": x.cuda()}, params)["#x"].cpu()
        for k, p in enumerate(params):
            if p is None:
                want = x[k]
            elif "flip_axis" in p:
                want = torch.flip(x[k], (p["flip_axis"],))
            else:
                want = torch.rot90(x[k], p["rotate_times"], p["rotate_axis"])
            assert torch.equal(out[k], want), (shape, p)


def test_maskout_equals_reference(gold):
    s = _sample(gold, "odd")
    params = [{"mask_centers": gold["maskout/mask_centers"][k].tolist(), "mask_sizes": gold["maskout/mask_sizes"][k].tolist(),
               "u": gold["maskout/u"][k].tolist()} for k in range(3)] + [None]
    params = [params[0], params[3], params[1], params[2]]          # the inactive sample in the middle
    x = s["#image"][[0, 3, 1, 2]].contiguous()
    out = A.RandomMaskOut(**MASK_KW).apply({"#image": x, "#lobe_reference": s["#lobe_reference"]}, params)
    assert out["#lobe_reference"] is s["#lobe_reference"]
    for k, j in ((0, 0), (2, 1), (3, 2)):
        assert not np.array_equal(gold["maskout/out"][j], gold["odd"][j])
        assert _same(out["#image"][k], gold["maskout/out"][j])
    assert torch.equal(out["#image"][1], x[1])


def test_maskout_scalar_path_and_empty_boxes():
    """A width that is no multiple of 4 (element-wise kernel), clipped and empty boxes, against the slices spelt in numpy."""
    rng = np.random.default_rng(0)
    shape = (9, 11, 13)
    x = (rng.random((3,) + shape) * 300 - 100).astype(np.float32)
    p = {"mask_centers": [(1, 9, 6), (4, 5, 12), (8, 0, 0), (3, 3, 3), (4, 4, 4)],
         "mask_sizes": [(5, 6, 3), (3, 0, 4), (4, 4, 4), (1, 1, 1), (0, 0, 0)], "u": [0.1, 0.5, 0.9, 0.25, 0.75]}
    out = A.RandomMaskOut().apply({"#image": dev(x)}, [p, None, p])["#image"].cpu().numpy()
    for k in (0, 2):
        want, lo, hi = x[k].copy(), x[k].min(), x[k].max()
        for c, sz, u in zip(p["mask_centers"], p["mask_sizes"], p["u"]):
            sl = tuple(slice(max(0, ci - si // 2), min(ci + (si - si // 2), d)) for ci, si, d in zip(c, sz, shape))
            want[sl] = float(lo) + (float(hi) - float(lo)) * u
        assert np.array_equal(out[k], want)
    assert np.array_equal(out[1], x[1])


def test_minmax_is_exact():
    g = torch.Generator().manual_seed(1)
    for shape in [(5, 3, 5, 7), (4, 1, 12, 10, 14), (3, 64, 64, 64)]:
        x = ((torch.rand(shape, generator=g) - 0.3) * 1000).cuda()
        mm = A.sample_minmax(x)
        flat = x.reshape(shape[0], -1)
        assert torch.equal(mm[:, 0], flat.amin(1)) and torch.equal(mm[:, 1], flat.amax(1))
        assert torch.equal(A.sample_minmax(x), mm)


# ------------------------------------------------------------------------------------------------------------------ blur
@pytest.mark.parametrize("tag, which", [("blur", "odd"), ("blur_wide", "cube")])
def test_blur_matches_reference(gold, tag, which):
    """Bound 2e-6 for inputs in [0, 1]: three passes of at most 5 taps (7 fp32 roundings each) against scipy's
    fp64-accumulate-then-round give at most 3 * 7 * 2^-24 = 1.25e-6.  (`blur_wide` has up to 9 taps: 3 * 11 * 2^-24 = 2e-6.)"""
    s = _sample(gold, which)
    params = [{"sigma": float(v)} for v in gold[f"{tag}/sigma"]]
    params = [params[0], None, params[1], params[2]]
    x = s["#image"][[0, 3, 1, 2]].contiguous()
    out = A.GaussianBlur((0.3, 0.5), "random").apply({"#image": x, "#lobe_reference": s["#lobe_reference"]}, params)
    assert out["#lobe_reference"] is s["#lobe_reference"]
    for k, j in ((0, 0), (2, 1), (3, 2)):
        err = np.abs(out["#image"][k].cpu().numpy().astype(np.float64) - gold[f"{tag}/out"][j]).max()
        print(f"{tag} sigma {params[k]['sigma']:.4f} radius {A.blur_radius(params[k]['sigma'])}: max abs err {err:.3e}")
        assert err <= 2e-6
    assert torch.equal(out["#image"][1], x[1])


def test_blur_on_a_shape_of_many_tiles():
    """Several tiles per axis with ragged edges, every radius 0..4 in one batch, against scipy on the host."""
    from scipy import ndimage
    rng = np.random.default_rng(5)
    x = rng.random((6, 37, 21, 70)).astype(np.float32)
    sigmas = [0.1, 0.3, 0.5, None, 0.8, 1.1]
    out = A.GaussianBlur((0.3, 0.5)).apply({"#image": dev(x)}, [None if s is None else {"sigma": s} for s in sigmas])["#image"]
    out = out.cpu().numpy()
    for k, s in enumerate(sigmas):
        if s is None:
            assert np.array_equal(out[k], x[k])
            continue
        err = np.abs(out[k].astype(np.float64) - ndimage.gaussian_filter(x[k], s)).max()
        print(f"sigma {s} radius {A.blur_radius(s)}: max abs err {err:.3e}")
        assert err <= 2e-6


# ----------------------------------------------------------------------------------------------------------------- noise
def test_noise_arithmetic_matches_reference(gold):
    """With the reference's own fp64 noise: bound 2^-21 * max(|min|, |max|, range), i.e. eight fp32 roundings."""
    s = _sample(gold, "odd")
    params = [{"sigma": float(gold["noise/sigma"][k]), "seed": 0, "noise": dev(gold["noise/noise"][k])} for k in range(3)]
    params = [params[0], params[1], None, params[2]]
    x = s["#image"][[0, 1, 3, 2]].contiguous()
    out = A.GaussianAddictive((0.01, 0.02), None).apply({"#image": x}, params)["#image"]
    for k, j in ((0, 0), (1, 1), (3, 2)):
        lo, hi = float(gold["odd"][j].min()), float(gold["odd"][j].max())
        bound = 2.0 ** -21 * max(abs(lo), abs(hi), hi - lo)
        err = np.abs(out[k].cpu().numpy().astype(np.float64) - gold["noise/out"][j]).max()
        print(f"noise sample {j}: max abs err {err:.3e} (bound {bound:.3e})")
        assert err <= bound
    assert torch.equal(out[2], x[2])


def test_in_kernel_noise_is_a_function_of_seed_and_element():
    g = torch.Generator().manual_seed(2)
    x = torch.rand((4, 12, 10, 14), generator=g).cuda()
    aug = A.GaussianAddictive((0.01, 0.02), None)
    p = [{"sigma": 0.02, "seed": 7}, {"sigma": 0.02, "seed": 8}, None, {"sigma": 0.015, "seed": 7}]
    a = aug.apply({"#image": x}, p)["#image"]
    b = aug.apply({"#image": x}, p)["#image"]
    assert torch.equal(a, b) and torch.equal(a[2], x[2])
    c = aug.apply({"#image": x}, [{"sigma": 0.02, "seed": 9}] + p[1:])["#image"]
    assert not torch.equal(c[0], a[0]) and torch.equal(c[1:], a[1:])
    # the same seed on another position of the batch and in a batch of another size: the same noise for the same data
    d = aug.apply({"#image": x[[1, 0]].contiguous()}, [None, p[0]])["#image"]
    assert torch.equal(d[1], a[0])
    # two samples with the same data and different seeds differ
    e = aug.apply({"#image": x[[0, 0, 0]].contiguous()}, [p[0], p[1], None])["#image"]
    assert not torch.equal(e[0], e[1]) and torch.equal(e[0], a[0])
    # a length that is no multiple of 4 takes the element-wise path: same values where the data agree
    y = torch.rand((3, 5, 7, 9), generator=g).cuda()
    q = [{"sigma": 0.02, "seed": 11}, None, {"sigma": 0.02, "seed": 12}]
    f1 = aug.apply({"#image": y}, q)["#image"]
    assert torch.equal(f1[1], y[1]) and torch.isfinite(f1).all() and not torch.equal(f1[0], y[0])


def test_in_kernel_noise_statistics():
    """Constant 0.5 with the range pinned to [0, 1] (no clamping at sigma 0.02): the recovered noise of n = 2^20 elements has
    |mean| <= 5 sigma / sqrt(n), |std / sigma - 1| <= 5 / sqrt(2n), and lag-1 correlation along x within 5 / sqrt(n)."""
    sigma, shape = 0.02, (3, 64, 128, 128)
    n = shape[1] * shape[2] * shape[3]
    assert n >= 10 ** 6
    x = torch.full(shape, 0.5, device="cuda")
    minmax = torch.tensor([[0.0, 1.0]] * 3, device="cuda")
    y = A.gaussian_noise(x, minmax, [sigma] * 3, [123456789, 2 ** 62 + 5, 3])
    base = np.float32(0.5) / np.float32(np.float32(1.0) + np.float32(1e-7))
    assert float(y.min()) > 0.0 and float(y.max()) < 1.0
    for k in range(3):
        z = y[k].cpu().numpy().astype(np.float64) - float(base)
        mean, std = z.mean(), z.std()
        zc = z - mean
        lag1 = (zc[..., 1:] * zc[..., :-1]).mean() / z.var()
        print(f"sample {k}: mean {mean:.3e} (bound {5 * sigma / math.sqrt(n):.3e}), std/sigma-1 {std / sigma - 1:.3e} "
              f"(bound {5 / math.sqrt(2 * n):.3e}), lag-1 {lag1:.3e} (bound {5 / math.sqrt(n):.3e})")
        assert abs(mean) <= 5 * sigma / math.sqrt(n)
        assert abs(std / sigma - 1) <= 5 / math.sqrt(2 * n)
        assert abs(lag1) <= 5 / math.sqrt(n)
    assert not torch.equal(y[0], y[1])


# -------------------------------------------------------------------------------------------------------------- ensemble
def test_ensemble_equals_sample_by_sample(gold):
    random.seed(41)
    np.random.seed(41)
    x = torch.cat([dev(gold["cube"]), dev(gold["cube"]).flip(0) * 0.5 + 0.25]).unsqueeze(1)
    m = torch.cat([dev(gold["cube_mask"]), dev(gold["cube_mask"]).flip(1)]).unsqueeze(1)
    sample = {"#image": x, "#lobes_reference": m, "#lesions_reference": m.float(), "meta": {"a": 1}}
    aug = A.EnsembleScanAugmentation(1.0)
    chains = aug.draw(8, CUBE)
    assert all(len(c) == 5 for c in chains) and len({tuple(n) for n in aug.chain_names(chains)}) > 1
    keep = {k: v.clone() for k, v in sample.items() if "#" in k}
    out = aug.apply(sample, chains)
    assert out["meta"] is sample["meta"]
    for k, v in keep.items():
        assert torch.equal(sample[k], v)                    # the input is not written
    for i, chain in enumerate(chains):
        one = {k: v[i:i + 1].contiguous() for k, v in keep.items()}
        for t, p in chain:
            one = t.apply(one, [p])
        for k in keep:
            assert out[k].dtype == keep[k].dtype and torch.equal(out[k][i:i + 1], one[k]), (i, k, aug.chain_names(chains)[i])
    # chains of different lengths, an empty one included
    chains2 = [c[:j % 6] for j, c in enumerate(chains)]
    out2 = aug.apply(sample, chains2)
    for i, chain in enumerate(chains2):
        one = {k: v[i:i + 1].contiguous() for k, v in keep.items()}
        for t, p in chain:
            one = t.apply(one, [p])
        for k in keep:
            assert torch.equal(out2[k][i:i + 1], one[k]), (i, k)


def test_ensemble_ratio_zero_returns_the_input():
    x = torch.rand((3, 1, 12, 12, 12), device="cuda")
    m = torch.zeros((3, 1, 12, 12, 12), dtype=torch.uint8, device="cuda")
    sample = {"#image": x, "#m_reference": m, "meta": {}}
    out = A.EnsembleScanAugmentation(0)(sample)
    assert out["#image"] is x and out["#m_reference"] is m


# ------------------------------------------------------------------------------------------------------------ end to end
_CHILD = r"""
import os, random, sys
sys.path[:0] = [ROOT, os.path.join(ROOT, "bodyct-dram_amd")]
import numpy as np
import torch
import models
from dram_amd.configs import SLIM
from dram_amd.train_step import DataParallelTrainer, synthetic_batch


def step(augment):
    torch.manual_seed(5)
    m = models.DC3D(**SLIM)
    m.init(models.HeNorm(mode="fan_in"))
    m = m.cuda().train()
    tr = DataParallelTrainer(m, torch.optim.SGD(m.parameters(), lr=1e-3))
    batch = synthetic_batch(4, 32, 7, torch.device("cuda"))
    if augment is not None:
        batch = batch.augmented(augment)
    reg, seg = tr.step(batch)
    return float(reg), float(seg)


before = step(None)
assert "dram_amd.augment" not in sys.modules
from dram_amd import augment as A
after = step(None)
print("plain", before, after)
assert before == after, (before, after)
random.seed(3)
np.random.seed(3)
aug = A.EnsembleScanAugmentation(1.0)
got = step(aug)
print("augmented", got)
assert all(np.isfinite(got)) and got != before
print("CHILD-OK")
"""


def test_trainer_step_on_an_augmented_batch():
    """One DataParallelTrainer.step on an augmented synthetic_batch(4, 32, ...) gives finite losses, and the un-augmented step's
    losses are bit-identical before and after `dram_amd.augment` is imported (a fresh process, so that 'before' is true)."""
    r = subprocess.run([sys.executable, "-c", "ROOT = %r\n%s" % (ROOT, _CHILD)], capture_output=True, text=True, timeout=900)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0 and "CHILD-OK" in r.stdout
