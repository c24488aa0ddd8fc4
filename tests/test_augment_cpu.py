"""CPU checks of the training augmentation pool's host side (dram_amd/augment.py): the draw sequences against the parameters
the reference drew under the same seeds (tests/golden/augment.npz, written by scripts/make_golden_augment.py), the blur weight
table against scipy's, and the argument errors of the C entry points (reported without a GPU)."""
import ctypes
import os
import random

import numpy as np
import pytest

from dram_amd import _lib
from dram_amd import augment as A

ODD, CUBE = (12, 10, 14), (12, 12, 12)
MASK_KW = dict(times=5, region_size=((0.1, 0.5), (0.1, 0.5), (0.1, 0.5)))


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "augment.npz"))


def _seed(s):
    random.seed(int(s))
    np.random.seed(int(s))


def _draws(gold, aug, shape):
    out = []
    for s in gold["seeds"]:
        _seed(s)
        out.append(aug.draw(1, shape)[0])
    return out


@pytest.mark.parametrize("tag, sigma, shape", [("blur", (0.3, 0.5), ODD), ("blur_wide", (0.3, 1.1), CUBE)])
def test_blur_draws(gold, tag, sigma, shape):
    got = _draws(gold, A.GaussianBlur(sigma, "random"), shape)
    assert [p["sigma"] for p in got] == list(gold[f"{tag}/sigma"])
    assert A.GaussianBlur((0.4, 0.5)).draw(2, shape) == [{"sigma": 0.4}] * 2       # mode 'fixed' draws nothing


@pytest.mark.parametrize("tag, kw, shape", [("maskout", MASK_KW, ODD), ("maskout_default", {}, CUBE)])
def test_maskout_draws(gold, tag, kw, shape):
    got = _draws(gold, A.RandomMaskOut(**kw), shape)
    for k, p in enumerate(got):
        assert np.array_equal(np.array(p["mask_centers"]), gold[f"{tag}/mask_centers"][k])
        assert np.array_equal(np.array(p["mask_sizes"]), gold[f"{tag}/mask_sizes"][k])
        assert p["u"] == list(gold[f"{tag}/u"][k])
    if tag == "maskout_default":        # int(0.05 * 12) == 0: every box of the default sizes is empty on a 12-voxel axis
        assert not np.any(gold[f"{tag}/mask_sizes"])
        rows = np.array(A.mask_boxes(got[0]["mask_centers"], got[0]["mask_sizes"], shape))
        assert np.all(rows[:, 1::2] <= rows[:, 0::2])


def test_flip_and_rotate_draws(gold):
    assert [p["flip_axis"] for p in _draws(gold, A.RandomFlip(3), ODD)] == list(gold["flip/flip_axis"])
    got = _draws(gold, A.RandomRotate90(3), CUBE)
    assert [p["rotate_times"] for p in got] == list(gold["rotate/rotate_times"])
    assert [list(p["rotate_axis"]) for p in got] == gold["rotate/rotate_axis"].tolist()


def test_noise_draws(gold):
    got = _draws(gold, A.GaussianAddictive((0.01, 0.02), None), ODD)
    assert [p["sigma"] for p in got] == list(gold["noise/sigma"])
    assert all(0 <= p["seed"] < 2 ** 63 for p in got) and len({p["seed"] for p in got}) == len(got)
    with pytest.raises(NotImplementedError):
        A.GaussianAddictive((0.01, 0.02), 1)


@pytest.mark.parametrize("ratio", [0.5, 1.0])
def test_ensemble_chains(gold, ratio):
    """The reference's chain of class names per seed: compared up to and including the first GaussianAddictive (host draws
    after it differ from the reference's by design), and as a whole when the chain has none."""
    aug = A.EnsembleScanAugmentation(ratio)
    assert len(gold["ensemble/seeds"]) >= 8
    for s, want in zip(gold["ensemble/seeds"], gold[f"ensemble/chains_{ratio}"]):
        _seed(s)
        got = A.EnsembleScanAugmentation.chain_names(aug.draw(1, CUBE))[0]
        want = [w for w in str(want).split(",") if w]
        cut = want.index("GaussianAddictive") + 1 if "GaussianAddictive" in want else len(want)
        assert got[:cut] == want[:cut]
        if cut == len(want):
            assert got == want
        # the order and the keep decisions of ONE sample are all drawn before any parameter: the whole chain agrees
        assert got == want


def test_ensemble_draws_samples_in_order():
    """A batch is drawn sample by sample: the first sample's chain and parameters are those of a batch of one."""
    aug = A.EnsembleScanAugmentation(1.0)
    _seed(5)
    one = aug.draw(1, CUBE)[0]
    _seed(5)
    many = aug.draw(3, CUBE)
    assert [(type(t).__name__, p) for t, p in many[0]] == [(type(t).__name__, p) for t, p in one]
    assert all(len(c) == 5 for c in many)
    _seed(5)
    assert A.EnsembleScanAugmentation(0).draw(4, CUBE) == [[]] * 4


@pytest.mark.parametrize("sigma", [0.3, 0.37, 0.499, 0.5, 0.8, 1.1])
def test_blur_weights_equal_scipy(sigma):
    from scipy.ndimage import _filters
    radius = int(4.0 * sigma + 0.5)
    want = _filters._gaussian_kernel1d(sigma, 0, radius)
    got = A.blur_weights(sigma)
    assert A.blur_radius(sigma) == radius and got.dtype == np.float64 and got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-15


def test_blur_weights_reproduce_the_filter(gold):
    """The table is what scipy applies: a float64 restatement with it (reflect, z then y then x, fp32 between passes) gives
    the golden's output bit for bit."""
    x, sigma = gold["odd"][0], float(gold["blur/sigma"][0])
    w, r = A.blur_weights(sigma), A.blur_radius(sigma)
    y = x
    for axis in range(3):
        pad = [(r, r) if a == axis else (0, 0) for a in range(3)]
        p = np.pad(y.astype(np.float64), pad, mode="symmetric")
        acc = np.zeros(y.shape)
        for j in range(2 * r + 1):
            acc += w[j] * np.take(p, np.arange(j, j + y.shape[axis]), axis=axis)
        y = acc.astype(np.float32)
    assert np.abs(y.astype(np.float64) - gold["blur/out"][0]).max() <= 2e-7


FAKE = ctypes.c_void_p(16)      # never dereferenced: the argument checks come first


def test_entries_refuse_null_pointers():
    for name, args in [
        ("dram_aug_minmax", (None, FAKE, None, 2, 64)),
        ("dram_aug_gaussian_blur", (FAKE, None, FAKE, FAKE, 2, 2, 2, 4, 4, 4)),
        ("dram_aug_mask_out", (FAKE, FAKE, None, FAKE, FAKE, FAKE, 2, 5, 2, 4, 4, 4)),
        ("dram_aug_gaussian_noise", (FAKE, FAKE, FAKE, None, None, FAKE, 2, None, 2, 64)),
        ("dram_aug_permute_flip", (FAKE, FAKE, 4, FAKE, FAKE, None, 2, 2, 1, 4, 4, 4)),
    ]:
        with pytest.raises(_lib.DramHipError, match="null pointer"):
            _lib.call(name, *args, None)


def test_blur_refuses_a_radius_above_the_limit():
    with pytest.raises(_lib.DramHipError, match=r"radius 5 outside the supported 0\.\.4"):
        _lib.call("dram_aug_gaussian_blur", FAKE, FAKE, FAKE, FAKE, 2, 5, 2, 4, 4, 4, None)
    with pytest.raises(ValueError, match="at most 4"):
        A.GaussianBlur((1.2, 1.2))._tables([{"sigma": 1.2}], CUBE, "cpu")


def test_entries_refuse_a_mismatched_table_length():
    for name, args in [
        ("dram_aug_gaussian_blur", (FAKE, FAKE, FAKE, FAKE, 3, 2, 2, 4, 4, 4)),
        ("dram_aug_mask_out", (FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 3, 5, 2, 4, 4, 4)),
        ("dram_aug_gaussian_noise", (FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 3, None, 2, 64)),
        ("dram_aug_permute_flip", (FAKE, FAKE, 4, FAKE, FAKE, FAKE, 3, 2, 1, 4, 4, 4)),
    ]:
        with pytest.raises(_lib.DramHipError, match="table length 3 does not match the batch of 2"):
            _lib.call(name, *args, None)


def test_entries_refuse_other_bad_arguments():
    with pytest.raises(_lib.DramHipError, match="17 boxes"):
        _lib.call("dram_aug_mask_out", FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 2, 17, 2, 4, 4, 4, None)
    with pytest.raises(_lib.DramHipError, match="element size 2"):
        _lib.call("dram_aug_permute_flip", FAKE, FAKE, 2, FAKE, FAKE, FAKE, 2, 2, 1, 4, 4, 4, None)
    with pytest.raises(_lib.DramHipError, match="in place"):
        _lib.call("dram_aug_gaussian_blur", FAKE, FAKE, FAKE, FAKE, 2, 2, 2, 4, 4, 4, None)


def test_odd_rotation_of_unequal_extents_is_refused():
    with pytest.raises(ValueError, match="unequal extents 14 x 10"):
        A.rotate_table((-1, -2), 1, ODD)
    with pytest.raises(ValueError, match="unequal extents"):
        A.RandomRotate90(3)._tables([None, {"rotate_axis": (-2, -3), "rotate_times": 3}], ODD, "cpu")
    assert A.rotate_table((-1, -2), 2, ODD) == ((0, 1, 2), (0, 1, 1))       # a half turn keeps the shape
    assert A.rotate_table((-1, -2), 0, ODD) == ((0, 1, 2), (0, 0, 0))
    assert A.rotate_table((-1, -3), 1, (12, 10, 12))[0] == (2, 1, 0)        # equal extents in the plane are enough
