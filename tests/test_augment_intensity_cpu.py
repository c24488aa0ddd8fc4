"""CPU checks of the host side of the four intensity transforms beyond the pool (dram_amd/augment.py: IntensityInverse,
GammaTransform, ContrastStretchingTransform, ContrastJitter): the draw sequences and constructor signatures against what the
reference drew and declares (tests/golden/augment_intensity.npz, written by scripts/make_golden_intensity.py), the refused
`channel_dim` values, and the argument errors of the new C entry points (reported without a GPU)."""
import ctypes
import inspect
import os
import random

import numpy as np
import pytest

import dram_amd
from dram_amd import _lib
from dram_amd import augment as A

SHAPES = {"s5x7x9": (5, 7, 9), "s6x8x8": (6, 8, 8), "s24x40x48": (24, 40, 48)}
CASES = {"inverse": (A.IntensityInverse, {}), "gamma": (A.GammaTransform, {}), "stretch": (A.ContrastStretchingTransform, {}),
         "jitter": (A.ContrastJitter, {}), "jitter_volume": (A.ContrastJitter, {"channel_dim": None})}


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "augment_intensity.npz"))


def _seed(s):
    random.seed(int(s))
    np.random.seed(int(s))


@pytest.mark.parametrize("tag", list(SHAPES))
@pytest.mark.parametrize("name", list(CASES))
def test_draws_equal_the_reference(gold, name, tag):
    """Seeded as the fixture was, `draw(3, shape)` gives the reference's parameters bit for bit, and the generator stands where
    the reference left it: the next draw is the recorded one."""
    cls, kw = CASES[name]
    shape = SHAPES[tag]
    _seed(gold["seed"])
    got = cls(**kw).draw(3, shape)
    nxt = np.random.random_sample()
    assert len(got) == 3 and all(isinstance(p, dict) for p in got)
    if name == "inverse":
        assert got == [{}] * 3
    if name in ("gamma", "stretch"):
        assert [p["factor"] for p in got] == list(gold[f"{name}/{tag}/factor"])
    if name == "stretch":
        assert [p["mp"] for p in got] == list(gold[f"{name}/{tag}/mp"])
    if name.startswith("jitter"):
        want = gold[f"{name}/{tag}/factor"]
        assert want.shape == (3, shape[0] if name == "jitter" else 1)       # D draws per sample by default, one with None
        assert [p["factor"] for p in got] == want.tolist()
    assert nxt == float(gold[f"{name}/{tag}/next"])


@pytest.mark.parametrize("name", list(CASES))
def test_constructor_signatures_equal_the_reference(gold, name):
    cls, _ = CASES[name]
    assert str(inspect.signature(cls.__init__)) == str(gold[f"{name}/signature"])


def test_exported_from_the_package():
    for name in ("IntensityInverse", "GammaTransform", "ContrastStretchingTransform", "ContrastJitter", "GaussianBlur",
                 "RandomMaskOut", "RandomFlip", "RandomRotate90", "GaussianAddictive", "EnsembleScanAugmentation"):
        assert getattr(dram_amd, name) is getattr(A, name) and name in dram_amd.__all__
    with pytest.raises(AttributeError):
        dram_amd.HistogramEqual


def test_unsupported_channel_dim_is_refused():
    for cls in (A.IntensityInverse, A.GammaTransform, A.ContrastStretchingTransform):
        for ok in (0, None):
            assert cls(channel_dim=ok).channel_dim == ok
        for bad in (1, 2, -1):
            with pytest.raises(NotImplementedError, match="channel_dim"):
                cls(channel_dim=bad)
    assert A.ContrastJitter().channel_dim == 0 and A.ContrastJitter(channel_dim=None).channel_dim is None
    for bad in (1, 2, -1):
        with pytest.raises(NotImplementedError, match="channel_dim"):
            A.ContrastJitter(channel_dim=bad)


def test_jitter_wants_one_factor_per_row():
    with pytest.raises(ValueError, match="5 factors per sample"):
        A.ContrastJitter()._tables([{"factor": [1.0]}], (5, 7, 9), "cpu")
    with pytest.raises(ValueError, match="1 factors per sample"):
        A.ContrastJitter(channel_dim=None)._tables([{"factor": [1.0] * 5}], (5, 7, 9), "cpu")
    table, rows = A.ContrastJitter()._tables([{"factor": [1.0, 1.1, 1.2, 0.9, 0.8]}, None], (5, 7, 9), "cpu")
    assert rows == 5 and tuple(table.shape) == (10, 2)


def test_pool_hooks():
    """What the ensemble driver reads: the three range maps share its {min, max} pre-pass, the jitter brings its own."""
    for cls in (A.IntensityInverse, A.GammaTransform, A.ContrastStretchingTransform, A.RandomMaskOut, A.GaussianAddictive):
        assert cls.intensity and cls.pointwise and cls.uses_minmax
    assert A.ContrastJitter.intensity and A.ContrastJitter.pointwise and not A.ContrastJitter.uses_minmax
    for cls in (A.GaussianBlur, A.RandomFlip, A.RandomRotate90):
        assert not cls.pointwise and not cls.uses_minmax
    assert len(A.EnsembleScanAugmentation(0.5).transform_pool) == 5      # the default pool stays the reference's five


FAKE = ctypes.c_void_p(16)      # never dereferenced: the argument checks come first


def test_new_entries_check_their_arguments():
    assert _lib.lib.dram_aug_row_mean_ws_bytes(3, 63) == 3 * 8 and _lib.lib.dram_aug_row_mean_ws_bytes(0, 63) == 0
    assert _lib.lib.dram_aug_row_mean_ws_bytes(2, 1 << 24) == 2 * 128 * 8
    with pytest.raises(_lib.DramHipError, match="null pointer"):
        _lib.call("dram_aug_row_mean", FAKE, None, None, 2, 64, FAKE, 64, None)
    with pytest.raises(_lib.DramHipError, match="workspace too small"):
        _lib.call("dram_aug_row_mean", FAKE, FAKE, None, 2, 64, FAKE, 8, None)
    with pytest.raises(_lib.DramHipError, match="bad sizes"):
        _lib.call("dram_aug_row_mean", FAKE, FAKE, None, 70000, 64, FAKE, 1 << 20, None)
    with pytest.raises(_lib.DramHipError, match="unknown mode 4"):
        _lib.call("dram_aug_intensity_map", FAKE, FAKE, 4, FAKE, FAKE, FAKE, 1, FAKE, 2, 2, 64, None)
    for mode, mm, mean, par, keep in [(A.MAP_GAMMA, None, None, FAKE, 0), (A.MAP_GAMMA, FAKE, None, None, 0),
                                      (A.MAP_JITTER, FAKE, None, FAKE, 1), (A.MAP_JITTER, None, FAKE, FAKE, 1)]:
        with pytest.raises(_lib.DramHipError, match="null pointer"):
            _lib.call("dram_aug_intensity_map", FAKE, FAKE, mode, mm, mean, par, keep, FAKE, 2, 2, 64, None)
    with pytest.raises(_lib.DramHipError, match="table length 3 does not match the batch of 2"):
        _lib.call("dram_aug_intensity_map", FAKE, FAKE, A.MAP_INVERSE, FAKE, None, None, 0, FAKE, 3, 2, 64, None)
