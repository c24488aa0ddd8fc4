"""CPU checks of the host side of RandomCrop and StandarizeChannel (dram_amd/augment.py): the draw sequences and constructor
signatures against what the reference drew and declares (tests/golden/augment_crop.npz, written by
scripts/make_golden_crop.py), the numpy restatement of its pad and slice (`pad_crop` over `crop_window`) against the crops the
reference itself handed to the resampler, the record table, the refusals, and the argument errors of the C entry points
(reported without a GPU)."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import dram_amd
from dram_amd import _lib
from dram_amd import augment as A

KEYS = ("crop_sizes_ratio", "crop_sizes", "offset", "shifted_center", "padding")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "augment_crop.npz"))


def _cases(gold):
    return range(int(gold["n_cases"]))


def _make(gold, i):
    return A.RandomCrop(tuple(gold[f"case{i}/shift_from_center"].tolist()), tuple(gold[f"case{i}/ratio"].tolist()))


def _params(gold, i):
    p = {k: gold[f"case{i}/{k}"].tolist() for k in KEYS}
    p["padding"] = [tuple(q) for q in p["padding"]]
    p["spacing"] = tuple(gold["spacing"].tolist())
    return p


def test_draws_equal_the_reference(gold):
    """Seeded as the fixture was, draw_one gives what the reference stored in the output's meta, as plain ints and floats, and
    numpy's generator stands where the reference left it."""
    for i in _cases(gold):
        shape = tuple(gold[f"case{i}/shape"].tolist())
        np.random.seed(int(gold[f"case{i}/seed"]))
        got = _make(gold, i).draw_one(shape)
        nxt = np.random.random_sample()
        assert set(got) == set(KEYS)
        for k in KEYS:
            assert np.array_equal(np.asarray(got[k]), gold[f"case{i}/{k}"]), (i, k)
        assert nxt == float(gold[f"case{i}/next_random"]), i
        flat = [v for k in KEYS for q in got[k] for v in (q if isinstance(q, tuple) else (q,))]
        assert all(type(v) in (int, float) for v in flat), flat
        assert str(gold[f"case{i}/padding_mode"]) == "minimum"
    assert A.StandarizeChannel(0).draw_one((4, 4, 4)) == {}


def test_constructor_signatures_equal_the_reference(gold):
    assert str(inspect.signature(A.RandomCrop.__init__)) == str(gold["sig/RandomCrop"])
    assert str(inspect.signature(A.StandarizeChannel.__init__)) == str(gold["sig/StandarizeChannel"])


def test_exported_from_the_package():
    for name in ("RandomCrop", "StandarizeChannel"):
        assert getattr(dram_amd, name) is getattr(A, name) and name in dram_amd.__all__
    with pytest.raises(AttributeError):
        dram_amd.HistogramEqual
    assert not A.RandomCrop.intensity and not A.RandomCrop.pointwise and not A.RandomCrop.uses_minmax
    assert A.StandarizeChannel.intensity and A.StandarizeChannel.pointwise and not A.StandarizeChannel.uses_minmax


def test_pad_crop_equals_the_reference_s_crops(gold):
    """Bit for bit, fp32 and uint8, the truncated and the two- and three-axis padded cases included; the window's size is the
    recorded crop's shape."""
    seen = {"truncated": 0, "two": 0, "three": 0}
    for i in _cases(gold):
        p = _params(gold, i)
        shape = tuple(gold[f"case{i}/shape"].tolist())
        start, size = A.crop_window(p, shape)
        want = gold[f"case{i}/crop_image"]
        assert size == want.shape, i
        got = A.pad_crop(gold[f"case{i}/x"], p, "minimum")
        assert got.dtype == np.float32 and np.array_equal(got, want), i
        got = A.pad_crop(gold[f"case{i}/lobe"], p, "minimum")
        assert got.dtype == np.uint8 and np.array_equal(got, gold[f"case{i}/crop_lobe"]), i
        out = sum(1 for st, sz, d in zip(start, size, shape) if st < 0 or st + sz > d)
        seen["truncated"] += size != tuple(p["crop_sizes"])
        seen["two"] += out == 2
        seen["three"] += out == 3
    assert all(seen.values()), seen


def test_pad_crop_equals_numpy_pad(gold):
    """'constant' and 'edge': np.pad of the whole chunk by the window's overhang, sliced at the window."""
    for i in _cases(gold):
        p = _params(gold, i)
        x = gold[f"case{i}/x"]
        start, size = A.crop_window(p, x.shape)
        over = [(max(0, -st), max(0, st + sz - d)) for st, sz, d in zip(start, size, x.shape)]
        for mode in ("constant", "edge"):
            want = np.pad(x, over, mode=mode)[tuple(slice(st + o[0], st + o[0] + sz) for st, sz, o in zip(start, size, over))]
            assert np.array_equal(A.pad_crop(x, p, mode), want), (i, mode)


def test_minimum_pad_is_the_projection_over_the_outside_axes(gold):
    """What the device kernel rests on: a padded position holds the minimum of the chunk over exactly the axes in which it lies
    outside, the inside coordinates held fixed."""
    for i in _cases(gold):
        p = _params(gold, i)
        for src in (gold[f"case{i}/x"], gold[f"case{i}/lobe"]):
            start, size = A.crop_window(p, src.shape)
            crop = A.pad_crop(src, p, "minimum")
            for idx in np.ndindex(*size):
                c = [st + k for st, k in zip(start, idx)]
                sel = tuple(slice(None) if not 0 <= v < d else v for v, d in zip(c, src.shape))
                assert crop[idx] == np.min(src[sel]), (i, idx)


def test_crop_table(gold):
    """Window start, actual size, mode and the steps of resample_plan('fixed_size') on the actual crop shape."""
    i = 5                                                     # seed 24: low z, high x, truncated
    p = _params(gold, i)
    shape = tuple(gold[f"case{i}/shape"].tolist())
    tab, pads = _make(gold, i)._tables([p, None], shape, "cpu")
    rec = np.frombuffer(tab.numpy().tobytes(), dtype=A.CROP_DTYPE)
    start, size = A.crop_window(p, shape)
    assert (rec["z0"][0], rec["y0"][0], rec["x0"][0]) == start and (rec["cd"][0], rec["ch"][0], rec["cw"][0]) == size
    assert rec["mode"][0] == A.PAD_MODES["minimum"] == 2 and pads == [True, False]
    sp = gold["spacing"]
    for a, name in enumerate(("sz", "sy", "sx")):
        assert rec[name][0] == (sp[a] * (size[a] / shape[a])) / sp[a]
    assert np.allclose(gold[f"case{i}/meta_spacing"], [rec[n][0] * s for n, s in zip(("sz", "sy", "sx"), sp)], rtol=1e-15)
    assert (rec["cd"][1], rec["ch"][1], rec["cw"][1]) == shape and rec["sx"][1] == 1.0
    _, pads = A.RandomCrop((0.5,) * 3, (0.4,) * 3, padding_mode="edge")._tables([p], shape, "cpu")
    assert pads == [False]                                    # only 'minimum' needs the pre-pass


def test_refusals():
    with pytest.raises(NotImplementedError):
        A.RandomCrop((0.5,) * 2, (0.4,) * 2, spatial_dim=2)
    with pytest.raises(AssertionError):
        A.RandomCrop((0.5,) * 2, (0.4,) * 3)
    for mode in ("reflect", "mean", "wrap"):
        with pytest.raises(NotImplementedError, match="padding_mode"):
            A.RandomCrop((0.5,) * 3, (0.4,) * 3, padding_mode=mode)
    for mode in ("minimum", "constant", "edge"):
        A.RandomCrop((0.5,) * 3, (0.4,) * 3, padding_mode=mode)
    with pytest.raises(ValueError, match="changes the sample's shape and cannot live in a batch tensor"):
        A.RandomCrop((0.5,) * 3, (0.4,) * 3, keep_size=False)
    t = A.RandomCrop((0.5,) * 3, (0.4,) * 3)
    p = {"crop_sizes": (4, 4, 4), "shifted_center": (4, 4, 4), "padding": [(0, 0)] * 3}
    tables = t._tables([p], (8, 8, 8), "cpu")
    flags = torch.ones(1, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="linear"):      # a uint8 key that is no reference / weight map
        t._launch_key("#image", torch.zeros((1, 1, 8, 8, 8), dtype=torch.uint8), tables, flags)
    with pytest.raises(NotImplementedError, match="single-channel"):
        t._launch_key("#image", torch.zeros((1, 2, 8, 8, 8)), tables, flags)
    with pytest.raises(ValueError, match="empty crop"):
        t._tables([dict(p, crop_sizes=(0, 4, 4))], (8, 8, 8), "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        t.apply({"#image": torch.zeros((1, 8, 8, 8))}, [p])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.StandarizeChannel(0).apply({"#image": torch.zeros((1, 8, 8, 8))}, [{}])


FAKE = ctypes.c_void_p(16)      # never dereferenced: the argument checks come first


def test_new_entries_check_their_arguments():
    per = 12 * 20 + 9 * 20 + 9 * 12 + 20 + 12 + 9 + 1
    assert _lib.lib.dram_aug_pad_min_ws_bytes(3, 9, 12, 20, 4) == 3 * ((per + 3) // 4 * 4) * 4
    assert _lib.lib.dram_aug_pad_min_ws_bytes(3, 9, 12, 20, 1) == 3 * ((per + 3) // 4 * 4)
    assert _lib.lib.dram_aug_pad_min_ws_bytes(3, 9, 12, 20, 2) == 0 and _lib.lib.dram_aug_pad_min_ws_bytes(0, 9, 12, 20, 4) == 0
    with pytest.raises(_lib.DramHipError, match="null pointer"):
        _lib.call("dram_aug_pad_min", FAKE, 4, None, 2, 4, 4, 4, FAKE, 1 << 20, None)
    with pytest.raises(_lib.DramHipError, match="element size 2"):
        _lib.call("dram_aug_pad_min", FAKE, 2, FAKE, 2, 4, 4, 4, FAKE, 1 << 20, None)
    with pytest.raises(_lib.DramHipError, match="bad sizes"):
        _lib.call("dram_aug_pad_min", FAKE, 4, FAKE, 2, 4, 4, 4096, FAKE, 1 << 30, None)
    with pytest.raises(_lib.DramHipError, match="workspace too small"):
        _lib.call("dram_aug_pad_min", FAKE, 4, FAKE, 2, 4, 4, 4, FAKE, 8, None)
    other = ctypes.c_void_p(32)
    with pytest.raises(_lib.DramHipError, match="null pointer"):
        _lib.call("dram_aug_crop_resample", FAKE, other, 4, 1, None, None, 0, FAKE, 2, 2, 4, 4, 4, None)
    with pytest.raises(_lib.DramHipError, match="float32 only"):
        _lib.call("dram_aug_crop_resample", FAKE, other, 1, 1, FAKE, None, 0, FAKE, 2, 2, 4, 4, 4, None)
    with pytest.raises(_lib.DramHipError, match="table length 3 does not match the batch of 2"):
        _lib.call("dram_aug_crop_resample", FAKE, other, 4, 1, FAKE, None, 0, FAKE, 3, 2, 4, 4, 4, None)
    with pytest.raises(_lib.DramHipError, match="cannot run in place"):
        _lib.call("dram_aug_crop_resample", FAKE, FAKE, 4, 1, FAKE, None, 0, FAKE, 2, 2, 4, 4, 4, None)
    with pytest.raises(_lib.DramHipError, match="bad sizes"):
        _lib.call("dram_aug_crop_resample", FAKE, other, 4, 1, FAKE, None, 0, FAKE, 2, 2, 4, 4, 4096, None)
    with pytest.raises(_lib.DramHipError, match="workspace too small"):
        _lib.call("dram_aug_crop_resample", FAKE, other, 4, 1, FAKE, FAKE, 8, FAKE, 2, 2, 4, 4, 4, None)
    assert _lib.lib.dram_aug_row_mean_std_ws_bytes(3, 63) == 3 * 3 * 8
    with pytest.raises(_lib.DramHipError, match="null pointer"):
        _lib.call("dram_aug_row_mean_std", FAKE, None, None, 2, 64, FAKE, 64, None)
    with pytest.raises(_lib.DramHipError, match="workspace too small"):
        _lib.call("dram_aug_row_mean_std", FAKE, FAKE, None, 2, 64, FAKE, 8, None)
    assert A.MAP_STANDARDIZE == 5
    with pytest.raises(_lib.DramHipError, match="null pointer"):       # standardize needs its {mean, std} table only
        _lib.call("dram_aug_intensity_map", FAKE, FAKE, A.MAP_STANDARDIZE, None, None, None, 0, FAKE, 2, 2, 64, None)
    with pytest.raises(_lib.DramHipError, match="unknown mode 6"):
        _lib.call("dram_aug_intensity_map", FAKE, FAKE, 6, FAKE, FAKE, FAKE, 0, FAKE, 2, 2, 64, None)
