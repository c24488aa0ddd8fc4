"""Host side of RandomAffineTransform3D and RandomRotate (dram_amd/augment.py): the numpy restatement of scipy's order-3 and
order-0 resampling (tests/spline_restatement.py) against what the reference's own classes produced
(tests/golden/augment_spline.npz, written by scripts/make_golden_spline.py), the draw sequences, the host-built matrices
(against the ones the reference handed to scipy, which the fixture records), the constructor signatures, the per-sample
tables and the argument errors of the C entry points (reported without a GPU).

Bounds.  Restatement and scipy both add the taps in fp64 and round once to fp32, so an image may differ by that one rounding:
at most one fp32 step (np.spacing) of the fixture's value.  Order-0 entries (uint8 and fp32) are copies: exactly equal."""
import ctypes
import inspect
import os
import random

import numpy as np
import pytest
import torch

import dram_amd
from dram_amd import _lib
from dram_amd import augment as A

import spline_restatement as SR

ENTRIES = (("image", 3), ("lobe", 0), ("lesion", 0))


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "augment_spline.npz"))


def within_one_ulp(got, want):
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)


def check_entry(got, want, order, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if order == 3:
        ok = within_one_ulp(got, want)
        assert ok.all(), f"{what}: {int((~ok).sum())} voxels off by more than one fp32 step"
    else:
        assert np.array_equal(got, want), what


def affine_params(gold, i):
    return {"scales": [float(v) for v in gold["affine/scales"][i]], "rotate_angles": [float(v) for v in gold["affine/angles"][i]]}


def rotate_params(gold, case, i):
    return {"rotate_axis": tuple(int(v) for v in gold[f"{case}/axes"][i]), "rotate_angle": int(gold[f"{case}/angles"][i])}


def test_restatement_equals_the_reference_affine(gold):
    for i, seed in enumerate(gold["affine/seeds"]):
        if seed < 0:
            for name, _ in ENTRIES:
                assert np.array_equal(gold[f"affine/out_{name}"][i], gold[f"affine/x_{name}"][i])
            continue
        m, off = gold["affine/matrix"][i], gold["affine/offset"][i]      # what the reference handed to scipy
        for name, order in ENTRIES:
            x = gold[f"affine/x_{name}"][i]
            check_entry(SR.affine_transform(x, m, off, order, x.min()), gold[f"affine/out_{name}"][i], order, f"affine {i} {name}")


def test_restatement_equals_the_reference_identity(gold):
    for name, order in ENTRIES:
        x = gold[f"affine/x_{name}"][0]
        got = SR.affine_transform(x, np.eye(3), np.zeros(3), order, x.min())
        check_entry(got, gold[f"identity/out_{name}"][0], order, f"identity {name}")
    # the spline round trip gives the image back to a few fp32 steps, and the fixture says so itself
    x, y = gold["affine/x_image"][0], gold["identity/out_image"][0]
    assert np.abs(y - x).max() <= 4 * np.spacing(np.abs(x).max())


@pytest.mark.parametrize("case", ["rotate", "rotate1"])
def test_restatement_equals_the_reference_rotate(gold, case):
    for i in range(len(gold[f"{case}/seeds"])):
        p = rotate_params(gold, case, i)
        for name, order in ENTRIES:
            x = gold[f"{case}/x_{name}"][i]
            check_entry(SR.rotate(x, p["rotate_angle"], p["rotate_axis"], order), gold[f"{case}/out_{name}"][i], order,
                        f"{case} {i} {name}")


def test_affine_draw_reproduces_the_reference(gold):
    shape = gold["affine/x_image"].shape[1:]
    for i, seed in enumerate(gold["affine/seeds"]):
        if seed < 0:
            continue
        np.random.seed(int(seed))
        p = A.RandomAffineTransform3D(3).draw_one(tuple(shape))
        assert p == affine_params(gold, i)
        assert np.random.random_sample() == gold["affine/next_random"][i]
    np.random.seed(3)
    p = A.RandomAffineTransform3D(3, rotations=(0.0, 0.0, 0.0), scales=(0.0, 0.0, 0.0)).draw_one(tuple(shape))
    assert p == {"scales": [1.0] * 3, "rotate_angles": [0.0] * 3}


@pytest.mark.parametrize("case", ["rotate", "rotate1"])
def test_rotate_draw_reproduces_the_reference(gold, case):
    shape = gold[f"{case}/x_image"].shape[1:]
    rng = tuple(int(v) for v in gold["rotate_range"])
    for i, seed in enumerate(gold[f"{case}/seeds"]):
        random.seed(int(seed))
        assert A.RandomRotate(3, rng).draw_one(tuple(shape)) == rotate_params(gold, case, i)
        assert random.random() == gold[f"{case}/next_random"][i]


def test_host_matrices(gold):
    shape = tuple(gold["affine/x_image"].shape[1:])
    for i, seed in enumerate(gold["affine/seeds"]):
        if seed < 0:
            continue
        p = affine_params(gold, i)
        m, off = A.affine_matrix(p["scales"], p["rotate_angles"], shape)
        assert np.array_equal(m, gold["affine/matrix"][i]) and np.array_equal(off, gold["affine/offset"][i])
    m, off = A.affine_matrix([1.0] * 3, [0.0] * 3, shape)
    assert np.array_equal(m, np.eye(3)) and not off.any()
    assert np.array_equal(m, gold["identity/matrix"]) and np.array_equal(off, gold["identity/offset"])
    for case in ("rotate", "rotate1"):
        shape = tuple(gold[f"{case}/x_image"].shape[1:])
        for i in range(len(gold[f"{case}/seeds"])):
            p = rotate_params(gold, case, i)
            m, off, fixed = A.rotate_matrix(p["rotate_angle"], p["rotate_axis"], shape)
            ax, rot, shift = SR.rotate_plane_matrix(p["rotate_angle"], p["rotate_axis"], shape)
            m2, off2 = SR.embed_plane(ax, rot, shift)
            assert np.array_equal(m, m2) and np.array_equal(off, off2) and fixed not in ax and sorted(ax + [fixed]) == [0, 1, 2]
            assert np.array_equal(m[fixed], np.eye(3)[fixed]) and off[fixed] == 0.0
    m, off, fixed = A.rotate_matrix(90, (-2, -3), (12, 20, 67))      # a quarter turn is exact
    assert np.array_equal(m, [[0, 1, 0], [-1, 0, 0], [0, 0, 1]]) and np.array_equal(off, [-4.0, 15.0, 0.0]) and fixed == 2
    with pytest.raises(ValueError, match="no plane"):
        A.rotate_matrix(10, (-1, -1), (4, 4, 4))


def test_tables(gold):
    shape = (12, 20, 67)
    params = [rotate_params(gold, "rotate", 0), None, rotate_params(gold, "rotate", 2)]
    tab, axes = A.RandomRotate(3, (0, 0))._tables(params, shape, "cpu")
    rec = tab.numpy().view(A.SPLINE_DTYPE)
    assert rec.shape == (3,) and axes.tolist() == [6, 0, 3] and rec["fixed"].tolist() == [0, -1, 2]
    assert np.array_equal(rec["m"][1], np.eye(3).reshape(9)) and not rec["off"][1].any()
    m, off, _ = A.rotate_matrix(90, (-2, -3), shape)
    assert np.array_equal(rec["m"][2], m.reshape(9)) and np.array_equal(rec["off"][2], off)
    tab, axes = A.RandomAffineTransform3D(3)._tables([affine_params(gold, 0)], (13, 18, 70), "cpu")
    assert axes.tolist() == [7] and tab.numpy().view(A.SPLINE_DTYPE)["fixed"].tolist() == [-1]
    with pytest.raises(ValueError, match="not finite"):
        A.RandomAffineTransform3D(3)._tables([{"scales": [1.0, np.nan, 1.0], "rotate_angles": [0.0] * 3}], shape, "cpu")


def test_classes_and_signatures(gold):
    for name in ("RandomAffineTransform3D", "RandomRotate"):
        cls = getattr(A, name)
        assert getattr(dram_amd, name) is cls and name in dram_amd.__all__
        assert str(inspect.signature(cls.__init__)) == str(gold[f"sig/{name}"])
        assert issubclass(cls, A._Augmentation) and cls.intensity is False
    pool = A.EnsembleScanAugmentation(0.5).transform_pool
    assert not any(isinstance(t, A._SplineTransform) for t in pool)
    for bad in (lambda: A.RandomAffineTransform3D(2), lambda: A.RandomRotate(2, (0, 10))):
        with pytest.raises(NotImplementedError):
            bad()


def test_host_tensors_are_refused():
    t = A.RandomRotate(3, (0, 10))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        t.apply({"#image": torch.zeros(1, 4, 4, 4)}, [{"rotate_axis": (-1, -2), "rotate_angle": 3}])


FAKE = ctypes.c_void_p(16)      # never dereferenced: the argument checks come first


def test_new_entries_check_their_arguments():
    other = ctypes.c_void_p(4096)
    assert _lib.lib.dram_aug_spline_ws_bytes(2, 4, 5, 6) == 2 * 4 * 5 * 6 * 8
    assert _lib.lib.dram_aug_spline_ws_bytes(0, 4, 5, 6) == 0 and _lib.lib.dram_aug_spline_ws_bytes(1, 1024, 1024, 1024) == 0
    with pytest.raises(_lib.DramHipError, match="null pointer"):
        _lib.call("dram_aug_minmax_u8", None, FAKE, None, 2, 64, None)
    with pytest.raises(_lib.DramHipError, match="null pointer"):
        _lib.call("dram_aug_spline_prefilter", FAKE, None, FAKE, 2, 2, 4, 4, 4, FAKE, 1024, None)
    with pytest.raises(_lib.DramHipError, match="table length 3 does not match the batch of 2"):
        _lib.call("dram_aug_spline_prefilter", FAKE, FAKE, FAKE, 3, 2, 4, 4, 4, FAKE, 1024, None)
    with pytest.raises(_lib.DramHipError, match="workspace too small"):
        _lib.call("dram_aug_spline_prefilter", FAKE, FAKE, FAKE, 2, 2, 4, 4, 4, FAKE, 1023, None)
    with pytest.raises(_lib.DramHipError, match="bad sizes"):
        _lib.call("dram_aug_spline_prefilter", FAKE, FAKE, FAKE, 2, 2, 1024, 1024, 1024, FAKE, 1024, None)
    with pytest.raises(_lib.DramHipError, match="null pointer"):
        _lib.call("dram_aug_spline_resample", FAKE, other, 4, 3, None, FAKE, FAKE, 1024, FAKE, 2, 2, 4, 4, 4, None)
    with pytest.raises(_lib.DramHipError, match="element size 2"):
        _lib.call("dram_aug_spline_resample", FAKE, other, 2, 0, FAKE, FAKE, None, 0, FAKE, 2, 2, 4, 4, 4, None)
    with pytest.raises(_lib.DramHipError, match="order 1"):
        _lib.call("dram_aug_spline_resample", FAKE, other, 4, 1, FAKE, FAKE, None, 0, FAKE, 2, 2, 4, 4, 4, None)
    with pytest.raises(_lib.DramHipError, match="float32 only"):
        _lib.call("dram_aug_spline_resample", FAKE, other, 1, 3, FAKE, FAKE, FAKE, 1024, FAKE, 2, 2, 4, 4, 4, None)
    with pytest.raises(_lib.DramHipError, match="cannot run in place"):
        _lib.call("dram_aug_spline_resample", FAKE, FAKE, 4, 0, FAKE, FAKE, None, 0, FAKE, 2, 2, 4, 4, 4, None)
    with pytest.raises(_lib.DramHipError, match="needs the coefficients"):
        _lib.call("dram_aug_spline_resample", FAKE, other, 4, 3, FAKE, FAKE, None, 0, FAKE, 2, 2, 4, 4, 4, None)
    with pytest.raises(_lib.DramHipError, match="workspace too small"):
        _lib.call("dram_aug_spline_resample", FAKE, other, 4, 3, FAKE, FAKE, FAKE, 8, FAKE, 2, 2, 4, 4, 4, None)
    with pytest.raises(_lib.DramHipError, match="table length 3"):
        _lib.call("dram_aug_spline_resample", FAKE, other, 4, 0, FAKE, FAKE, None, 0, FAKE, 3, 2, 4, 4, 4, None)
