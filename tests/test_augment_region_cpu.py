"""CPU checks of the host side of the slab projections, region masks and axis moves (dram_amd/augment.py:
MinimalIntensityProjection, MaximumIntensityProjection, MinimalIntensityAxialProjection, DiskMaskOut, RandomCubeMask,
RandomMoveAxis, RandomRotateInplane90): the draw sequences and constructor signatures against what the reference drew and
declares (tests/golden/augment_region.npz, written by scripts/make_golden_region.py), the refusals, the box / disk / (perm, flip)
tables, and the argument errors of the two C entry points (reported without a GPU)."""
import ctypes
import inspect
import os
import random

import numpy as np
import pytest

import dram_amd
from dram_amd import _lib
from dram_amd import augment as A

SHAPES = {"s5x7x9": (5, 7, 9), "s6x8x8": (6, 8, 8), "s18x18x277": (18, 18, 277), "s6x6x6": (6, 6, 6), "s7x7x7": (7, 7, 7)}
THREE = ["s5x7x9", "s6x8x8", "s18x18x277"]
CASES = {"minip": (lambda: A.MinimalIntensityProjection(), THREE, ("slab_thickness", "angle")),
         "maxip": (lambda: A.MaximumIntensityProjection(), THREE, ("slab_thickness", "angle")),
         "minip_axial": (lambda: A.MinimalIntensityAxialProjection(), THREE, ("slab_thickness",)),
         "disk": (lambda: A.DiskMaskOut(), THREE, ()),
         "cube": (lambda: A.RandomCubeMask((0.2,) * 3, (0.5,) * 3), THREE, ("shifted_center", "crop_sizes")),
         "moveaxis": (lambda: A.RandomMoveAxis(3), ["s6x6x6", "s7x7x7"], ("sampled_comb",)),
         "rot_inplane": (lambda: A.RandomRotateInplane90(3), ["s6x8x8"], ("rotate_times",))}
NAMES = ("MinimalIntensityProjection", "MaximumIntensityProjection", "MinimalIntensityAxialProjection", "DiskMaskOut",
         "RandomCubeMask", "RandomMoveAxis", "RandomRotateInplane90")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "augment_region.npz"))


def _plain(v):
    return v.tolist() if isinstance(v, np.ndarray) else (list(v) if isinstance(v, tuple) else v)


@pytest.mark.parametrize("name,tag", [(n, t) for n, c in CASES.items() for t in c[1]])
def test_draws_equal_the_reference(gold, name, tag):
    """Seeded as the fixture was, `draw(3, shape)` gives the reference's parameters for the three samples in order, and both
    generators stand where the reference left them."""
    make, _, keys = CASES[name]
    random.seed(int(gold["seed"]))
    np.random.seed(int(gold["seed"]))
    got = make().draw(3, SHAPES[tag])
    nxt, nxt_random = np.random.random_sample(), random.random()
    assert len(got) == 3 and all(isinstance(p, dict) and set(p) == set(keys) for p in got)
    for key in keys:
        want = gold[f"{name}/{tag}/{key}"]
        assert [_plain(p[key]) for p in got] == want.tolist(), key
    assert nxt == float(gold[f"{name}/{tag}/next"]) and nxt_random == float(gold[f"{name}/{tag}/next_random"])


def test_the_reference_cube_mask_raised(gold):
    """What the deviation note of RandomCubeMask rests on: the reference's __call__ raised on every sample of the fixture."""
    assert int(gold["cube/raised"]) == 9


@pytest.mark.parametrize("name", list(CASES))
def test_constructor_signatures_equal_the_reference(gold, name):
    assert str(inspect.signature(type(CASES[name][0]()).__init__)) == str(gold[f"{name}/signature"])


def test_exported_from_the_package():
    for name in NAMES:
        assert getattr(dram_amd, name) is getattr(A, name) and name in dram_amd.__all__
    assert A.MAX_SLAB >= 16


def test_pool_hooks():
    """What the ensemble driver reads: the projections are neighbourhood operations on image entries, the masks run in place on
    every '#' entry, the axis moves are permutations; none takes the driver's {min, max}."""
    for cls in (A.MinimalIntensityProjection, A.MaximumIntensityProjection, A.MinimalIntensityAxialProjection):
        assert cls.intensity and not cls.pointwise and not cls.uses_minmax
    for cls in (A.DiskMaskOut, A.RandomCubeMask):
        assert not cls.intensity and cls.pointwise and not cls.uses_minmax
    for cls in (A.RandomMoveAxis, A.RandomRotateInplane90):
        assert not cls.intensity and not cls.pointwise and not cls.uses_minmax
    assert A.MaximumIntensityProjection.is_max and not A.MinimalIntensityProjection.is_max
    assert not A.MinimalIntensityAxialProjection.is_max


def test_refusals():
    for kw in ({"spatial_dim": 2}, {"select_axis": -1}, {"select_axis": -2}, {"select_axis": 0}):
        with pytest.raises(NotImplementedError):
            A.DiskMaskOut(**kw)
    with pytest.raises(NotImplementedError):
        A.RandomCubeMask((0.2,) * 2, (0.5,) * 2, spatial_dim=2)
    for cls in (A.MinimalIntensityProjection, A.MaximumIntensityProjection, A.MinimalIntensityAxialProjection):
        with pytest.raises(ValueError, match="slab_thickness 17"):
            cls()._tables([{"slab_thickness": A.MAX_SLAB + 1, "angle": 0}], (5, 7, 9), "cpu")
        with pytest.raises(ValueError, match="slab_thickness -1"):
            cls()._tables([{"slab_thickness": -1, "angle": 0}], (5, 7, 9), "cpu")
    with pytest.raises(ValueError, match="angle 3"):
        A.MinimalIntensityProjection()._tables([{"slab_thickness": 3, "angle": 3}], (5, 7, 9), "cpu")
    # a move or a turn that would change the sample's shape
    with pytest.raises(ValueError, match="shape"):
        A.RandomMoveAxis(3)._tables([{"sampled_comb": (-1, -2)}], (6, 8, 9), "cpu")
    with pytest.raises(ValueError, match="shape"):
        A.RandomMoveAxis(3)._tables([{"sampled_comb": (-1, -3)}], (6, 8, 8), "cpu")
    with pytest.raises(ValueError, match="shape"):
        A.RandomRotateInplane90(3)._tables([{"rotate_times": 1}], (8, 8, 6), "cpu")
    A.RandomRotateInplane90(3)._tables([{"rotate_times": 2}], (8, 8, 6), "cpu")       # a half turn keeps any shape
    A.RandomMoveAxis(3)._tables([{"sampled_comb": (-1, -2)}], (6, 8, 8), "cpu")


def test_projection_tables():
    th, ax = A.MaximumIntensityProjection()._tables([{"slab_thickness": 9, "angle": 2}, None, {"slab_thickness": 0, "angle": -1},
                                                     {"slab_thickness": 16, "angle": 1}], (5, 7, 9), "cpu")
    assert th.tolist() == [9, 0, 0, 16] and ax.tolist() == [2, 0, 2, 1] and th.dtype == ax.dtype
    th, ax = A.MinimalIntensityAxialProjection()._tables([{"slab_thickness": 4}], (5, 7, 9), "cpu")
    assert th.tolist() == [4] and ax.tolist() == [0]         # always along z


def test_box_and_disk_tables():
    """Hand-computed: [max(0, c - s // 2), min(c + (s - s // 2), dim)) per axis."""
    # odd size 5 about 4: 4 - 2 .. 4 + 3; even size 4 about 3: 1 .. 5; size 1 about 0: 0 .. 1
    assert A.cube_box((4, 3, 0), (5, 4, 1), (10, 10, 10)) == [2, 7, 1, 5, 0, 1]
    # clipped on both sides: size 9 about 2 in an axis of 5: max(0, -2) .. min(7, 5); about 1 in 4: max(0, -3) .. min(6, 4)
    assert A.cube_box((2, 1, 3), (9, 9, 2), (5, 4, 8)) == [0, 5, 0, 4, 2, 4]
    # empty: size 0 (z1 == z0), and a centre so far out that the box ends before it starts
    z0, z1, y0, y1, x0, x1 = A.cube_box((3, 9, 2), (0, 2, 3), (6, 6, 6))
    assert (z0, z1) == (3, 3) and (y0, y1) == (8, 6) and (x0, x1) == (1, 4)
    boxes, disk = A.RandomCubeMask((0.2,) * 3, (0.5,) * 3)._tables(
        [{"shifted_center": (2, 3, 4), "crop_sizes": (2, 6, 7)}, None], (5, 7, 9), "cpu")
    assert boxes.tolist() == [[1, 3, 0, 6, 1, 8], [0] * 6] and disk.tolist() == [[0, 0, -1]] * 2
    # the disk: centre (H // 2, W // 2), radius min(H, W) // 2, squared
    assert A.disk_table((5, 7, 9)) == [3, 4, 9] and A.disk_table((6, 8, 8)) == [4, 4, 16] and A.disk_table((3, 2, 9)) == [1, 4, 1]
    boxes, disk = A.DiskMaskOut()._tables([{}, None], (5, 7, 9), "cpu")
    assert boxes.tolist() == [[0, 5, 0, 7, 0, 9]] * 2 and disk.tolist() == [[3, 4, 9]] * 2


def _apply_table(vol, perm, flip):
    """dram_aug_permute_flip in numpy: out[o] = in[i], i[perm[k]] = flip[k] ? n_k - 1 - o[k] : o[k]."""
    out = np.transpose(vol, perm)
    return np.flip(out, [k for k in range(3) if flip[k]]) if any(flip) else out


def test_move_and_turn_tables_equal_numpy():
    vol = np.arange(7 * 7 * 7).reshape(7, 7, 7)
    for comb in [(-1, -2), (-1, -3), (-2, -3), (-2, -1), (-3, -1), (-3, -2)]:
        perm, flip = A.moveaxis_table(comb, vol.shape)
        assert np.array_equal(_apply_table(vol, perm, flip), np.moveaxis(vol, comb[0], comb[1])), comb
        assert A.RandomMoveAxis(3)._table_one({"sampled_comb": comb}, vol.shape) == (perm, flip)
    assert A.moveaxis_table((-1, -3), vol.shape)[0] == (2, 0, 1)          # a 3-cycle
    slab = np.arange(5 * 6 * 6).reshape(5, 6, 6)
    for times in range(4):
        perm, flip = A.RandomRotateInplane90(3)._table_one({"rotate_times": times}, slab.shape)
        assert np.array_equal(_apply_table(slab, perm, flip), np.rot90(slab, axes=(-1, -2), k=times)), times
    tables = A.RandomMoveAxis(3)._tables([{"sampled_comb": (-1, -3)}, None], (6, 6, 6), "cpu")
    assert tables[0].tolist() == [[2, 0, 1], [0, 1, 2]] and tables[1].tolist() == [[0, 0, 0]] * 2


FAKE = ctypes.c_void_p(16)      # never dereferenced: the argument checks come first


def test_new_entries_check_their_arguments():
    assert _lib.lib.dram_abi_version() == 2
    with pytest.raises(_lib.DramHipError, match="null pointer"):
        _lib.call("dram_aug_slab_project", FAKE, FAKE, None, FAKE, 0, FAKE, 2, 2, 4, 4, 4, None)
    with pytest.raises(_lib.DramHipError, match="table length 3 does not match the batch of 2"):
        _lib.call("dram_aug_slab_project", FAKE, FAKE, FAKE, FAKE, 1, FAKE, 3, 2, 4, 4, 4, None)
    with pytest.raises(_lib.DramHipError, match="cannot run in place"):
        _lib.call("dram_aug_slab_project", FAKE, FAKE, FAKE, FAKE, 1, FAKE, 2, 2, 4, 4, 4, None)
    with pytest.raises(_lib.DramHipError, match="bad sizes"):
        _lib.call("dram_aug_slab_project", FAKE, ctypes.c_void_p(32), FAKE, FAKE, 1, FAKE, 2, 2, 4, 0, 4, None)
    with pytest.raises(_lib.DramHipError, match="null pointer"):
        _lib.call("dram_aug_keep_region", FAKE, FAKE, 4, FAKE, None, FAKE, 2, 2, 1, 4, 4, 4, None)
    with pytest.raises(_lib.DramHipError, match="element size 2"):
        _lib.call("dram_aug_keep_region", FAKE, FAKE, 2, FAKE, FAKE, FAKE, 2, 2, 1, 4, 4, 4, None)
    with pytest.raises(_lib.DramHipError, match="table length 1 does not match the batch of 2"):
        _lib.call("dram_aug_keep_region", FAKE, FAKE, 1, FAKE, FAKE, FAKE, 1, 2, 1, 4, 4, 4, None)
