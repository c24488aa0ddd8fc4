"""Writes tests/golden/augment_spline.npz: the reference's RandomAffineTransform3D and RandomRotate
(dram/data_transforms.py:995-1102), run on the CPU under fixed seeds, with the values they drew.

Needs the reference checkout (see oracle/make_golden.py for where it is expected) and scipy; nothing of the reference is
copied: the fixture holds inputs, drawn parameters, outputs, the next draw of the generator after each sample, the constructor
signatures as strings and the numpy / scipy versions.  RandomAffineTransform3D leaves its draws in the output's meta;
RandomRotate does not, so `ndimage.rotate` is wrapped for this process to note the angle and the axes it is called with.  The
module's `affine_transform` is wrapped in the same way to note the matrix and the offset the reference hands to scipy: the
fixture holds them, and the tests compare the package's host-built matrices with them.

Cases (tests/test_gpu_augment_spline.py says what each is for):
  affine     3 samples of 13 x 18 x 70, the middle one left alone; '#image' fp32, '#lobe_reference' uint8, '#lesion_reference' fp32
  identity   the first of those samples with scales 1 and angles 0
  rotate     4 samples of 12 x 20 x 67 from RandomRotate(3, (-20, 90)): 17 degrees in (-1, -2), -20 in (-1, -3), 90 in (-2, -3)
             (both centres are half-integers there, so every source coordinate is an integer) and 0 degrees; the seeds are the
             first ones whose draws are these
  rotate1    3 samples of 1 x 9 x 11, 17 degrees in each of the three planes

Knife edges.  A voxel whose fp64 source coordinate (tests/spline_restatement.py) lies within 1e-9 of a bound 0 or n - 1 -- for
the order-0 entries also within 1e-9 of a .5 tie -- WITHOUT being that number exactly may fall on either side when one bit of
the matrix changes; the GPU test leaves those out, and main() asserts that they are at most 0.1 % of every case.  A coordinate
that IS the bound or the tie (the identity and the 90 degree sample consist of them) is kept: the same IEEE operations in the
same order give the same number.

    python scripts/make_golden_spline.py
"""
import inspect
import itertools
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import make_golden as MG  # noqa: E402
import spline_restatement as SR  # noqa: E402

AFFINE_SHAPE, ROTATE_SHAPE, FLAT_SHAPE = (13, 18, 70), (12, 20, 67), (1, 9, 11)
AFFINE_SEEDS = (5, None, 11)
ROTATE_RANGE = (-20, 90)
ROTATE_WANTED = ((17, (-1, -2)), (-20, (-1, -3)), (90, (-2, -3)), (0, None))
FLAT_WANTED = ((17, (-1, -2)), (17, (-1, -3)), (17, (-2, -3)))
KNIFE = 1e-9
NOTED = []        # (angle, axes) of every ndimage.rotate call
HANDED = []       # (matrix, offset) of every affine_transform call


def make_input(shape, seed):
    """A ramp plus noise on the odd multiples of 1/16 (compresses well), a label volume and a float map of a few values.  No
    image voxel is 0: where the exact result of the identity transform is 0, scipy's own output is the rounding noise of its
    fp64 sums (1e-15), which no bound relative to the value (the tests' one fp32 step) can hold."""
    rng = np.random.default_rng(2000 + seed)
    z, y, x = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    img = (z * 3 - y * 2 + x + rng.integers(-40, 40, size=shape)) / 8.0 + 0.0625
    lobe = (rng.integers(1, 6, size=shape) + (x > shape[2] // 2)).astype(np.uint8)
    lesion = rng.choice(np.asarray([-1.25, 0.0, 0.5, 1.0], dtype=np.float32), size=shape)
    return img.astype(np.float32), lobe, lesion.astype(np.float32)


def rotate_seed(angle, axes):
    """The first seed from which RandomRotate(3, ROTATE_RANGE) draws this angle and (when given) this plane."""
    combs = list(itertools.combinations([-1, -2, -3], 2))
    for seed in range(100000):
        random.seed(seed)
        a = random.randint(*ROTATE_RANGE)
        ax = tuple(random.sample(list(combs), 2)[0])
        if a == angle and (axes is None or ax == tuple(axes)):
            return seed
    raise AssertionError(f"no seed draws {angle}, {axes}")


def knife_edges(matrix, offset, shape, ties):
    """Voxels whose source coordinate is within KNIFE of a bound (and, with `ties`, of a .5 tie) but is not that number."""
    coords = SR.source_coordinates(matrix, offset, shape)
    edge = np.zeros(shape, dtype=bool)
    for h, n in enumerate(shape):
        for bound in (0.0, float(n - 1)):
            edge |= (np.abs(coords[h] - bound) < KNIFE) & (coords[h] != bound)
        if ties:
            frac = coords[h] - np.floor(coords[h])
            edge |= (np.abs(frac - 0.5) < KNIFE) & (frac != 0.5)
    return edge


def sample_dict(img, lobe, lesion, shape):
    return {"#image": img.copy(), "#lobe_reference": lobe.copy(), "#lesion_reference": lesion.copy(), "other": 1,
            "meta": {"size": shape}}


def main():
    MG._import_reference()
    import scipy
    import data_transforms as DT
    real_rotate = DT.ndimage.rotate

    def noting_rotate(data, angle, *args, **kw):
        NOTED.append((angle, tuple(kw["axes"])))
        return real_rotate(data, angle, *args, **kw)

    real_affine = DT.affine_transform

    def noting_affine(data, matrix, *args, **kw):
        HANDED.append((np.array(matrix, dtype=np.float64), np.array(kw["offset"], dtype=np.float64)))
        return real_affine(data, matrix, *args, **kw)

    def handed_once():
        """The one (matrix, offset) of a sample's three calls."""
        assert len(HANDED) == 3 and all(np.array_equal(h[0], HANDED[0][0]) and np.array_equal(h[1], HANDED[0][1]) for h in HANDED)
        assert HANDED[0][0].shape == (3, 3) and HANDED[0][1].shape == (3,)
        return HANDED[0]

    DT.affine_transform = noting_affine
    out = {"numpy_version": np.array(np.__version__), "scipy_version": np.array(scipy.__version__),
           "sig/RandomAffineTransform3D": np.array(str(inspect.signature(DT.RandomAffineTransform3D.__init__))),
           "sig/RandomRotate": np.array(str(inspect.signature(DT.RandomRotate.__init__))),
           "rotate_range": np.asarray(ROTATE_RANGE)}
    worst = {}

    def store(case, key, samples):
        out[f"{case}/{key}"] = np.stack(samples)

    def check_types(res, src):
        for k in ("#image", "#lobe_reference", "#lesion_reference"):
            assert res[k].dtype == src[k].dtype and res[k].shape == src[k].shape, k

    # ---- affine and identity
    ins, outs, scales, angles, nxt, edges, mats, offs = [], [], [], [], [], 0, [], []
    for i, seed in enumerate(AFFINE_SEEDS):
        src = sample_dict(*make_input(AFFINE_SHAPE, i), AFFINE_SHAPE)
        ins.append(src)
        if seed is None:
            outs.append(src)
            scales.append([np.nan] * 3)
            angles.append([np.nan] * 3)
            nxt.append(np.nan)
            mats.append(np.full((3, 3), np.nan))
            offs.append(np.full(3, np.nan))
            continue
        np.random.seed(seed)
        del HANDED[:]
        res = DT.RandomAffineTransform3D(3)(sample_dict(src["#image"], src["#lobe_reference"], src["#lesion_reference"], AFFINE_SHAPE))
        nxt.append(np.random.random_sample())
        check_types(res, src)
        outs.append(res)
        scales.append(res["meta"]["RandomAffineTransform3D_scales"])
        angles.append(res["meta"]["RandomAffineTransform3D_rotate_angle"])
        m, off = handed_once()
        mats.append(m)
        offs.append(off)
        edges += int(knife_edges(m, off, AFFINE_SHAPE, True).sum())
        outside = 1.0 - SR.inside(SR.source_coordinates(m, off, AFFINE_SHAPE), AFFINE_SHAPE).mean()
        assert 0.02 < outside < 0.6, outside
    worst["affine"] = edges / (2 * np.prod(AFFINE_SHAPE))
    out["affine/seeds"] = np.asarray([-1 if s is None else s for s in AFFINE_SEEDS])
    out["affine/scales"], out["affine/angles"] = np.asarray(scales, dtype=np.float64), np.asarray(angles, dtype=np.float64)
    out["affine/next_random"] = np.asarray(nxt)
    out["affine/matrix"], out["affine/offset"] = np.stack(mats), np.stack(offs)
    for name, key in (("image", "#image"), ("lobe", "#lobe_reference"), ("lesion", "#lesion_reference")):
        store("affine", "x_" + name, [s[key] for s in ins])
        store("affine", "out_" + name, [s[key] for s in outs])

    src = ins[0]
    del HANDED[:]
    res = DT.RandomAffineTransform3D(3, rotations=(0.0, 0.0, 0.0), scales=(0.0, 0.0, 0.0))(
        sample_dict(src["#image"], src["#lobe_reference"], src["#lesion_reference"], AFFINE_SHAPE))
    check_types(res, src)
    assert res["meta"]["RandomAffineTransform3D_scales"] == [1.0] * 3 and res["meta"]["RandomAffineTransform3D_rotate_angle"] == [0.0] * 3
    m, off = handed_once()
    DT.affine_transform = real_affine
    assert np.array_equal(m, np.eye(3)) and not off.any()
    out["identity/matrix"], out["identity/offset"] = m, off
    assert np.array_equal(res["#lobe_reference"], src["#lobe_reference"]) and np.array_equal(res["#lesion_reference"], src["#lesion_reference"])
    worst["identity"] = float(knife_edges(m, off, AFFINE_SHAPE, True).mean())
    for name, key in (("image", "#image"), ("lobe", "#lobe_reference"), ("lesion", "#lesion_reference")):
        store("identity", "out_" + name, [res[key]])

    # ---- rotate
    DT.ndimage.rotate = noting_rotate
    try:
        for case, shape, wanted, base in (("rotate", ROTATE_SHAPE, ROTATE_WANTED, 10), ("rotate1", FLAT_SHAPE, FLAT_WANTED, 20)):
            ins, outs, seeds, drawn_angle, drawn_axes, nxt, edges = [], [], [], [], [], [], 0
            for i, (angle, axes) in enumerate(wanted):
                src = sample_dict(*make_input(shape, base + i), shape)
                seed = rotate_seed(angle, axes)
                random.seed(seed)
                del NOTED[:]
                res = DT.RandomRotate(3, ROTATE_RANGE)(sample_dict(src["#image"], src["#lobe_reference"], src["#lesion_reference"], shape))
                nxt.append(random.random())
                check_types(res, src)
                assert len(NOTED) == 3 and len(set(NOTED)) == 1 and NOTED[0][0] == angle and (axes is None or NOTED[0][1] == axes)
                ins.append(src)
                outs.append(res)
                seeds.append(seed)
                drawn_angle.append(NOTED[0][0])
                drawn_axes.append(NOTED[0][1])
                m, off = SR.embed_plane(*SR.rotate_plane_matrix(NOTED[0][0], NOTED[0][1], shape))
                edges += int(knife_edges(m, off, shape, True).sum())
            worst[case] = edges / (len(wanted) * np.prod(shape))
            out[f"{case}/seeds"], out[f"{case}/angles"] = np.asarray(seeds), np.asarray(drawn_angle)
            out[f"{case}/axes"], out[f"{case}/next_random"] = np.asarray(drawn_axes), np.asarray(nxt)
            for name, key in (("image", "#image"), ("lobe", "#lobe_reference"), ("lesion", "#lesion_reference")):
                store(case, "x_" + name, [s[key] for s in ins])
                store(case, "out_" + name, [s[key] for s in outs])
    finally:
        DT.ndimage.rotate = real_rotate
    assert len({tuple(sorted(a)) for a in out["rotate/axes"][:3].tolist()}) == 3, "the rotate case misses a plane"
    m, off = SR.embed_plane(*SR.rotate_plane_matrix(90, (-2, -3), ROTATE_SHAPE))
    c = SR.source_coordinates(m, off, ROTATE_SHAPE)
    assert np.array_equal(c, np.round(c)), "the 90 degree sample's coordinates are not integers"

    for case, frac in worst.items():
        assert frac <= 1e-3, f"{case}: {frac:.2%} knife-edge voxels"
    path = os.path.join(MG.OUT, "augment_spline.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB; knife-edge fractions {worst}")
    print("rotate seeds", out["rotate/seeds"], out["rotate/axes"].tolist(), "rotate1 seeds", out["rotate1/seeds"])


if __name__ == "__main__":
    main()
