"""Writes tests/golden/augment_region.npz: the reference's MinimalIntensityProjection, MaximumIntensityProjection,
MinimalIntensityAxialProjection, DiskMaskOut, RandomCubeMask, RandomMoveAxis and RandomRotateInplane90
(dram/data_transforms.py), run on the CPU under fixed seeds, with the parameters they drew read back out.

Needs the reference checkout (see oracle/make_golden.py for where it is expected); nothing of it is copied: the fixture holds
inputs, outputs, drawn parameters, the next `np.random.random_sample()` and `random.random()` after each case, the constructor
signatures as strings and the numpy version.

Per (transform, shape) the generators are seeded once and the three samples go through the transform one after another, as the
reference's loader sends chunk after chunk, so the fixture pins the order of the draws across samples as well.  Three seeded
draws do not reach every axis and thickness of the projections, so `forced/...` holds cases whose ranges leave one choice:
every axis with a thickness of 0, 1, 9 and 16 (the device kernel's largest).

RandomCubeMask.__call__ raises KeyError('crop_sizes_ratio') after its `_mask` has produced the outputs; `_mask` is wrapped (in
this process only) to keep them, the error is caught and recorded as `cube/raised`.

    python scripts/make_golden_region.py
"""
import inspect
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from oracle import make_golden as MG  # noqa: E402
from make_golden_intensity import _phantom  # noqa: E402

SMALL = {"s5x7x9": (5, 7, 9),           # every axis shorter than the largest window; rows odd and off a 16-byte boundary
         "s6x8x8": (6, 8, 8)}           # aligned rows
# The x walk stages 256 columns of a row per pass and a block of either walk covers three or four rows of this width, so every
# axis spans two tiles and more, with a full 17-element window across the seam; W is no multiple of 4.
BIG = {"s18x18x277": (18, 18, 277)}
CUBES = {"s6x6x6": (6, 6, 6), "s7x7x7": (7, 7, 7)}
N = 3
SEED = 54                               # the three draws reach every axis, every pair of RandomMoveAxis, odd and even turns
FORCED_T = (0, 1, 9, 16)
REC = []                                # what the wrapped workers saw, in call order


def _seed(s):
    random.seed(s)
    np.random.seed(s)


def _instrument(DT):
    def wrap_maip(cls):
        orig = cls.maip

        def maip(self, data, meta):
            out = orig(self, data, meta)
            REC.append(dict(meta))
            return out
        cls.maip = maip

    for cls in (DT.MinimalIntensityProjection, DT.MaximumIntensityProjection, DT.MinimalIntensityAxialProjection):
        wrap_maip(cls)

    def wrap(cls, method):
        orig = getattr(cls, method)

        def wrapped(self, data, meta):
            out = orig(self, data, meta)
            REC.append((dict(meta), np.array(out)))
            return out
        setattr(cls, method, wrapped)

    wrap(DT.RandomCubeMask, "_mask")
    wrap(DT.RandomMoveAxis, "_move_axis")
    wrap(DT.RandomRotateInplane90, "_rotate90")


def _run(arrs, name, tag, transform, x, lobe=None):
    """Seed once, send the samples through one after another; returns the per-sample worker records."""
    _seed(SEED)
    outs, lobes, recs, raised = [], [], [], 0
    for k in range(len(x)):
        del REC[:]
        sample = {"#image": x[k].copy(), "meta": {"spacing": (1.0, 1.0, 1.0)}}
        if lobe is not None:
            sample["#lobe_reference"] = lobe[k].copy()
        try:
            res = transform(sample)
            outs.append(np.asarray(res["#image"]))
            if lobe is not None:
                lobes.append(np.asarray(res["#lobe_reference"]))
        except KeyError as e:                       # RandomCubeMask: the outputs are what `_mask` returned
            assert name == "cube" and e.args == ("crop_sizes_ratio",)
            raised += 1
            outs.append(REC[0][1])
            lobes.append(REC[1][1])
        recs.append(list(REC))
        assert outs[-1].shape == x[k].shape and outs[-1].dtype == x.dtype
    arrs[f"{name}/{tag}/next"] = np.array(np.random.random_sample())
    arrs[f"{name}/{tag}/next_random"] = np.array(random.random())
    arrs[f"{name}/{tag}/out"] = np.stack(outs)
    if lobe is not None:
        assert all(o.dtype == np.uint8 for o in lobes)
        arrs[f"{name}/{tag}/out_lobe"] = np.stack(lobes)
    if name == "cube":
        arrs["cube/raised"] = np.array(arrs.get("cube/raised", 0) + raised)
    return recs


def main():
    MG._import_reference()
    import data_transforms as DT
    _instrument(DT)
    rng = np.random.default_rng(2026)
    arrs = {"numpy_version": np.array(np.__version__), "seed": np.array(SEED), "forced_t": np.array(FORCED_T)}
    for tag, shape in {**SMALL, **CUBES, **BIG}.items():
        x = np.stack([_phantom(rng, shape) for _ in range(N)]) if tag in BIG else rng.random((N,) + shape).astype(np.float32)
        x[1] = x[1] * np.float32(0.75) - np.float32(0.25)
        arrs[f"x/{tag}"] = x
        arrs[f"lobe/{tag}"] = (rng.integers(0, 6, (N,) + shape) * (x > np.median(x))).astype(np.uint8)
    three = list(SMALL) + list(BIG)

    proj = {"minip": DT.MinimalIntensityProjection, "maxip": DT.MaximumIntensityProjection,
            "minip_axial": DT.MinimalIntensityAxialProjection}
    for name, cls in proj.items():
        arrs[f"{name}/signature"] = np.array(str(inspect.signature(cls.__init__)))
        for tag in three:
            recs = _run(arrs, name, tag, cls(), arrs[f"x/{tag}"])
            key = "axial_thickness" if name == "minip_axial" else "slab_thickness"      # spacing 1: the same number
            arrs[f"{name}/{tag}/slab_thickness"] = np.array([r[0][key] for r in recs])
            if name != "minip_axial":
                arrs[f"{name}/{tag}/angle"] = np.array([r[0]["angle"] for r in recs])
            print(name, tag, [r[0] for r in recs])
    # forced (axis, thickness): both operations on the small odd shape, one each on the large one
    for tag, ops in (("s5x7x9", ("minip", "maxip")), ("s18x18x277", None)):
        for a in range(3):
            for t in FORCED_T:
                for name in ops or (("maxip",) if t == 9 else ("minip",) if t == 16 else ()):
                    x = arrs[f"x/{tag}"][:1 if ops is None else N]
                    _run(arrs, f"forced/{name}/a{a}t{t}", tag, proj[name](slab_thickness=(t, t + 1), angle=(a, a + 1)), x)

    masks = {"disk": DT.DiskMaskOut(), "cube": DT.RandomCubeMask((0.2,) * 3, (0.5,) * 3)}
    for name, transform in masks.items():
        arrs[f"{name}/signature"] = np.array(str(inspect.signature(type(transform).__init__)))
        for tag in three:
            recs = _run(arrs, name, tag, transform, arrs[f"x/{tag}"], arrs[f"lobe/{tag}"])
            if name == "cube":
                arrs[f"cube/{tag}/shifted_center"] = np.array([r[0][0]["shifted_center"] for r in recs])
                arrs[f"cube/{tag}/crop_sizes"] = np.array([r[0][0]["crop_sizes"] for r in recs])
                print(name, tag, [r[0][0] for r in recs])
    assert arrs["cube/raised"] == N * len(three)

    moves = {"moveaxis": (DT.RandomMoveAxis(3), list(CUBES)), "rot_inplane": (DT.RandomRotateInplane90(3), ["s6x8x8"])}
    for name, (transform, tags) in moves.items():
        arrs[f"{name}/signature"] = np.array(str(inspect.signature(type(transform).__init__)))
        for tag in tags:
            recs = _run(arrs, name, tag, transform, arrs[f"x/{tag}"], arrs[f"lobe/{tag}"])
            key = "sampled_comb" if name == "moveaxis" else "rotate_times"
            arrs[f"{name}/{tag}/{key}"] = np.array([r[0][0][key] for r in recs])
            print(name, tag, arrs[f"{name}/{tag}/{key}"].tolist())
    MG._save("augment_region", **arrs)


if __name__ == "__main__":
    main()
