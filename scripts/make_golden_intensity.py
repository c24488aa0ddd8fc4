"""Writes tests/golden/augment_intensity.npz: the reference's IntensityInverse, GammaTransform, ContrastStretchingTransform and
ContrastJitter (dram/data_transforms.py), run on the CPU under fixed seeds, with the parameters they drew read back out.

Needs the reference checkout (see oracle/make_golden.py for where it is expected); nothing of it is copied: the fixture holds
inputs, outputs in the dtype the reference returned, drawn parameters, the next `np.random` draw after each case, the
constructor signatures as strings and the numpy version.

Per (transform, shape) the generators are seeded once and the three samples go through the transform one after another, as the
reference's loader sends chunk after chunk, so the fixture pins the order of the draws across samples as well.

    python scripts/make_golden_intensity.py
"""
import inspect
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import make_golden as MG  # noqa: E402

SHAPES = {"s5x7x9": (5, 7, 9),          # 315 elements, no multiple of 4; slices of 63 start off a 16-byte boundary
          "s6x8x8": (6, 8, 8),          # aligned rows
          "s24x40x48": (24, 40, 48)}    # more than one block per sample
N = 3
SEED = 31
REC = []                                # parameter records of the worker calls, in call order


def _seed(s):
    random.seed(s)
    np.random.seed(s)


def _instrument(DT):
    """Wrap the worker methods (in this process only) so that every call leaves what it recorded in its `meta` in REC."""
    def wrap(cls, method):
        orig = getattr(cls, method)

        def wrapped(self, data, channel_id, meta):
            out = orig(self, data, channel_id, meta)
            REC.append(meta[channel_id])
            return out
        setattr(cls, method, wrapped)

    wrap(DT.GammaTransform, "_gamma_transform")
    wrap(DT.ContrastStretchingTransform, "_transform")
    wrap(DT.ContrastJitter, "_contrast_jitter")


def _phantom(rng, shape):
    """A large sample that compresses: a smooth field in steps of 1/32 (runs along x whose ends differ from row to row and from
    slice to slice) with 6 % of the voxels replaced by random steps.  Every z-slice has its own mean, minimum and maximum."""
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    a, b, c, d = rng.uniform(0.05, 0.25, 4)
    p = rng.uniform(0, 6.28, 3)
    field = 0.5 + 0.22 * np.sin(a * x + b * y + p[0]) + 0.18 * np.sin(c * y - d * z + p[1]) + 0.08 * np.sin(0.3 * z + p[2])
    field += 0.004 * z
    speck = rng.random(shape) < 0.06
    field[speck] = rng.random(int(speck.sum()))
    return (np.round(field * 32) / 32).astype(np.float32)


def main():
    MG._import_reference()
    import data_transforms as DT
    _instrument(DT)
    rng = np.random.default_rng(2025)
    arrs = {"numpy_version": np.array(np.__version__), "seed": np.array(SEED)}
    for tag, shape in SHAPES.items():
        if tag == "s24x40x48":
            x = np.stack([_phantom(rng, shape) for _ in range(N)])
        else:
            x = rng.random((N,) + shape).astype(np.float32)
        x[1] = x[1] * np.float32(0.75) - np.float32(0.25)       # a sample whose minimum is not near 0
        arrs[f"x/{tag}"] = x
    arrs["x/const"] = np.full((1, 5, 7, 9), 0.37, dtype=np.float32)     # range 0: the epsilon path

    cases = {"inverse": DT.IntensityInverse(), "gamma": DT.GammaTransform(), "stretch": DT.ContrastStretchingTransform(),
             "jitter": DT.ContrastJitter(),                             # the default channel_dim=0: every z-slice on its own
             "jitter_volume": DT.ContrastJitter(channel_dim=None)}
    for name, transform in cases.items():
        arrs[f"{name}/signature"] = np.array(str(inspect.signature(type(transform).__init__)))
        for tag in list(SHAPES) + ["const"]:
            x = arrs[f"x/{tag}"]
            _seed(SEED)
            outs, params = [], []
            for k in range(len(x)):
                del REC[:]
                res = transform({"#image": x[k].copy(), "meta": {}})
                outs.append(np.asarray(res["#image"]))
                assert outs[-1].shape == x[k].shape
                params.append(list(REC))
            arrs[f"{name}/{tag}/next"] = np.array(np.random.random_sample())
            arrs[f"{name}/{tag}/out"] = np.stack(outs)
            if name == "gamma":
                arrs[f"{name}/{tag}/factor"] = np.array([p[0] for p in params])
            elif name == "stretch":
                arrs[f"{name}/{tag}/factor"] = np.array([p[0][0] for p in params])
                arrs[f"{name}/{tag}/mp"] = np.array([p[0][1] for p in params])
            elif name.startswith("jitter"):
                arrs[f"{name}/{tag}/factor"] = np.array(params)          # [N, D] (or [N, 1]) in slice order
            print(name, tag, arrs[f"{name}/{tag}/out"].dtype, [len(p) for p in params])
    MG._save("augment_intensity", **arrs)


if __name__ == "__main__":
    main()
