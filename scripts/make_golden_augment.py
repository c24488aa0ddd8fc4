"""Writes tests/golden/augment.npz: the reference's five training-pool transforms and its ensemble driver, run on the CPU
under fixed seeds, with the parameters they drew read back out.

Needs the reference checkout (see oracle/make_golden.py for where it is expected); nothing of it is copied: the fixture holds
inputs, drawn parameters, outputs, the fp64 noise arrays of GaussianAddictive, and the ensemble's chains of class names.

    python scripts/make_golden_augment.py
"""
import importlib
import logging
import os
import random
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import make_golden as MG  # noqa: E402

ODD, CUBE = (12, 10, 14), (12, 12, 12)
SEEDS = (11, 12, 13)                      # per-transform cases (sample k of the inputs with seed k)
ENSEMBLE_SEEDS = tuple(range(100, 110))   # 10 seeds per aug_ratio
MASK_KW = dict(times=5, region_size=((0.1, 0.5), (0.1, 0.5), (0.1, 0.5)))   # boxes that are not empty on a 12-voxel axis
REC = []                                  # (class name, parameter dict) in call order


def _seed(s):
    random.seed(s)
    np.random.seed(s)


class _Stub(types.ModuleType):
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return None


def _import_job_runner():
    """job_runner pulls in plotting / table / metric libraries that the pool does not use: absent ones become empty modules."""
    for name in ("pandas", "torchvision", "torchvision.transforms", "matplotlib", "matplotlib.pyplot", "matplotlib.font_manager",
                 "matplotlib.collections", "sklearn", "sklearn.metrics", "seaborn", "tensorboardX", "tqdm", "scipy.misc"):
        try:
            mod = importlib.import_module(name)
        except Exception:
            mod = None
        if getattr(mod, "__file__", None) is None:      # absent, or one of oracle.make_golden's bare placeholders
            stub = _Stub(name)
            stub.__dict__.update({k: v for k, v in getattr(mod, "__dict__", {}).items() if not k.startswith("__")})
            sys.modules[name] = stub
    import job_runner
    return job_runner


def _instrument(DT):
    """Wrap the pool elements' worker methods (in this process only) so that every call leaves its parameters in REC."""
    def wrap(cls, method, reader):
        orig = getattr(cls, method)

        def wrapped(self, *args):
            state = np.random.get_state()
            out = orig(self, *args)
            after = np.random.get_state()
            REC.append((cls.__name__, reader(self, args, state)))
            np.random.set_state(after)
            return out
        setattr(cls, method, wrapped)

    def mask_reader(self, args, state):
        data, meta = args
        np.random.set_state(state)      # replay the box values as raw uniforms: uniform(a, b) = a + (b - a) * random_sample()
        u = [np.random.random_sample() for _ in meta["mask_centers"]]
        return {"mask_centers": [tuple(c) for c in meta["mask_centers"]], "mask_sizes": [tuple(s) for s in meta["mask_sizes"]],
                "u": u}

    def noise_reader(self, args, state):
        data, _, meta = args
        np.random.set_state(state)      # replay: the sigma draw, then the noise array
        sigma = np.random.uniform(self.sigma[0], self.sigma[1])
        assert sigma == meta["sigma"]
        return {"sigma": sigma, "noise": np.random.normal(0, sigma, size=data.shape)}

    wrap(DT.GaussianBlur, "gaussian_blur", lambda self, args, state: {"sigma": args[1]["sigma"]})
    wrap(DT.RandomMaskOut, "_mask_out", mask_reader)
    wrap(DT.RandomFlip, "_flip_axis", lambda self, args, state: {"flip_axis": args[1]["flip_axis"]})
    wrap(DT.RandomRotate90, "_rotate90", lambda self, args, state: {"rotate_axis": tuple(args[1]["rotate_axis"]),
                                                                    "rotate_times": args[1]["rotate_times"]})
    wrap(DT.GaussianAddictive, "_gaussian_addictive", noise_reader)


def main():
    MG._import_reference()
    import data_transforms as DT
    _instrument(DT)
    rng = np.random.default_rng(2024)
    arrs = {"seeds": np.array(SEEDS), "odd": rng.random((4,) + ODD).astype(np.float32),
            "cube": rng.random((4,) + CUBE).astype(np.float32),
            "odd_mask": rng.integers(0, 3, (4,) + ODD).astype(np.uint8),
            "cube_mask": rng.integers(0, 3, (4,) + CUBE).astype(np.uint8)}

    def run(tag, transform, images, masks):
        outs, mouts, params = [], [], []
        for k, s in enumerate(SEEDS):
            _seed(s)
            del REC[:]
            res = transform({"#image": images[k].copy(), "#lobe_reference": masks[k].copy(), "meta": {}})
            image_calls = [p for _, p in REC]
            params.append(image_calls[0])
            outs.append(np.asarray(res["#image"]))
            mouts.append(np.asarray(res["#lobe_reference"]))
            assert outs[-1].dtype == np.float32 and outs[-1].shape == images[k].shape
        arrs[f"{tag}/out"] = np.stack(outs)
        if not np.array_equal(np.stack(mouts), masks[:len(SEEDS)]):
            arrs[f"{tag}/mask_out"] = np.stack(mouts)
        for name in params[0]:
            arrs[f"{tag}/{name}"] = np.array([p[name] for p in params])

    run("blur", DT.GaussianBlur((0.3, 0.5), "random"), arrs["odd"], arrs["odd_mask"])
    run("blur_wide", DT.GaussianBlur((0.3, 1.1), "random"), arrs["cube"], arrs["cube_mask"])     # radii up to 4
    run("maskout", DT.RandomMaskOut(**MASK_KW), arrs["odd"], arrs["odd_mask"])
    run("maskout_default", DT.RandomMaskOut(), arrs["cube"], arrs["cube_mask"])                   # empty boxes
    run("flip", DT.RandomFlip(3), arrs["odd"], arrs["odd_mask"])
    run("rotate", DT.RandomRotate90(3), arrs["cube"], arrs["cube_mask"])
    run("noise", DT.GaussianAddictive((0.01, 0.02), None), arrs["odd"], arrs["odd_mask"])
    del arrs["maskout_default/out"]           # equals the input: the boxes are empty; only the draws are checked

    # rotations are drawn from 4 counts x 3 planes; add every combination on the cube with explicit parameters
    combos = [(axis, k) for axis in ((-1, -2), (-1, -3), (-2, -3)) for k in (1, 2, 3)]
    arrs["rotate_all/axis"] = np.array([c[0] for c in combos])
    arrs["rotate_all/times"] = np.array([c[1] for c in combos])
    arrs["rotate_all/out"] = np.stack([DT.RandomRotate90(3)._rotate90(arrs["cube"][0], {"rotate_axis": a, "rotate_times": k})
                                       for a, k in combos])
    arrs["rotate_all/mask_out"] = np.stack([DT.RandomRotate90(3)._rotate90(arrs["cube_mask"][0],
                                                                            {"rotate_axis": a, "rotate_times": k})
                                            for a, k in combos])
    arrs["flip_all/out"] = np.stack([np.flip(arrs["odd"][0], axis=a).copy() for a in (-1, -2, -3)])

    # the ensemble driver: the chain of class names per seed
    JR = _import_job_runner()
    runner = object.__new__(JR.LesionSegChunkTrain)
    runner.logger = logging.getLogger("golden")
    arrs["ensemble/seeds"] = np.array(ENSEMBLE_SEEDS)
    for ratio in (0.5, 1.0):
        runner.settings = types.SimpleNamespace(AUG_RATIO=ratio)
        aug = runner.ensemble_scan_augmentation()
        chains = []
        for s in ENSEMBLE_SEEDS:
            _seed(s)
            del REC[:]
            aug({"#image": arrs["cube"][0].copy(), "meta": {}})
            chains.append(",".join(name for name, _ in REC))
        arrs[f"ensemble/chains_{ratio}"] = np.array(chains)
        print(ratio, chains)
    MG._save("augment", **arrs)


if __name__ == "__main__":
    main()
