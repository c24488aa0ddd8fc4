"""Writes tests/golden/preprocess.json: what the reference's own `Resample` (dram/data_transforms.py:56-211) asks of the
resampler for every one of its modes -- required spacing, new size and interpolator per "#" key.

Needs the reference checkout (see oracle/make_golden.py for where it is expected); nothing of it is copied: the fixture holds
settings and recorded numbers only.  SimpleITK is not installed, so the reference's modules are imported with a stand-in for
it (oracle.make_golden._import_reference) whose image and ResampleImageFilter are filled in here just far enough that the
reference's OWN `utils.resample` and `utils.resample_sitk_image` (dram/utils.py:299-434) run unchanged down to
`ResampleImageFilter.Execute`, whose arguments are recorded -- so the fixture also pins the `new_size is None` arithmetic of
utils.py:365-370, not only Resample.__call__.  (`np.int`, which that code still spells, is aliased for this process.)  No voxel
is resampled: Execute returns an empty image of the requested size.

    python scripts/make_golden_preprocess.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import make_golden as MG  # noqa: E402

# three (spacing, size) inputs in (z, y, x) order; the second is anisotropic in every axis
INPUTS = [((1.0, 0.7, 0.7), (30, 48, 48)), ((2.5, 0.68359375, 0.9), (17, 40, 33)), ((0.8, 0.8, 0.8), (9, 14, 23))]
SIZE = (12, 10, 16)
# mode -> (factor, size, seed)
MODES = {
    "random_spacing": ((0.9, 1.6), None, 5),
    "fixed_factor": (1.5, None, None),
    "fixed_spacing": (1.3, None, None),
    "fixed_spacing/list": ([2.0, 1.1, 0.9], None, None),
    "inplane_spacing_only": ([0.0, 1.2, 1.1], None, None),
    "inplane_resolution_only": (None, SIZE, None),
    "inplane_resolution_z_spacing": ([1.7, 0.0, 0.0], SIZE, None),
    "inplane_resolution_z_jittering": (0.3, SIZE, 6),
    "inplane_resolution_min_z_spacing": ([1.5, 0.0, 0.0], SIZE, None),
    "fixed_spacing_min_in_plane_resolution": ([0.0, 2.1, 2.1], SIZE, None),
    "fixed_spacing_min_in_plane_resolution/scalar": (4.0, SIZE, None),
    "iso_minimal": (None, None, None),
    "fixed_output_size": (None, SIZE, None),
    "fixed_size": (None, SIZE, None),
    "spacing_size_match": ([1.9, 1.4, 1.2], SIZE, None),
}
CALLS = []        # (new_size zyx, new_spacing zyx, interpolator code) per Execute


class _Image:
    def __init__(self, size_xyz, pixelid):
        self.size, self.pixelid, self.spacing = tuple(int(s) for s in size_xyz), pixelid, (1.0,) * 3

    def SetSpacing(self, s):
        self.spacing = tuple(float(v) for v in s)

    def GetSpacing(self):
        return self.spacing

    def GetSize(self):
        return self.size

    def GetDimension(self):
        return 3

    def GetPixelIDValue(self):
        return self.pixelid

    def GetOrigin(self):
        return (0.0,) * 3

    def GetDirection(self):
        return (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


class _Filter:
    def Execute(self, image, new_size, transform, interpolator, origin, new_spacing, direction, fill, pixelid):
        CALLS.append(([int(s) for s in new_size][::-1], [float(s) for s in new_spacing][::-1], interpolator))
        return _Image(new_size, pixelid)


def main():
    if not hasattr(np, "int"):
        np.int = int
    MG._import_reference()
    sitk = sys.modules["SimpleITK"]
    sitk.sitkNearestNeighbor, sitk.sitkLinear = "nearest", "linear"
    sitk.GetImageFromArray = lambda a: _Image(a.shape[::-1], {np.dtype(np.uint8): 1, np.dtype(np.int16): 2}.get(a.dtype, 8))
    sitk.GetArrayFromImage = lambda im: np.zeros(im.size[::-1], dtype=np.uint8)
    sitk.Transform = lambda: None
    sitk.ResampleImageFilter = _Filter
    import data_transforms as DT
    cases = []
    for name, (factor, size, seed) in MODES.items():
        mode = name.split("/")[0]
        for spacing, cur in INPUTS:
            if seed is not None:
                np.random.seed(seed)
            del CALLS[:]
            sample = {"#image": np.zeros(cur, dtype=np.float32), "#lobe_reference": np.zeros(cur, dtype=np.uint8),
                      "#weight_map": np.zeros(cur, dtype=np.float32), "other": 1,
                      "meta": {"spacing": np.asarray(spacing, dtype=np.float64), "size": cur}}
            out = DT.Resample(mode, factor, size)(sample)
            keys = [k for k in sample if "#" in k]
            # (a sample that already has the output size is resampled for its first key only: from the second key on
            #  `new_size` is the first result's shape tuple and utils.resample returns the array as it is, utils.py:415-417)
            same = tuple(CALLS[0][0]) == tuple(cur)
            assert len(CALLS) == (1 if same else len(keys)) and all(c[:2] == CALLS[0][:2] for c in CALLS), CALLS
            assert out["#image"].shape == tuple(CALLS[0][0])
            cases.append({"mode": mode, "factor": factor, "size": size, "seed": seed, "spacing": list(spacing),
                          "current_size": list(cur), "required_spacing": CALLS[0][1], "new_size": CALLS[0][0],
                          "meta_spacing": [float(s) for s in out["meta"]["spacing"]],
                          "interpolator": {k: c[2] for k, c in zip(keys, CALLS)}})
    try:
        DT.Resample("no_such_mode", None, SIZE)({"meta": {"spacing": (1.0,) * 3, "size": (4, 4, 4)}})
        unknown = None
    except Exception as e:
        unknown = type(e).__name__
    path = os.path.join(MG.OUT, "preprocess.json")
    with open(path, "w") as f:
        json.dump({"cases": cases, "unknown_mode_raises": unknown}, f, indent=1)
        f.write("\n")
    print(f"wrote {path}: {len(cases)} cases, {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
