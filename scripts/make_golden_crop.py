"""Writes tests/golden/augment_crop.npz: the reference's RandomCrop(keep_size=True) and StandarizeChannel
(dram/data_transforms.py:582-636, 873-899), run on the CPU under fixed seeds, with the values RandomCrop drew read back out of
the output's meta.

Needs the reference checkout (see oracle/make_golden.py for where it is expected); nothing of it is copied: the fixture holds
inputs, outputs, drawn parameters, the next `np.random.random_sample()` after each case, the constructor signatures as strings
and the numpy version.

SimpleITK is not installed, so the reference's modules are imported with a stand-in for it (oracle.make_golden._import_reference)
that is filled in here just far enough for the reference's OWN RandomCrop -> Resample('fixed_size') -> utils.resample ->
utils.resample_sitk_image to run unchanged down to `ResampleImageFilter.Execute`, which records the array it was handed (the
reference's own padded crop) and returns `oracle.resample_itk` of it: the pad, the slice and every number that reaches the
resampler are the reference's, the resampling grid is the oracle's restatement (SimpleITK absent: parity with the library itself
is unpinned, as everywhere else in the tree).  (`np.int`, which utils.py still spells, is aliased for this process.)

Per case the generators are seeded, the input is made from a seeded numpy Generator and stored.  The seeds were picked so that
the cases reach what main() asserts: a low and a high pad on every axis, a padded position outside in two and in three axes, a
truncated crop (an odd size at the top edge, one voxel shorter than drawn), an axis with a zero tail (cropped to half or less)
and the identity crop; a second shape has a W that is no multiple of 4.  With RandomCrop((0.5,) * 3, (0.4,) * 3) a window of these
two shapes cannot leave the chunk at the top of z (centre + size // 2 never exceeds D for D = 9 or 7) and no seed of 0..39
leaves it in three axes, so beside the cases of that setting there are cases of a wider one, RandomCrop((0.9,) * 3, (0.6,) * 3),
for exactly those; each case records its own constructor arguments.

    python scripts/make_golden_crop.py
"""
import inspect
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import make_golden as MG  # noqa: E402
from oracle import dram_oracle as O  # noqa: E402

SPACING = (1.0, 0.7, 0.7)
BASE = ((0.5, 0.5, 0.5), (0.4, 0.4, 0.4))          # (shift_from_center, crop_sizes_ratio)
WIDE = ((0.9, 0.9, 0.9), (0.6, 0.6, 0.6))
IDENT = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
A, B = (9, 12, 20), (7, 10, 23)
# (shape, seed, setting).  BASE on A: 3 truncated without a pad; 7 high y, zero tail; 12 low y, zero tail; 14 high x; 21 low x,
# zero tail; 24 low z and high x, truncated.  WIDE on A: 21 low in all three axes; 149 high in all three, truncated; 31 high z,
# low y and x.  BASE on B: 6 low z, zero tail; 14 high x, truncated.  WIDE on B: 18 low z, high y and x, truncated.
CASES = ([(A, s, BASE) for s in (3, 7, 12, 14, 21, 24)] + [(A, s, WIDE) for s in (21, 149, 31)] + [(A, 0, IDENT)] +
         [(B, s, BASE) for s in (6, 14)] + [(B, 18, WIDE)])
HANDED = []       # the arrays Execute was handed, in call order


class _Image:
    def __init__(self, array):
        self.array, self.spacing = array, (1.0,) * 3

    def SetSpacing(self, s):
        self.spacing = tuple(float(v) for v in s)

    def GetSpacing(self):
        return self.spacing

    def GetSize(self):
        return tuple(int(s) for s in self.array.shape[::-1])

    def GetDimension(self):
        return 3

    def GetPixelIDValue(self):
        return {np.dtype(np.uint8): 1, np.dtype(np.int16): 2}.get(self.array.dtype, 8)

    def GetOrigin(self):
        return (0.0,) * 3

    def GetDirection(self):
        return (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


class _Filter:
    def Execute(self, image, new_size, transform, interpolator, origin, new_spacing, direction, fill, pixelid):
        HANDED.append(image.array.copy())
        out = O.resample_itk(image.array, image.spacing[::-1], [float(s) for s in new_spacing][::-1],
                             [int(s) for s in new_size][::-1], interpolator)
        return _Image(out)


def make_input(shape, seed):
    """A smooth ramp plus noise on a 1/8 grid (so that minima along different axes differ) and a label volume."""
    rng = np.random.default_rng(1000 + seed)
    z, y, x = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    img = (z * 3 - y * 2 + x + rng.integers(-40, 40, size=shape)) / 8.0
    return img.astype(np.float32), rng.integers(0, 6, size=shape).astype(np.uint8)


def coverage(padding, crop_sizes, crop_shape, shape):
    low = [p[0] > 0 for p in padding]
    high = [p[1] > 0 for p in padding]
    axes_out = sum(1 for lo, hi in zip(low, high) if lo or hi)
    return {"low": low, "high": high, "axes_out": axes_out, "truncated": tuple(crop_shape) != tuple(crop_sizes),
            "zero_tail": any(2 * c <= d for c, d in zip(crop_shape, shape))}


def main():
    if not hasattr(np, "int"):
        np.int = int
    MG._import_reference()
    sitk = sys.modules["SimpleITK"]
    sitk.sitkNearestNeighbor, sitk.sitkLinear = "nearest", "linear"
    sitk.GetImageFromArray = lambda a: _Image(a)
    sitk.GetArrayFromImage = lambda im: im.array
    sitk.Transform = lambda: None
    sitk.ResampleImageFilter = _Filter
    import data_transforms as DT
    out = {"numpy_version": np.array(np.__version__), "spacing": np.asarray(SPACING, dtype=np.float64),
           "sig/RandomCrop": np.array(str(inspect.signature(DT.RandomCrop.__init__))),
           "sig/StandarizeChannel": np.array(str(inspect.signature(DT.StandarizeChannel.__init__)))}
    seen = []
    for i, (shape, seed, (shift, ratio)) in enumerate(CASES):
        x, lobe = make_input(shape, seed)
        t = DT.RandomCrop(shift, ratio)
        np.random.seed(seed)
        del HANDED[:]
        sample = {"#image": x.copy(), "#lobe_reference": lobe.copy(), "other": 1,
                  "meta": {"spacing": np.asarray(SPACING, dtype=np.float64), "size": shape}}
        res = t(sample)
        nxt = np.random.random_sample()
        meta = res["meta"]
        assert res["#image"].dtype == np.float32 and res["#lobe_reference"].dtype == np.uint8
        assert res["#image"].shape == shape and res["#lobe_reference"].shape == shape
        # (an identity crop is resampled for its first key only: from the second key on `new_size` is the first result's
        #  shape tuple and utils.resample returns the array as it is, utils.py:415-417)
        crop_img = HANDED[0]
        crop_lobe = HANDED[1] if len(HANDED) > 1 else res["#lobe_reference"]
        assert crop_img.dtype == np.float32 and crop_lobe.dtype == np.uint8 and crop_img.shape == crop_lobe.shape
        pre = f"case{i}/"
        out[pre + "shape"] = np.asarray(shape)
        out[pre + "seed"] = np.asarray(seed)
        out[pre + "shift_from_center"], out[pre + "ratio"] = np.asarray(shift), np.asarray(ratio)
        out[pre + "x"], out[pre + "lobe"] = x, lobe
        out[pre + "crop_sizes_ratio"] = np.asarray(meta["RandomCrop_crop_sizes_ratio"], dtype=np.float64)
        out[pre + "crop_sizes"] = np.asarray(meta["RandomCrop_crop_sizes"])
        out[pre + "offset"] = np.asarray(meta["RandomCrop_offset"])
        out[pre + "shifted_center"] = np.asarray(meta["RandomCrop_shifted_center"])
        out[pre + "padding"] = np.asarray(meta["RandomCrop_padding"])
        out[pre + "padding_mode"] = np.array(meta["RandomCrop_padding_mode"])
        out[pre + "next_random"] = np.asarray(nxt)
        out[pre + "crop_image"], out[pre + "crop_lobe"] = crop_img, crop_lobe
        out[pre + "out_image"], out[pre + "out_lobe"] = res["#image"], res["#lobe_reference"]
        out[pre + "meta_spacing"] = np.asarray(meta["spacing"], dtype=np.float64)
        seen.append(coverage(meta["RandomCrop_padding"], meta["RandomCrop_crop_sizes"], crop_img.shape, shape))
        if (shift, ratio) == IDENT:
            assert np.array_equal(res["#image"], x) and np.array_equal(res["#lobe_reference"], lobe)
    out["n_cases"] = np.asarray(len(CASES))
    for ax in range(3):
        assert any(c["low"][ax] for c in seen) and any(c["high"][ax] for c in seen), f"axis {ax}: no low or no high pad"
    assert any(c["axes_out"] == 2 for c in seen) and any(c["axes_out"] == 3 for c in seen), "no two- / three-axis pad"
    assert any(c["truncated"] for c in seen) and any(c["zero_tail"] for c in seen)
    assert any(c[2] == IDENT for c in CASES) and any(c[0][2] % 4 for c in CASES)

    # StandarizeChannel: a 3-d sample as a whole, a 4-d sample per index along ch_dim 0
    x3, _ = make_input((9, 12, 20), 3)
    x4 = np.stack([make_input((9, 12, 20), s)[0] * (s + 1) - s for s in (40, 41, 42)], axis=0)
    out["stand/x3"], out["stand/x4"] = x3, x4
    out["stand/out3"] = DT.StandarizeChannel(0)({"#image": x3.copy(), "meta": {}})["#image"]
    out["stand/out4"] = DT.StandarizeChannel(0)({"#image": x4.copy(), "meta": {}})["#image"]
    assert out["stand/out3"].dtype == np.float32 and out["stand/out4"].shape == x4.shape

    path = os.path.join(MG.OUT, "augment_crop.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(CASES)} cases, {os.path.getsize(path) / 1024:.1f} KiB")
    for (shape, seed, _), c in zip(CASES, seen):
        print(shape, seed, c)


if __name__ == "__main__":
    main()
