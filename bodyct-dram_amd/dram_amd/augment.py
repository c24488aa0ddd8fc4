"""The reference's training-time augmentation pool on a whole device batch.

`LesionSegChunkTrain.ensemble_scan_augmentation` (dram/job_runner.py:548-581) draws, for every chunk, a random order of
`GaussianBlur`, `RandomMaskOut`, `RandomFlip`, `RandomRotate90` and `GaussianAddictive` (dram/data_transforms.py) and applies a
random subset with numpy / scipy on the host.  The classes here keep those names, constructor signatures and defaults, and use
the sample-dict protocol of `transforms.py`: entries whose key contains "#" hold device tensors [N, D, H, W] or [N, 1, D, H, W];
the intensity transforms touch keys with both "#" and "image", flip and rotate touch every "#" key, everything else passes
through.  The work runs in per-batch launches of csrc/augment.hip over per-sample parameter tables: no host synchronisation.

Beside the pool's five, four more intensity transforms of data_transforms.py are here for pools of the user's own
(`EnsembleScanAugmentation(aug_ratio, pool=[...])`): `IntensityInverse`, `GammaTransform`, `ContrastStretchingTransform` and
`ContrastJitter`; the slab projections `MinimalIntensityProjection`, `MaximumIntensityProjection` and
`MinimalIntensityAxialProjection`; the region masks `DiskMaskOut` and `RandomCubeMask`; and the axis moves `RandomMoveAxis` and
`RandomRotateInplane90`; the scale-and-translate augmentation `RandomCrop` (pad, crop, resample back to the chunk's size);
`StandarizeChannel`; and the two spline-resampled geometric transforms `RandomAffineTransform3D` and `RandomRotate`
(csrc/spline.hip: cubic B-spline for the image, nearest neighbour for every other entry).

Drawing.  `draw(n, shape)` returns one parameter dict per sample, in sample order, from the same `random` / `numpy.random`
calls in the same order as the reference's `__call__` makes for one chunk, so a seeded run picks what the reference would pick
for that chunk.  (The reference draws an intensity transform's parameters once per "#image" entry; here one set per sample
serves every image entry, which is the same thing for the single-image samples of training.)  `apply(sample, params)` runs with
given parameters; an entry of `params` that is None leaves that sample untouched (bit-identical).
"""
import itertools
import math
import random

import numpy as np
import torch

from . import functional as HF
from . import _lib
from ._lib import call

MAX_RADIUS = 4     # DRAM_AUG_MAX_RADIUS
MAX_BOXES = 16     # DRAM_AUG_MAX_BOXES
MAX_SLAB = 16      # DRAM_AUG_MAX_SLAB
TRANSFORM, PASS, SKIP = 1, 0, -1   # per-sample flags of the C entries
MAP_INVERSE, MAP_GAMMA, MAP_STRETCH, MAP_JITTER, MAP_STANDARDIZE = 0, 1, 2, 3, 5   # DRAM_AUG_MAP_*
PAD_MODES = {"constant": 0, "edge": 1, "minimum": 2}     # DRAM_AUG_PAD_*
MAX_W = 2048       # csrc/crop.hip CROP_MAX_W / PAD_MAX_DIM
# one record per sample (csrc/crop.hip: CropRec): window start (z, y, x), actual crop size, pad mode, output-to-crop index steps
CROP_DTYPE = np.dtype([("z0", "<i4"), ("y0", "<i4"), ("x0", "<i4"), ("cd", "<i4"), ("ch", "<i4"), ("cw", "<i4"),
                       ("mode", "<i4"), ("pad", "<i4"), ("sz", "<f8"), ("sy", "<f8"), ("sx", "<f8")])
assert CROP_DTYPE.itemsize == 56
# one record per sample (csrc/spline.hip: SplineRec): source = m * (z, y, x) + off; fixed = the axis a plane transform leaves alone
SPLINE_DTYPE = np.dtype([("m", "<f8", (9,)), ("off", "<f8", (3,)), ("fixed", "<i4"), ("pad", "<i4")])
assert SPLINE_DTYPE.itemsize == 104
ROTATE_PLANES = [(-1, -2), (-1, -3), (-2, -3)]     # RandomRotate's planes, in the order of itertools.combinations([-1, -2, -3], 2)


# ---------------------------------------------------------------------------------------------------------------- tables
def blur_radius(sigma, truncate=4.0):
    return int(truncate * float(sigma) + 0.5)


def blur_weights(sigma, truncate=4.0):
    """The normalised 1-D kernel scipy.ndimage.gaussian_filter1d uses for `sigma` (fp64, length 2 * radius + 1)."""
    sigma = float(sigma)
    radius = blur_radius(sigma, truncate)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum()


def mask_boxes(centers, sizes, shape):
    """RandomMaskOut._mask_out's slices as rows (z0, z1, y0, y1, x0, x1), half-open; an empty box has z1 <= z0 etc."""
    rows = []
    for center, size in zip(centers, sizes):
        row = []
        for c, s, dim in zip(center, size, shape):
            row += [max(0, c - s // 2), min(c + (s - s // 2), dim)]
        rows.append(row)
    return rows


def cube_box(center, size, shape):
    """RandomCubeMask._mask's slices as one row (z0, z1, y0, y1, x0, x1), half-open: the box of `mask_boxes` for one centre."""
    return mask_boxes([center], [size], shape)[0]


def disk_table(shape):
    """DiskMaskOut's disk in every z-slice as (cy, cx, r^2): centre (H // 2, W // 2), radius min(H, W) // 2, rim included."""
    return [shape[1] // 2, shape[2] // 2, (min(shape[1], shape[2]) // 2) ** 2]


def moveaxis_table(comb, shape):
    """np.moveaxis(data, comb[0], comb[1]) for negative spatial axes as (perm, flip): the moved axis changes place with its
    neighbours one after another ((-1, -3) is a 3-cycle: two transposes).  A move that changes the sample's shape cannot live in
    a batch tensor."""
    a, b = (v % 5 for v in comb)
    if min(a, b) < 2:
        raise ValueError(f"RandomMoveAxis: axes {tuple(comb)} are not spatial axes")
    step = 1 if b > a else -1
    perm, _ = HF.signed_permutation([("transpose", j, j + step) for j in range(a, b, step)])
    if tuple(shape[k] for k in perm) != tuple(shape):
        raise ValueError(f"moving axis {comb[0]} to {comb[1]} turns extents {tuple(shape)} into "
                         f"{tuple(shape[k] for k in perm)}: it changes the sample's shape and cannot live in a batch tensor")
    return perm, (0, 0, 0)


def flip_table(axis):
    """np.flip(data, axis) for a negative spatial axis as (perm, flip) of dram_aug_permute_flip."""
    return HF.signed_permutation([("flip", (axis % 5,))])


def rotate_table(axis, times, shape):
    """np.rot90(data, k=times, axes=axis) for negative spatial axes as (perm, flip).  A quarter turn by an odd count between
    axes of different extents changes the sample's shape, which a batch tensor cannot hold."""
    a, b = (v % 5 for v in axis)
    if times % 2 and shape[a - 2] != shape[b - 2]:
        raise ValueError(f"a rotation by {times} quarter turns in a plane of unequal extents {shape[a - 2]} x {shape[b - 2]} "
                         f"changes the sample's shape and cannot live in a batch tensor (cubic chunks only)")
    return HF.signed_permutation(HF.rot90_ops(times, (a, b)))


def crop_window(params, shape):
    """RandomCrop._crop's slice in chunk coordinates: (start, size) per axis.  The reference pads by `padding` and slices
    [cc - s // 2 + p0 : cc + (s - s // 2) + p0]; the upper pad is max(0, cc + s // 2 - dim), so for an odd s that reaches the
    top edge the slice runs one past the padded array and numpy truncates it: the crop is then one voxel shorter than
    `crop_sizes`.  `start` is negative where the window begins in the lower pad."""
    start, size = [], []
    for cc, s, (p0, p1), dim in zip(params["shifted_center"], params["crop_sizes"], params["padding"], shape):
        lo = cc - s // 2
        hi = min(cc + (s - s // 2), dim + p1)
        start.append(int(lo))
        size.append(int(hi - lo))
    return tuple(start), tuple(size)


def pad_crop(x, params, mode="minimum"):
    """The reference's pad and slice of one [D, H, W] array in numpy (RandomCrop._crop), for the tests and the bench."""
    padding = [tuple(int(v) for v in p) for p in params["padding"]]
    padded = np.pad(x, padding, mode=mode)
    start, size = crop_window(params, x.shape)
    return padded[tuple(slice(st + p[0], st + p[0] + sz) for st, sz, p in zip(start, size, padding))]


def _homogeneous(lin, shift=(0.0, 0.0, 0.0)):
    h = np.eye(4)
    h[:3, :3] = lin
    h[:3, 3] = shift
    return h


def affine_matrix(scales, angles, shape):
    """RandomAffineTransform3D._affine's output-to-input map as (3 x 3 matrix, offset), fp64: the inverse (np.linalg.inv) of
    T1 . rotz . roty . rotx . T0, multiplied from the right as the reference multiplies them -- T0 scales and moves the centre
    shape / 2 to the origin, rotz / roty / rotx turn about the third / second / first axis of the array, T1 moves back."""
    half = [n / 2.0 for n in shape]
    (ca, sa), (cb, sb), (ct, st) = [(math.cos(v), math.sin(v)) for v in angles]
    T0 = _homogeneous(np.diag([scales[0], scales[1], scales[2]]), [-v for v in half])
    rotz = _homogeneous([[ca, -sa, 0], [sa, ca, 0], [0, 0, 1]])
    roty = _homogeneous([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    rotx = _homogeneous([[1, 0, 0], [0, ct, -st], [0, st, ct]])
    T1 = _homogeneous(np.eye(3), half)
    inv = np.linalg.inv(T1.dot(rotz.dot(roty.dot(rotx.dot(T0)))))
    return inv[:3, :3].copy(), inv[:3, 3].copy()


def rotate_matrix(angle, axes, shape):
    """scipy.ndimage.rotate(reshape=False) by `angle` degrees in the plane of the (negative) spatial axes `axes`, as (3 x 3
    matrix, offset, fixed axis): scipy sorts the two axes, turns every plane with [[c, s], [-s, c]] (cosdg / sindg: exact at
    multiples of 90) about the centre (n - 1) / 2 of each plane axis, and leaves the third axis alone."""
    from scipy import special
    plane = sorted(a % 3 for a in axes)
    if len(plane) != 2 or plane[0] == plane[1]:
        raise ValueError(f"RandomRotate: {tuple(axes)} is no plane of a 3-d sample")
    c, s = special.cosdg(angle), special.sindg(angle)
    rot = np.array([[c, s], [-s, c]])
    centre = (np.asarray([shape[a] for a in plane], dtype=np.float64) - 1) / 2
    shift = centre - rot @ centre
    m, off = np.eye(3), np.zeros(3)
    for i, a in enumerate(plane):
        off[a] = shift[i]
        m[a, a] = 0.0
        for j, b in enumerate(plane):
            m[a, b] = rot[i, j]
    return m, off, 3 - plane[0] - plane[1]


def _dev(values, dtype, device):
    """A small parameter table on the device.  From pinned memory, so that the copy neither waits for the stream nor outlives its
    source: the pinned block is recycled only after the copy has run."""
    t = torch.tensor(values, dtype=dtype)
    if torch.device(device).type != "cuda":
        return t.to(device)
    return t.pin_memory().to(device, non_blocking=True)


def _flags(params, device):
    return _dev([TRANSFORM if p is not None else PASS for p in params], torch.int32, device)


def _as_batch(t, name, dtypes=(torch.float32,)):
    """[N, D, H, W] or [N, C, D, H, W] device tensor -> (contiguous 5-d view, original shape)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: tensor is on {t.device}; the augmentation kernels only run on a ROCm device "
                           f"(there is no CPU fallback)")
    if t.dtype not in dtypes:
        raise TypeError(f"{name}: expected {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
    if t.dim() not in (4, 5):
        raise ValueError(f"{name}: expected [N, D, H, W] or [N, C, D, H, W], got shape {tuple(t.shape)}")
    shape = tuple(t.shape)
    t = t.contiguous()
    return (t.unsqueeze(1) if t.dim() == 4 else t), shape


def _as_image(t, name):
    v, shape = _as_batch(t, name)
    if v.shape[1] != 1:
        raise ValueError(f"{name}: the intensity transforms work on single-channel samples, got shape {shape}")
    return v, shape


# --------------------------------------------------------------------------------------------- batched device primitives
# Each takes the 5-d view, per-sample DEVICE tables and an int32 flag tensor (TRANSFORM / PASS / SKIP), and an optional `out`.
def sample_minmax(x, flags=None, out=None):
    """[N, 2] fp32 {min, max} of every sample (deterministic).  Rows whose flag is not TRANSFORM are left untouched."""
    x, _ = _as_batch(x, "minmax input")
    N = x.shape[0]
    mm = out if out is not None else torch.empty((N, 2), dtype=torch.float32, device=x.device)
    call("dram_aug_minmax", HF._p(x), HF._p(mm), HF._p(flags), N, x[0].numel(), HF._stream())
    return mm


def _rows(x, rows):
    """(R, L) of the 5-d view split into `rows` rows per sample."""
    return x.shape[0] * rows, x[0].numel() // rows


def row_minmax(x, rows, flags=None):
    """[N * rows, 2] fp32 {min, max} of every sample cut into `rows` equal rows (rows = D: its z-slices); `flags` per row."""
    R, L = _rows(x, rows)
    mm = torch.empty((R, 2), dtype=torch.float32, device=x.device)
    call("dram_aug_minmax", HF._p(x), HF._p(mm), HF._p(flags), R, L, HF._stream())
    return mm


def row_mean(x, rows, flags=None):
    """[N * rows] fp32 mean of every row (fp64 sums added in a fixed order: deterministic); `flags` per row."""
    R, L = _rows(x, rows)
    mean = torch.empty((R,), dtype=torch.float32, device=x.device)
    nbytes = _lib.lib.dram_aug_row_mean_ws_bytes(R, L)
    ws = HF._ws(nbytes, x.device)
    call("dram_aug_row_mean", HF._p(x), HF._p(mean), HF._p(flags), R, L, HF._p(ws), nbytes, HF._stream())
    return mean


def _intensity_map(x, mode, minmax, mean, par, keep_range, flags, rows=1, out=None):
    R, L = _rows(x, rows)
    y = torch.empty_like(x) if out is None else out
    call("dram_aug_intensity_map", HF._p(x), HF._p(y), mode, HF._p(minmax), HF._p(mean), HF._p(par), int(bool(keep_range)),
         HF._p(flags), flags.numel(), R, L, HF._stream())
    return y


def _blur(x, weights, flags, radius, out=None):
    N, _, D, H, W = x.shape
    y = torch.empty_like(x) if out is None else out
    call("dram_aug_gaussian_blur", HF._p(x), HF._p(y), HF._p(weights), HF._p(flags), flags.numel(), int(radius), N, D, H, W,
         HF._stream())
    return y


def _mask_out(x, minmax, boxes, u, flags, out=None):
    N, _, D, H, W = x.shape
    y = torch.empty_like(x) if out is None else out
    call("dram_aug_mask_out", HF._p(x), HF._p(y), HF._p(minmax), HF._p(boxes), HF._p(u), HF._p(flags), flags.numel(),
         boxes.shape[1], N, D, H, W, HF._stream())
    return y


def _noise(x, minmax, sigma, seeds, flags, noise=None, out=None):
    N = x.shape[0]
    y = torch.empty_like(x) if out is None else out
    call("dram_aug_gaussian_noise", HF._p(x), HF._p(y), HF._p(minmax), HF._p(sigma), HF._p(seeds), HF._p(flags), flags.numel(),
         HF._p(noise), N, x[0].numel(), HF._stream())
    return y


def _permute_flip(x, perm, flip, flags, out=None):
    N, C, D, H, W = x.shape
    y = torch.empty_like(x) if out is None else out
    call("dram_aug_permute_flip", HF._p(x), HF._p(y), x.element_size(), HF._p(perm), HF._p(flip), HF._p(flags), flags.numel(),
         N, C, D, H, W, HF._stream())
    return y


def slab_project(x, thickness, axis, is_max, flags, out=None):
    """y[.., i, ..] = min (max when is_max) of x[.., max(0, i - t) .. i, ..] along the sample's axis (0 = z, 1 = y, 2 = x);
    thickness, axis: [N] int32 device tables.  Not in place."""
    N, _, D, H, W = x.shape
    y = torch.empty_like(x) if out is None else out
    call("dram_aug_slab_project", HF._p(x), HF._p(y), HF._p(thickness), HF._p(axis), int(bool(is_max)), HF._p(flags),
         flags.numel(), N, D, H, W, HF._stream())
    return y


def keep_region(x, boxes, disk, flags, out=None):
    """x inside the sample's half-open box (and disk, when its r^2 >= 0), 0 elsewhere; boxes [N, 6], disk [N, 3] int32 device
    tables; fp32 or uint8; `out` may be x."""
    N, C, D, H, W = x.shape
    y = torch.empty_like(x) if out is None else out
    call("dram_aug_keep_region", HF._p(x), HF._p(y), x.element_size(), HF._p(boxes), HF._p(disk), HF._p(flags), flags.numel(),
         N, C, D, H, W, HF._stream())
    return y


def pad_min(x, flags):
    """(workspace, bytes) of dram_aug_pad_min: the min projections np.pad(mode='minimum') needs, for the samples whose flag is
    TRANSFORM; fp32 or uint8."""
    N, _, D, H, W = x.shape
    nbytes = _lib.lib.dram_aug_pad_min_ws_bytes(N, D, H, W, x.element_size())
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    call("dram_aug_pad_min", HF._p(x), x.element_size(), HF._p(flags), N, D, H, W, HF._p(ws), nbytes, HF._stream())
    return ws, nbytes


def crop_resample(x, table, flags, linear, pad_ws=None, out=None):
    """The window of every sample (table: N CROP_DTYPE records as a uint8 device tensor) stretched back to (D, H, W); `pad_ws`:
    what `pad_min` returned, for the samples that pad with 'minimum'.  Not in place."""
    N, _, D, H, W = x.shape
    y = torch.empty_like(x) if out is None else out
    ws, nbytes = pad_ws if pad_ws is not None else (None, 0)
    call("dram_aug_crop_resample", HF._p(x), HF._p(y), x.element_size(), int(bool(linear)), HF._p(table), HF._p(ws), nbytes,
         HF._p(flags), flags.numel(), N, D, H, W, HF._stream())
    return y


def sample_min_table(x, flags=None):
    """[N, 2] fp32 {min, max} of every fp32 or uint8 sample: what `spline_resample` fills with."""
    if x.dtype == torch.float32:
        return sample_minmax(x, flags)
    N = x.shape[0]
    mm = torch.empty((N, 2), dtype=torch.float32, device=x.device)
    call("dram_aug_minmax_u8", HF._p(x), HF._p(mm), HF._p(flags), N, x[0].numel(), HF._stream())
    return mm


def spline_prefilter(x, axes, flags):
    """(workspace, bytes): the fp64 cubic B-spline coefficients [N, D, H, W] of the fp32 samples whose flag is TRANSFORM,
    filtered along the axes of the sample's mask (`axes`: [N] int32 device table, bit 0 = z, 1 = y, 2 = x).  The workspace is
    allocated here on every call and is 8 bytes per voxel of the whole batch -- twice the tensor itself, 1 GiB at 64 x 128^3 --,
    transient memory to count when sizing a batch; it goes back to torch's caching allocator once the gather has run."""
    N, _, D, H, W = x.shape
    nbytes = _lib.lib.dram_aug_spline_ws_bytes(N, D, H, W)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x.device)
    call("dram_aug_spline_prefilter", HF._p(x), HF._p(axes), HF._p(flags), flags.numel(), N, D, H, W, HF._p(ws), nbytes,
         HF._stream())
    return ws, nbytes


def spline_resample(x, table, minmax, flags, order, coef=None, out=None):
    """Every sample resampled at source = m * index + off (table: N SPLINE_DTYPE records as a uint8 device tensor), `minmax[n, 0]`
    where the source lies outside; order 3 (fp32, `coef` = what `spline_prefilter` returned) or order 0.  Not in place."""
    N, _, D, H, W = x.shape
    y = torch.empty_like(x) if out is None else out
    ws, nbytes = coef if coef is not None else (None, 0)
    call("dram_aug_spline_resample", HF._p(x), HF._p(y), x.element_size(), int(order), HF._p(table), HF._p(minmax), HF._p(ws),
         nbytes, HF._p(flags), flags.numel(), N, D, H, W, HF._stream())
    return y


def row_mean_std(x, rows, flags=None):
    """[N * rows, 2] fp32 {mean, std} of every row: fp64 sums in a fixed order (deterministic), the std of the centred fp32
    values in numpy's population form; `flags` per row."""
    R, L = _rows(x, rows)
    ms = torch.empty((R, 2), dtype=torch.float32, device=x.device)
    nbytes = _lib.lib.dram_aug_row_mean_std_ws_bytes(R, L)
    ws = HF._ws(nbytes, x.device)
    call("dram_aug_row_mean_std", HF._p(x), HF._p(ms), HF._p(flags), R, L, HF._p(ws), nbytes, HF._stream())
    return ms


def gaussian_noise(x, minmax, sigma, seeds, noise=None):
    """The noise kernel with explicit tables (every sample active): x [N, ...] fp32, minmax [N, 2] device tensor, sigma and
    seeds sequences of N.  `noise`: optional [N, ...] float64 device tensor used instead of the in-kernel generator."""
    v, shape = _as_image(x, "noise input")
    N = v.shape[0]
    if len(sigma) != N or len(seeds) != N:
        raise ValueError("gaussian_noise: one sigma and one seed per sample")
    if noise is not None and (noise.dtype != torch.float64 or noise.numel() != v.numel() or not noise.is_cuda):
        raise ValueError("gaussian_noise: the explicit noise is a float64 device tensor of the input's shape")
    y = _noise(v, minmax.contiguous(), _dev([float(s) for s in sigma], torch.float32, v.device),
               _dev([int(s) for s in seeds], torch.int64, v.device), _dev([TRANSFORM] * N, torch.int32, v.device),
               None if noise is None else noise.contiguous())
    return y.view(shape)


# ------------------------------------------------------------------------------------------------------------ transforms
def _first_tensor(sample):
    for key, value in sample.items():
        if "#" in key:
            return value
    raise ValueError("the sample holds no '#' entry")


class _Augmentation:
    """draw / apply / __call__ shared by the transforms."""
    intensity = True      # True: touches '#...image...' entries only; False: every '#' entry
    pointwise = False     # True: every element is read and written by one lane, so the ensemble driver may run it in place
    uses_minmax = False   # True: _launch takes the samples' {min, max} (minmax=), which the ensemble driver computes for it

    def draw_one(self, shape):   # pragma: no cover - overridden
        raise NotImplementedError

    def draw(self, n, shape):
        """One parameter dict per sample, in sample order; `shape` = the spatial extents (D, H, W)."""
        return [self.draw_one(tuple(shape)) for _ in range(n)]

    def _touches(self, key):
        return "#" in key and ("image" in key or not self.intensity)

    def _tables(self, params, shape, device):   # pragma: no cover - overridden
        raise NotImplementedError

    def _launch(self, x, tables, flags, out=None):   # pragma: no cover - overridden
        raise NotImplementedError

    def _launch_key(self, key, x, tables, flags, out=None, **kw):
        """`_launch` for the entry `key` of the sample dict (for the transforms that treat keys differently)."""
        return self._launch(x, tables, flags, out, **kw)

    def apply(self, sample, params):
        """`params`: one entry per sample (a dict as `draw` returns it, or None = leave the sample untouched)."""
        out, tables = {}, None
        for key, value in sample.items():
            if not self._touches(key):
                out[key] = value
                continue
            dtypes = (torch.float32,) if self.intensity else (torch.float32, torch.uint8)
            v, shape = (_as_image(value, key) if self.intensity else _as_batch(value, key, dtypes))
            if len(params) != v.shape[0]:
                raise ValueError(f"{type(self).__name__}: {len(params)} parameter sets for a batch of {v.shape[0]}")
            if tables is None:
                tables = self._tables(params, tuple(v.shape[2:]), v.device)
                flags = _flags(params, v.device)
            out[key] = self._launch_key(key, v, tables, flags).view(shape)
        return out

    def __call__(self, sample):
        first = _first_tensor(sample)
        return self.apply(sample, self.draw(first.shape[0], tuple(first.shape[-3:])))


class GaussianBlur(_Augmentation):
    """scipy.ndimage.gaussian_filter(chunk, sigma) per sample: sigma[0] when mode == 'fixed', otherwise one
    np.random.uniform(sigma[0], sigma[1]) draw.  Radius int(4 * sigma + 0.5), at most 4 (sigma < 1.125)."""

    def __init__(self, sigma, mode='fixed'):
        self.sigma = sigma
        self.mode = mode

    def draw_one(self, shape):
        return {"sigma": self.sigma[0] if self.mode == 'fixed' else np.random.uniform(self.sigma[0], self.sigma[1])}

    def _tables(self, params, shape, device):
        rows, radius = [], 0
        for p in params:
            row = [0.0] * (MAX_RADIUS + 1)
            if p is not None:
                r = blur_radius(p["sigma"])
                if r > MAX_RADIUS:
                    raise ValueError(f"GaussianBlur: sigma {p['sigma']} needs radius {r}; the kernel supports at most {MAX_RADIUS}")
                w = blur_weights(p["sigma"])
                row[:r + 1] = [float(v) for v in w[r:]]
                radius = max(radius, r)
            rows.append(row)
        return _dev(rows, torch.float32, device), radius

    def _launch(self, x, tables, flags, out=None):
        return _blur(x, tables[0], flags, tables[1], out)


class RandomMaskOut(_Augmentation):
    """`times` boxes per sample, centre int(dim * U(region_range)) and size int(U(region_size) * dim) per axis, each filled with
    one value min + (max - min) * u of the sample's own range (taken before any box is written).  `assign_value` is unused, as in
    the reference."""
    pointwise = uses_minmax = True

    def __init__(self, times=5, region_range=((0.2, 0.8), (0.2, 0.8), (0.2, 0.8)),
                 region_size=((0.01, 0.06), (0.01, 0.06), (0.01, 0.06)), spatial_dim=3, assign_value=0):
        self.region_range = region_range
        self.region_size = region_size
        self.spatial_dim = spatial_dim
        self.assign_value = assign_value
        self.times = times
        assert (len(region_range) == spatial_dim == len(region_size))
        if spatial_dim != 3 or not 1 <= times <= MAX_BOXES:
            raise NotImplementedError(f"RandomMaskOut: supported: spatial_dim 3, times 1..{MAX_BOXES}")

    def draw_one(self, shape):
        centers = [tuple(int(ds * np.random.uniform(r[0], r[1])) for ds, r in zip(shape, self.region_range))
                   for _ in range(self.times)]
        sizes = [tuple(int(np.random.uniform(rs[0], rs[1]) * ds) for rs, ds in zip(self.region_size, shape))
                 for _ in range(self.times)]
        # np.random.uniform(min, max) per box in the reference: min + (max - min) * random_sample()
        u = [float(np.random.random_sample()) for _ in range(self.times)]
        return {"mask_centers": centers, "mask_sizes": sizes, "u": u}

    def _tables(self, params, shape, device):
        boxes, u = [], []
        for p in params:
            if p is None:
                boxes.append([[0] * 6] * self.times)
                u.append([0.0] * self.times)
                continue
            if len(p["u"]) != self.times or len(p["mask_centers"]) != self.times or len(p["mask_sizes"]) != self.times:
                raise ValueError(f"RandomMaskOut: {self.times} boxes per sample expected")
            boxes.append(mask_boxes(p["mask_centers"], p["mask_sizes"], shape))
            u.append([float(v) for v in p["u"]])
        return _dev(boxes, torch.int32, device), _dev(u, torch.float64, device)

    def _launch(self, x, tables, flags, out=None, minmax=None):
        minmax = sample_minmax(x, flags) if minmax is None else minmax
        return _mask_out(x, minmax, tables[0], tables[1], flags, out)


class RandomFlip(_Augmentation):
    """np.flip along one spatial axis drawn from (-1, ..., -spatial_dim), the same axis for every '#' entry of a sample."""
    intensity = False

    def __init__(self, spatial_dim):
        self.spatial_dim = spatial_dim
        if spatial_dim not in (1, 2, 3):
            raise NotImplementedError("RandomFlip: supported: spatial_dim 1..3")

    def draw_one(self, shape):
        return {"flip_axis": random.sample([-n for n in range(1, self.spatial_dim + 1)], 1)[0]}

    def _table_one(self, p, shape):
        return flip_table(p["flip_axis"])

    def _tables(self, params, shape, device):
        perm, flip = [], []
        for p in params:
            pf = ((0, 1, 2), (0, 0, 0)) if p is None else self._table_one(p, shape)
            perm.append(list(pf[0]))
            flip.append(list(pf[1]))
        return _dev(perm, torch.int32, device), _dev(flip, torch.int32, device)

    def _launch(self, x, tables, flags, out=None):
        return _permute_flip(x, tables[0], tables[1], flags, out)


class RandomRotate90(RandomFlip):
    """np.rot90 by 0..3 quarter turns in one of the three spatial planes; an odd count needs equal extents in that plane
    (ValueError otherwise: the sample's shape would change)."""

    def __init__(self, spatial_dim):
        self.spatial_dim = spatial_dim
        if spatial_dim not in (2, 3):
            raise NotImplementedError("RandomRotate90: supported: spatial_dim 2 or 3")

    def draw_one(self, shape):
        rotate_times = random.sample(range(4), 1)[0]
        all_combs = list(itertools.combinations([-n for n in range(1, self.spatial_dim + 1)], 2))
        rotate_axis = tuple(random.sample(list(all_combs), 1)[0])
        return {"rotate_axis": rotate_axis, "rotate_times": rotate_times}

    def _table_one(self, p, shape):
        return rotate_table(p["rotate_axis"], p["rotate_times"], shape)


class GaussianAddictive(_Augmentation):
    """Additive Gaussian noise on the sample rescaled to [0, 1]: ((x - min) / (range + 1e-7) + N(0, s)) clamped to [0, 1] and
    rescaled back, s = one np.random.uniform(sigma[0], sigma[1]) draw per sample.

    Deviation from the reference: its `np.random.normal(size=data.shape)` is replaced by a generator inside the kernel
    (Philox4x32-10 keyed by a per-sample seed and the element index, then Box-Muller).  That consumes ONE host draw
    (np.random.randint for the seed) instead of one per voxel, so `numpy.random` draws made after a GaussianAddictive differ
    from the reference's, and the noise values are not numpy's.  A parameter dict may carry "noise" (a float64 device tensor of
    the sample's shape) to run the reference's arithmetic on given noise instead.  Only channel_dim 0 / None (the whole sample
    as one array) is supported."""
    pointwise = uses_minmax = True

    def __init__(self, sigma, channel_dim=0):
        self.sigma = sigma
        self.channel_dim = channel_dim
        self.epsilon = 1e-7
        if channel_dim:
            raise NotImplementedError("GaussianAddictive: per-channel noise (channel_dim != 0 / None) is not supported")

    def draw_one(self, shape):
        sigma = np.random.uniform(self.sigma[0], self.sigma[1])
        seed = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64))
        return {"sigma": sigma, "seed": seed}

    def _tables(self, params, shape, device):
        sigma = _dev([0.0 if p is None else float(p["sigma"]) for p in params], torch.float32, device)
        seeds = _dev([0 if p is None else int(p["seed"]) for p in params], torch.int64, device)
        given = [p is not None and p.get("noise") is not None for p in params]
        noise = None
        if any(given):
            if not all(g or p is None for g, p in zip(given, params)):
                raise ValueError("GaussianAddictive: explicit noise for every active sample of the batch, or for none")
            n_el = int(np.prod(shape))
            noise = torch.zeros((len(params), n_el), dtype=torch.float64, device=device)
            for i, p in enumerate(params):
                if p is not None:
                    noise[i] = p["noise"].to(device=device, dtype=torch.float64).reshape(-1)
        return sigma, seeds, noise

    def _launch(self, x, tables, flags, out=None, minmax=None):
        minmax = sample_minmax(x, flags) if minmax is None else minmax
        return _noise(x, minmax, tables[0], tables[1], flags, tables[2], out)


class _RangeMap(_Augmentation):
    """A point-wise map of the sample rescaled to [0, 1] by its own {min, max} and back, every step in fp32 as numpy computes
    it.  These classes test `not channel_dim`: 0 and None both mean the whole chunk as one array, anything else makes the
    reference work slice by slice along that axis with draws per slice, which is not built."""
    pointwise = uses_minmax = True
    mode = None

    def _check_channel_dim(self):
        if self.channel_dim:
            raise NotImplementedError(f"{type(self).__name__}: channel_dim={self.channel_dim!r} (per-slice transforms along "
                                      f"that axis) is not supported; supported: channel_dim 0 or None (the whole chunk)")

    def _row(self, p):   # pragma: no cover - overridden
        raise NotImplementedError

    def _tables(self, params, shape, device):
        return _dev([[0.0, 0.0] if p is None else self._row(p) for p in params], torch.float32, device)

    def _launch(self, x, tables, flags, out=None, minmax=None):
        minmax = sample_minmax(x, flags) if minmax is None else minmax
        return _intensity_map(x, self.mode, minmax, None, tables, False, flags, 1, out)


class IntensityInverse(_RangeMap):
    """(1 - rescaled), shifted so that its minimum is 0, rescaled back: max <-> min.  Draws nothing."""
    mode = MAP_INVERSE

    def __init__(self, channel_dim=0):
        self.channel_dim = channel_dim
        self.epsilon = 1e-7
        self._check_channel_dim()

    def draw_one(self, shape):
        return {}

    def _tables(self, params, shape, device):
        return None


class GammaTransform(_RangeMap):
    """rescaled ** factor, factor = one np.random.uniform(gamma_range) draw per sample."""
    mode = MAP_GAMMA

    def __init__(self, gamma_range=(0.5, 2), channel_dim=0):
        self.gamma_range = gamma_range
        self.epsilon = 1e-7
        self.channel_dim = channel_dim
        self._check_channel_dim()

    def draw_one(self, shape):
        return {"factor": np.random.uniform(self.gamma_range[0], self.gamma_range[1])}

    def _row(self, p):
        return [float(p["factor"]), 0.0]


class ContrastStretchingTransform(_RangeMap):
    """1 / (1 + (mp / (rescaled + 1e-7)) ** factor): two np.random.uniform draws per sample, factor (gamma_range) then mp
    (middle_point)."""
    mode = MAP_STRETCH

    def __init__(self, gamma_range=(0.5, 2), middle_point=(0.3, 0.7), channel_dim=0):
        self.gamma_range = gamma_range
        self.middle_point = middle_point
        self.epsilon = 1e-7
        self.channel_dim = channel_dim
        self._check_channel_dim()

    def draw_one(self, shape):
        factor = np.random.uniform(self.gamma_range[0], self.gamma_range[1])
        mp = np.random.uniform(self.middle_point[0], self.middle_point[1])
        return {"factor": factor, "mp": mp}

    def _row(self, p):
        return [float(p["factor"]), float(p["mp"])]


class ContrastJitter(_Augmentation):
    """(x - mean) * factor + mean, clamped to the data's own [min, max] when if_keep_range.

    Unlike the other intensity transforms the reference tests `channel_dim is None` here, so its DEFAULT channel_dim=0 jitters
    every z-slice of a [D, H, W] chunk on its own: mean, min, max and one np.random.uniform(jitter_range) draw per slice, D
    draws per sample in slice order.  Only channel_dim=None treats the chunk as one array (one draw).  Both are kept as they
    are; "factor" is the list of the sample's D factors (of its one factor for channel_dim=None).

    The mean is an fp64 sum rounded to fp32; numpy adds float32 pairwise, so the two means can differ in the last bit."""
    pointwise = True      # the slice statistics are its own: the driver's per-sample {min, max} do not serve them

    def __init__(self, jitter_range=(0.75, 1.25), if_keep_range=True, channel_dim=0):
        self.jitter_range = jitter_range
        self.if_keep_range = if_keep_range
        self.channel_dim = channel_dim
        if channel_dim not in (None, 0):
            raise NotImplementedError(f"ContrastJitter: channel_dim={channel_dim!r} is not supported; supported: channel_dim 0 "
                                      f"(every z-slice on its own) or None (the whole chunk)")

    def _rows(self, shape):
        return 1 if self.channel_dim is None else int(shape[0])

    def draw_one(self, shape):
        return {"factor": [np.random.uniform(self.jitter_range[0], self.jitter_range[1]) for _ in range(self._rows(shape))]}

    def _tables(self, params, shape, device):
        rows, table = self._rows(shape), []
        for p in params:
            factors = [0.0] * rows if p is None else [float(v) for v in p["factor"]]
            if len(factors) != rows:
                raise ValueError(f"ContrastJitter: {rows} factors per sample expected (channel_dim={self.channel_dim!r}), "
                                 f"got {len(factors)}")
            table += [[v, 0.0] for v in factors]
        return _dev(table, torch.float32, device), rows

    def _launch(self, x, tables, flags, out=None):
        par, rows = tables
        row_flags = flags if rows == 1 else flags.repeat_interleave(rows)
        minmax = row_minmax(x, rows, row_flags) if self.if_keep_range else None
        return _intensity_map(x, MAP_JITTER, minmax, row_mean(x, rows, row_flags), par, self.if_keep_range, row_flags, rows, out)


class MinimalIntensityProjection(_Augmentation):
    """A causal slab projection: voxel i along axis `angle` becomes the minimum of voxels max(0, i - slab_thickness) .. i, that
    is slab_thickness + 1 voxels.  Two np.random.randint draws per sample: the thickness from `slab_thickness`, then the axis
    from `angle` (0 = z, 1 = y, 2 = x).  The reference stores both draws in a copy of `meta`; `meta` passes through here."""
    is_max = False

    def __init__(self, slab_thickness=(3, 10), angle=(0, 3)):
        self.slab_thickness = slab_thickness
        self.angle = angle
        self.epsilon = 1e-7

    def draw_one(self, shape):
        slab_thickness = np.random.randint(self.slab_thickness[0], self.slab_thickness[1])
        angle = np.random.randint(self.angle[0], self.angle[1])
        return {"slab_thickness": slab_thickness, "angle": angle}

    def _tables(self, params, shape, device):
        name, thickness, axis = type(self).__name__, [], []
        for p in params:
            t, a = (0, 0) if p is None else (int(p["slab_thickness"]), int(p.get("angle", 0)))
            if not 0 <= t <= MAX_SLAB:
                raise ValueError(f"{name}: slab_thickness {t} outside the supported 0..{MAX_SLAB}")
            if not -3 <= a < 3:
                raise ValueError(f"{name}: angle {a} is no axis of a 3-d sample")
            thickness.append(t)
            axis.append(a % 3)
        return _dev(thickness, torch.int32, device), _dev(axis, torch.int32, device)

    def _launch(self, x, tables, flags, out=None):
        return slab_project(x, tables[0], tables[1], self.is_max, flags, out)


class MaximumIntensityProjection(MinimalIntensityProjection):
    """MinimalIntensityProjection with the maximum.  (The reference stores nothing in `meta` for this one.)"""
    is_max = True


class MinimalIntensityAxialProjection(MinimalIntensityProjection):
    """MinimalIntensityProjection along z, one np.random.randint draw per sample.  The window is slab_thickness + 1 VOXELS, as
    in the reference, whose `axial_thickness = int(slab_thickness / spacing[0])` is computed and never used.

    Deviation from the reference: it reads meta['spacing'] for that unused value and stores it as 'axial_thickness' in the
    caller's own meta; this class neither reads nor writes `meta`."""

    def __init__(self, slab_thickness=(3, 10)):
        self.slab_thickness = slab_thickness
        self.epsilon = 1e-7

    def draw_one(self, shape):
        return {"slab_thickness": np.random.randint(self.slab_thickness[0], self.slab_thickness[1])}


class DiskMaskOut(_Augmentation):
    """Every z-slice of every '#' entry (fp32 and uint8) times the disk of centre (H // 2, W // 2) and radius min(H, W) // 2,
    rim included; zero outside.  Draws nothing.  Only select_axis=-3 (the slices along z) and spatial_dim=3 are supported."""
    intensity = False
    pointwise = True

    def __init__(self, select_axis=-3, spatial_dim=3):
        self.spatial_dim = spatial_dim
        self.select_axis = select_axis
        if spatial_dim != 3 or select_axis != -3:
            raise NotImplementedError(f"DiskMaskOut: select_axis={select_axis!r}, spatial_dim={spatial_dim!r} is not supported; "
                                      f"supported: select_axis -3 with spatial_dim 3 (a disk in every z-slice)")

    def draw_one(self, shape):
        return {}

    def _tables(self, params, shape, device):
        whole = [0, shape[0], 0, shape[1], 0, shape[2]]
        return (_dev([whole] * len(params), torch.int32, device), _dev([disk_table(shape)] * len(params), torch.int32, device))

    def _launch(self, x, tables, flags, out=None):
        return keep_region(x, tables[0], tables[1], flags, out)


class RandomCubeMask(DiskMaskOut):
    """Every '#' entry kept inside one box per sample and zeroed outside: sizes int(np.random.uniform(ratio, 1) * dim) per axis
    (three draws), then the centre dim // 2 + int(np.random.uniform(-c * shift, c * shift)) per axis (three draws); the box is
    [max(0, c - s // 2), min(c + (s - s // 2), dim)).

    Deviation from the reference: its `__call__` raises KeyError('crop_sizes_ratio') after the work is done (it stores a meta
    entry that was never made); this class returns the result."""

    def __init__(self, shift_from_center, crop_sizes_ratio, spatial_dim=3):
        self.shift_from_center = shift_from_center
        self.crop_sizes_ratio = crop_sizes_ratio
        self.spatial_dim = spatial_dim
        assert (len(crop_sizes_ratio) == spatial_dim == len(shift_from_center))
        if spatial_dim != 3:
            raise NotImplementedError("RandomCubeMask: supported: spatial_dim 3")

    def draw_one(self, shape):
        crop_sizes_ratio = tuple([np.random.uniform(ratio, 1.0) for ratio in self.crop_sizes_ratio])
        crop_sizes = tuple([int(cs * ds) for cs, ds in zip(crop_sizes_ratio, shape)])
        center = np.asarray(shape) // 2
        offset = tuple([int(np.random.uniform(-c * sh, c * sh)) for c, sh in zip(center, self.shift_from_center)])
        shifted_center = tuple([int(c + offs) for c, offs in zip(center, offset)])
        return {"shifted_center": shifted_center, "crop_sizes": crop_sizes}

    def _tables(self, params, shape, device):
        boxes = [[0] * 6 if p is None else cube_box(p["shifted_center"], p["crop_sizes"], shape) for p in params]
        return _dev(boxes, torch.int32, device), _dev([[0, 0, -1]] * len(params), torch.int32, device)


class RandomMoveAxis(RandomFlip):
    """np.moveaxis(data, a, b) with (a, b) drawn from the pairs of (-1, ..., -spatial_dim), the same pair for every '#' entry of
    a sample.  A move between unequal extents changes the sample's shape: ValueError."""

    def __init__(self, spatial_dim):
        self.spatial_dim = spatial_dim
        if spatial_dim not in (2, 3):
            raise NotImplementedError("RandomMoveAxis: supported: spatial_dim 2 or 3")

    def draw_one(self, shape):
        all_combs = list(itertools.combinations([-n for n in range(1, self.spatial_dim + 1)], 2))
        return {"sampled_comb": tuple(random.sample(all_combs, 1)[0])}

    def _table_one(self, p, shape):
        return moveaxis_table(p["sampled_comb"], shape)


class RandomRotateInplane90(RandomFlip):
    """np.rot90 by 0..3 quarter turns in the (x, y) plane, axes (-1, -2); an odd count needs H == W (ValueError otherwise)."""

    def __init__(self, spatial_dim):
        self.spatial_dim = spatial_dim
        if spatial_dim not in (2, 3):
            raise NotImplementedError("RandomRotateInplane90: supported: spatial_dim 2 or 3")

    def draw_one(self, shape):
        return {"rotate_times": random.sample(range(4), 1)[0]}

    def _table_one(self, p, shape):
        return rotate_table((-1, -2), p["rotate_times"], shape)


class RandomCrop(_Augmentation):
    """A window of every '#' entry, padded where it leaves the chunk, stretched back to the chunk's size.  Six
    np.random.uniform draws per sample: the window's size int(U(ratio, 1) * dim) per axis, then its centre dim // 2 +
    int(U(-c * shift, c * shift)) per axis; `padding` is what np.pad gets ((max(0, s // 2 - cc), max(0, cc + s // 2 - dim))), and
    the window is `crop_window(params, shape)`.  keep_size=True then runs Resample('fixed_size', 1, shape) on the crop: linear for
    the image, nearest neighbour for every key with 'reference' or 'weight_map' in its name, on the grid of `ChunkLoader`
    (`preprocess.resample_plan`; output voxel o reads crop index o * crop / dim, and is 0 from crop - 0.5 on: an axis cropped to
    less than half ends in zeros, as ITK leaves it).  A parameter dict may carry "spacing" (default (1.0, 1.0, 1.0)), the
    sample's meta['spacing'], from which the steps are formed as the reference forms them.  Padding modes 'minimum', 'constant'
    and 'edge'.  `meta` passes through: the reference's entries (the draws, 'size', 'spacing') are not written."""
    intensity = False

    def __init__(self, shift_from_center, crop_sizes_ratio, spatial_dim=3, padding_mode='minimum', keep_size=True):
        self.shift_from_center = shift_from_center
        self.crop_sizes_ratio = crop_sizes_ratio
        self.spatial_dim = spatial_dim
        self.padding_mode = padding_mode
        self.keep_size = keep_size
        assert (len(crop_sizes_ratio) == spatial_dim == len(shift_from_center))
        if spatial_dim != 3:
            raise NotImplementedError("RandomCrop: supported: spatial_dim 3")
        if padding_mode not in PAD_MODES:
            raise NotImplementedError(f"RandomCrop: padding_mode={padding_mode!r} is not supported; supported: "
                                      f"{', '.join(sorted(PAD_MODES))}")
        if not keep_size:
            raise ValueError("RandomCrop: keep_size=False changes the sample's shape and cannot live in a batch tensor")

    def draw_one(self, shape):
        crop_sizes_ratio = tuple([float(np.random.uniform(ratio, 1.0)) for ratio in self.crop_sizes_ratio])
        crop_sizes = tuple([int(cs * ds) for cs, ds in zip(crop_sizes_ratio, shape)])
        center = np.asarray(shape) // 2
        offset = tuple([int(np.random.uniform(-c * sh, c * sh)) for c, sh in zip(center, self.shift_from_center)])
        shifted_center = tuple([int(c + offs) for c, offs in zip(center, offset)])
        padding = [(int(max(0, si // 2 - cc)), int(max(0, cc + si // 2 - sh)))
                   for sh, si, cc in zip(shape, crop_sizes, shifted_center)]
        return {"crop_sizes_ratio": crop_sizes_ratio, "crop_sizes": crop_sizes, "offset": offset,
                "shifted_center": shifted_center, "padding": padding}

    def _tables(self, params, shape, device):
        from .preprocess import resample_plan
        if shape[2] > MAX_W or shape[1] > MAX_W:
            raise ValueError(f"RandomCrop: rows and columns of up to {MAX_W} voxels, got {tuple(shape)}")
        table = np.zeros(len(params), dtype=CROP_DTYPE)
        pads = []
        for i, p in enumerate(params):
            if p is None:
                table[i] = (0, 0, 0) + tuple(shape) + (0, 0, 1.0, 1.0, 1.0)
                pads.append(False)
                continue
            start, size = crop_window(p, shape)
            if min(size) <= 0:
                raise ValueError(f"RandomCrop: sample {i}: empty crop {size}")
            spacing = np.asarray(p.get("spacing", (1.0, 1.0, 1.0)), dtype=np.float64)
            req, new_size = resample_plan("fixed_size", 1, list(shape), spacing, size)
            step = [float(req[a]) / float(spacing[a]) for a in range(3)]
            if tuple(new_size) != tuple(shape) or not all(np.isfinite(v) and v > 0 for v in step):
                raise ValueError(f"RandomCrop: sample {i}: resampling steps {step}")
            table[i] = start + size + (PAD_MODES[self.padding_mode], 0) + tuple(step)
            pads.append(self.padding_mode == "minimum" and
                        any(st < 0 or st + sz > dim for st, sz, dim in zip(start, size, shape)))
        tab = torch.from_numpy(table.view(np.uint8).copy())
        if torch.device(device).type == "cuda":
            tab = tab.pin_memory().to(device, non_blocking=True)
        return tab, pads

    def _launch(self, x, tables, flags, out=None):     # pragma: no cover - the key decides the interpolation
        raise NotImplementedError("RandomCrop works per key: _launch_key")

    def _launch_key(self, key, x, tables, flags, out=None):
        table, pads = tables
        linear = not ("reference" in key or "weight_map" in key)
        if x.shape[1] != 1:
            raise NotImplementedError(f"RandomCrop: '{key}': single-channel samples only, got shape {tuple(x.shape)}")
        if linear and x.dtype != torch.float32:
            raise NotImplementedError(f"RandomCrop: '{key}' is {x.dtype} and would be resampled linearly; linear interpolation "
                                      f"is built for float32 (nearest neighbour: keys with 'reference' or 'weight_map')")
        ws = None
        if any(pads):
            # SKIP samples of an ensemble launch (flag < 0) take no part: their flag is not TRANSFORM
            ws = pad_min(x, flags * _dev([1 if p else 0 for p in pads], torch.int32, x.device))
        return crop_resample(x, table, flags, linear, ws, out)


class StandarizeChannel(_Augmentation):
    """a = a.astype(float32); a = a - a.mean(); a /= a.std() on every '#...image...' entry: [N, D, H, W] and [N, 1, D, H, W] per
    sample, [N, C, D, H, W] with ch_dim == 0 per (sample, channel) -- the reference's 4-d sample [C, D, H, W] taken along its
    first axis.  Draws nothing.  The mean and the std come from fp64 sums (numpy adds float32 pairwise): results agree with
    the reference to a few fp32 steps, not bit for bit.  A constant sample (std 0) divides by zero, as in the reference."""
    pointwise = True

    def __init__(self, ch_dim):
        self.ch_dim = ch_dim

    def draw_one(self, shape):
        return {}

    def _tables(self, params, shape, device):
        return None

    def apply(self, sample, params):
        out = {}
        for key, value in sample.items():
            if not self._touches(key):
                out[key] = value
                continue
            v, shape = _as_batch(value, key)
            if len(params) != v.shape[0]:
                raise ValueError(f"StandarizeChannel: {len(params)} parameter sets for a batch of {v.shape[0]}")
            C = v.shape[1]
            if C != 1 and self.ch_dim != 0:
                raise NotImplementedError(f"StandarizeChannel: ch_dim={self.ch_dim!r} on a multi-channel tensor {shape} is not "
                                          f"supported; supported: ch_dim 0 (per sample and channel)")
            flags = _dev([TRANSFORM if p is not None else PASS for p in params for _ in range(C)], torch.int32, v.device)
            out[key] = self._launch(v, None, flags, rows=C).view(shape)
        return out

    def _launch(self, x, tables, flags, out=None, rows=1):
        return _intensity_map(x, MAP_STANDARDIZE, None, None, row_mean_std(x, rows, flags), False, flags, rows, out)


class _SplineTransform(_Augmentation):
    """Shared by the two spline-resampled transforms: every '#' entry is resampled at a per-sample affine map of the output
    index, keys containing "image" with cubic B-splines (scipy's order 3: fp64 coefficients from a prefilter, then 64 taps per
    voxel, 16 in a rotation plane), every other key at the nearest voxel (order 0; fp32 or uint8, dtype kept).  mode="constant":
    a voxel whose source lies outside [0, n - 1] in any axis gets the entry's own per-sample minimum."""
    intensity = False

    def _record(self, p, shape):   # pragma: no cover - overridden
        """(3 x 3 matrix, offset, fixed axis or -1, prefilter axes mask) of one sample."""
        raise NotImplementedError

    def _tables(self, params, shape, device):
        table = np.zeros(len(params), dtype=SPLINE_DTYPE)
        axes = []
        for i, p in enumerate(params):
            m, off, fixed, mask = (np.eye(3), np.zeros(3), -1, 0) if p is None else self._record(p, shape)
            if not (np.all(np.isfinite(m)) and np.all(np.isfinite(off))):
                raise ValueError(f"{type(self).__name__}: sample {i}: the transform is not finite")
            table[i] = (np.asarray(m, dtype=np.float64).reshape(9), np.asarray(off, dtype=np.float64), fixed, 0)
            axes.append(mask)
        tab = torch.from_numpy(table.view(np.uint8).copy())
        if torch.device(device).type == "cuda":
            tab = tab.pin_memory().to(device, non_blocking=True)
        return tab, _dev(axes, torch.int32, device)

    def _launch(self, x, tables, flags, out=None):     # pragma: no cover - the key decides the interpolation
        raise NotImplementedError(f"{type(self).__name__} works per key: _launch_key")

    def _launch_key(self, key, x, tables, flags, out=None):
        table, axes = tables
        order = 3 if "image" in key else 0
        if x.shape[1] != 1:
            raise NotImplementedError(f"{type(self).__name__}: '{key}': single-channel samples only, got shape {tuple(x.shape)}")
        if order == 3 and x.dtype != torch.float32:
            raise NotImplementedError(f"{type(self).__name__}: '{key}' is {x.dtype} and would be resampled with cubic splines; "
                                      f"order 3 is built for float32 (nearest neighbour: keys without 'image')")
        minmax = sample_min_table(x, flags)
        coef = spline_prefilter(x, axes, flags) if order == 3 else None
        return spline_resample(x, table, minmax, flags, order, coef, out)


class RandomAffineTransform3D(_SplineTransform):
    """scipy.ndimage.affine_transform of every '#' entry with one scale per axis and three rotation angles per sample: six
    np.random.uniform draws, the scales U(1 - s, 1 + s) first, then the angles U(-r, r); the matrix is `affine_matrix`, built
    and inverted on the host in fp64.  `meta` passes through (the reference stores the draws and 'size' there)."""

    def __init__(self, spatial_dim, rotations=(0.2 * math.pi, 0.2 * math.pi, 0.2 * math.pi), scales=(0.05, 0.05, 0.05)):
        self.spatial_dim = spatial_dim
        self.rotations = rotations
        self.scales = scales
        if spatial_dim != 3:
            raise NotImplementedError("RandomAffineTransform3D: supported: spatial_dim 3")

    def draw_one(self, shape):
        draw = np.random.uniform
        return {"scales": [float(draw(1.0 - s, 1.0 + s)) for s in self.scales],               # the scales first,
                "rotate_angles": [float(draw(-r, r)) for r in self.rotations]}                # then the angles

    def _record(self, p, shape):
        m, off = affine_matrix(p["scales"], p["rotate_angles"], shape)
        return m, off, -1, 7


class RandomRotate(_SplineTransform):
    """scipy.ndimage.rotate(reshape=False) of every '#' entry: one random.randint(*rotate_range) angle in degrees, then the
    plane as the first of two planes sampled from ROTATE_PLANES (Python's `random`, in that order).  scipy turns a 3-d array
    plane by plane with a 2-d transform, so the spline prefilter runs along the two plane axes only; the fill value is the
    minimum of the whole sample.  `meta` passes through."""

    def __init__(self, spatial_dim, rotate_range):
        self.spatial_dim = spatial_dim
        self.rotate_range = rotate_range
        if spatial_dim != 3:
            raise NotImplementedError("RandomRotate: supported: spatial_dim 3")

    def draw_one(self, shape):
        angle = random.randint(*self.rotate_range)
        plane = random.sample(ROTATE_PLANES, 2)[0]       # two are sampled and the first is used: the stream moves as it does there
        return {"rotate_axis": tuple(plane), "rotate_angle": angle}

    def _record(self, p, shape):
        m, off, fixed = rotate_matrix(p["rotate_angle"], p["rotate_axis"], shape)
        return m, off, fixed, 7 & ~(1 << fixed)


# -------------------------------------------------------------------------------------------------------------- ensemble
class EnsembleScanAugmentation:
    """The reference's `_T` (job_runner.py:556-579) on a batch: per sample one of the 120 orders of the pool
    (`random.sample`), each element kept iff `np.random.randint(0, 10) < 10 * aug_ratio`, then that chain applied.  All draws of
    a sample (order, keep decisions, then each kept element's parameters in chain order) are made before the next sample's, as
    the reference's chunk-by-chunk loop makes them.

    Execution: for each chain position and each pool element, one launch over the samples that have that element at that position
    (others are skipped, not copied).  Every sample lives in the input or in one of two work buffers; a launch reads the samples
    of one buffer and writes them to another, the two point-wise transforms work in place once a sample has left the input.
    What is not in the result buffer at the end is copied there.  The result equals applying each sample's chain to that sample
    alone.  `aug_ratio` 0 (the shipped settings' value) returns the sample dict's tensors untouched and launches nothing."""

    def __init__(self, aug_ratio, pool=None):
        self.aug_ratio = aug_ratio
        self.transform_pool = pool if pool is not None else [
            GaussianBlur((0.3, 0.5), "random"),
            RandomMaskOut(region_range=((0.2, 0.8), (0.2, 0.8), (0.2, 0.8)),
                          region_size=((0.01, 0.05), (0.01, 0.05), (0.01, 0.05))),
            RandomFlip(3),
            RandomRotate90(3),
            GaussianAddictive((0.01, 0.02), None),
        ]

    def aug_sampling(self, aug_list):
        return [x for x in aug_list if np.random.randint(0, 10) < (10 * self.aug_ratio)]

    def draw(self, n, shape):
        """Per sample a list of (pool element, parameters), in application order."""
        chains = []
        for _ in range(n):
            all_p = list(itertools.permutations(self.transform_pool, len(self.transform_pool)))
            p = list(random.sample(all_p, 1)[0])
            p = self.aug_sampling(p)
            chains.append([(t, t.draw_one(tuple(shape))) for t in p])
        return chains

    @staticmethod
    def chain_names(chains):
        return [[type(t).__name__ for t, _ in chain] for chain in chains]

    def apply(self, sample, chains):
        if not any(chains):
            return dict(sample)
        out = {}
        for key, value in sample.items():
            out[key] = self._run(key, value, chains) if "#" in key else value
        return out

    def _run(self, key, value, chains):
        steps = [[(t, p) for t, p in chain if t._touches(key)] for chain in chains]
        if not any(steps):
            return value
        image = "image" in key
        src, shape = (_as_image(value, key) if image and any(t.intensity for c in steps for t, _ in c)
                      else _as_batch(value, key, (torch.float32, torch.uint8)))
        N, device, spatial = src.shape[0], src.device, tuple(src.shape[2:])
        if len(chains) != N:
            raise ValueError(f"EnsembleScanAugmentation: {len(chains)} chains for a batch of {N}")
        bufs = [src, torch.empty_like(src), None]     # 0: the input (never written), 1: the result, 2: second work buffer
        where = [0] * N
        minmax = torch.empty((N, 2), dtype=torch.float32, device=device)
        for pos in range(max(len(c) for c in steps)):
            for t in self.transform_pool:
                members = [i for i in range(N) if pos < len(steps[i]) and steps[i][pos][0] is t]
                if not members:
                    continue
                params = [steps[i][pos][1] if i in members else None for i in range(N)]
                tables = t._tables(params, spatial, device)
                inplace = t.pointwise
                groups = {s: [i for i in members if where[i] == s] for s in sorted({where[i] for i in members})}
                for s, group in groups.items():
                    d = s if (inplace and s != 0) else (2 if s == 1 else 1)
                    if bufs[d] is None:
                        bufs[d] = torch.empty_like(src)
                    flags = _dev([TRANSFORM if i in group else SKIP for i in range(N)], torch.int32, device)
                    if t.uses_minmax:
                        sample_minmax(bufs[s], flags, out=minmax)
                        t._launch_key(key, bufs[s], tables, flags, out=bufs[d], minmax=minmax)
                    else:
                        t._launch_key(key, bufs[s], tables, flags, out=bufs[d])
                    for i in group:
                        where[i] = d
        ident = (_dev([[0, 1, 2]] * N, torch.int32, device), _dev([[0, 0, 0]] * N, torch.int32, device))
        for s in (0, 2):      # gather what did not end in the result buffer
            group = [i for i in range(N) if where[i] == s]
            if group:
                flags = _dev([TRANSFORM if where[i] == s else SKIP for i in range(N)], torch.int32, device)
                _permute_flip(bufs[s], ident[0], ident[1], flags, out=bufs[1])
        return bufs[1].view(shape)

    def __call__(self, sample):
        first = _first_tensor(sample)
        chains = self.draw(first.shape[0], tuple(first.shape[-3:]))     # (the reference draws at aug_ratio 0 as well)
        return self.apply(sample, chains) if any(chains) else sample
