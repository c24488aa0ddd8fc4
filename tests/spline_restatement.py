"""Restatement in numpy of the order-3 and order-0 paths of scipy.ndimage.affine_transform(mode="constant") and of
scipy.ndimage.rotate(reshape=False) as the reference's RandomAffineTransform3D and RandomRotate call them
(dram/data_transforms.py:995-1102).  tests/test_augment_spline_cpu.py pins it to the reference's own results
(tests/golden/augment_spline.npz); tests/test_gpu_augment_spline.py then leans on its fp64 source coordinates to find the
knife-edge voxels.  The device kernels (csrc/spline.hip) follow the same arithmetic step by step.

  prefilter      per axis in turn (axis 0 first) and per line: times (1 - z)(1 - 1/z), z = sqrt(3) - 2; the causal recursion
                 c[i] += z c[i-1] started from the exact mirror sum over the whole line; the anticausal recursion
                 c[i] = z (c[i+1] - c[i]) started from c[n-1] = z / (z^2 - 1) (c[n-1] + z c[n-2]).  fp32 in, fp64 out.  A line
                 of one element is left as it is.
  coordinates    x_h = off_h + sum_l M[h][l] idx_l, added left to right in fp64; outside [0, n_h - 1] in any axis: cval
  order 3        start floor(x) - 1, the four cubic B-spline weights at t = x - floor(x), coefficient indices mirrored with
                 period 2n - 2 (n == 1: index 0), the 64 taps (16 in a rotate plane) added in fp64, z slowest, then cast
  order 0        index floor(x + 0.5), the entry's dtype kept
"""
import math

import numpy as np

POLE = math.sqrt(3.0) - 2.0


def prefilter_line(c):
    """One line (last axis of `c`, fp64, changed in place) through the cubic B-spline prefilter with mirror boundaries."""
    n = c.shape[-1]
    if n < 2:
        return c
    z = POLE
    c *= (1.0 - z) * (1.0 - 1.0 / z)
    z_n_1 = z ** (n - 1)
    c0 = c[..., 0] + z_n_1 * c[..., n - 1]
    z_i = z
    for i in range(1, n - 1):
        c0 = c0 + z_i * (c[..., i] + z_n_1 * c[..., n - 1 - i])
        z_i *= z
    c[..., 0] = c0 / (1.0 - z_n_1 * z_n_1)
    for i in range(1, n):
        c[..., i] = c[..., i] + z * c[..., i - 1]
    c[..., n - 1] = (z * c[..., n - 2] + c[..., n - 1]) * z / (z * z - 1.0)
    for i in range(n - 2, -1, -1):
        c[..., i] = z * (c[..., i + 1] - c[..., i])
    return c


def prefilter(a, axes=None):
    """fp64 spline coefficients of `a`, filtered along `axes` (default: all), axis 0 first."""
    c = np.array(a, dtype=np.float64)
    for ax in sorted(range(c.ndim) if axes is None else axes):
        moved = np.moveaxis(c, ax, -1)      # a view: the lines are filtered in place
        prefilter_line(moved)
    return c


def source_coordinates(matrix, offset, shape):
    """fp64 source coordinate of every output voxel: [ndim, *shape]."""
    idx = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    out = []
    for h in range(len(shape)):
        x = np.full(shape, float(offset[h]), dtype=np.float64)
        for l in range(len(shape)):
            x = x + float(matrix[h][l]) * idx[l]
        out.append(x)
    return np.stack(out)


def inside(coords, shape):
    ok = np.ones(coords.shape[1:], dtype=bool)
    for h, n in enumerate(shape):
        ok &= ~((coords[h] < 0) | (coords[h] > n - 1))
    return ok


def mirror(i, n):
    if n == 1:
        return np.zeros_like(i)
    p = 2 * n - 2
    m = np.mod(i, p)
    return np.where(m < n, m, p - m)


def cubic_weights(t):
    """The four weights scipy forms for order 3, at the taps floor(x) - 1 .. floor(x) + 2."""
    y, z = t, 1.0 - t
    w1 = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0
    w2 = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0
    w0 = z * z * z / 6.0
    w3 = 1.0 - w0 - w1 - w2
    return [w0, w1, w2, w3]


def affine_transform(a, matrix, offset, order, cval):
    """scipy.ndimage.affine_transform(a, matrix, offset=offset, output_shape=a.shape, mode="constant", order=order, cval=cval)
    for order 3 (fp32 arrays) and order 0 (any dtype), in any number of dimensions."""
    shape = a.shape
    coords = source_coordinates(matrix, offset, shape)
    ok = inside(coords, shape)
    nd = a.ndim
    if order == 0:
        idx = tuple(np.clip(np.floor(coords[h] + 0.5).astype(np.int64), 0, shape[h] - 1) for h in range(nd))
        return np.where(ok, a[idx], np.asarray(cval, dtype=a.dtype)).astype(a.dtype)
    assert order == 3
    coef = prefilter(a)
    fl = np.floor(coords)
    start = fl.astype(np.int64) - 1
    w = [cubic_weights(coords[h] - fl[h]) for h in range(nd)]
    acc = np.zeros(shape, dtype=np.float64)
    for taps in np.ndindex(*([4] * nd)):
        term = coef[tuple(mirror(start[h] + taps[h], shape[h]) for h in range(nd))]
        for h in range(nd):
            term = term * w[h][taps[h]]
        acc = acc + term
    return np.where(ok, acc, float(cval)).astype(a.dtype)


def rotate_plane_matrix(angle, axes, shape):
    """scipy.ndimage.rotate(reshape=False): the sorted plane axes (non-negative), the 2 x 2 matrix and the offset."""
    from scipy import special
    nd = len(shape)
    ax = sorted(a % nd for a in axes)
    c, s = special.cosdg(angle), special.sindg(angle)
    rot = np.array([[c, s], [-s, c]])
    plane = np.asarray(shape, dtype=np.float64)[ax]
    out_center = rot @ ((plane - 1) / 2)
    in_center = (plane - 1) / 2
    return ax, rot, in_center - out_center


def rotate(a, angle, axes, order):
    """scipy.ndimage.rotate(a, angle, reshape=False, axes=axes, order=order, mode="constant", cval=a.min()) on a 3-d array: a
    2-d transform of every plane spanned by `axes`, the fill value taken from the whole array."""
    ax, rot, off = rotate_plane_matrix(angle, axes, a.shape)
    other = [k for k in range(3) if k not in ax][0]
    cval = a.min()
    out = np.empty_like(a)
    for i in range(a.shape[other]):
        sl = [slice(None)] * 3
        sl[other] = i
        out[tuple(sl)] = affine_transform(a[tuple(sl)], rot, off, order, cval)
    return out


def embed_plane(ax, rot, off):
    """The 2-d plane transform as a 3 x 3 matrix and offset that leave the third axis alone."""
    M, o = np.eye(3), np.zeros(3)
    for i, a in enumerate(ax):
        o[a] = off[i]
        M[a, a] = 0.0
        for j, b in enumerate(ax):
            M[a, b] = rot[i, j]
    return M, o
