"""Lesion shape report on the device: what a lesion looks like -- surface area, compactness, Euler number (cavities and tunnels),
principal axes -- without a host-side `regionprops` pass over the label volume.

    t = label_shape(labels, n)                                          # the two exact integer tables per label
    rows = lesion_shape(labels, n, spacing)                             # one dict per label
    rep = lesion_report(mask, lobe, spacing, shape=True)                # lesions.lesion_report with a `shape` entry

Kernel: csrc/shape.hip, one pass over the label volume for the histogram of 2x2x2 neighbourhood configurations (the route to the
Minkowski functionals of Ohser and Muecklich, as in Legland's imMinkowski / MorphoLibJ) and the moments up to second order
(include/dram_hip.h has the definition).  Only O(labels) integers travel to the host, where everything else is arithmetic on
them: voxel count, exposed faces, crossing counts and the Euler number are exact; `area_mm2` is the 13-direction Crofton
ESTIMATE of the surface area, good to a fraction of a percent on round bodies and biased low on axis-aligned flat faces (74.9
for a 3 x 4 x 5 box of area 94, where `area_faces_mm2`, the staircase area, is exact).

Adjacency: the Euler number is that of the union of closed voxels, which is 26-adjacency.  Index 0 is the low-index end of each
axis; nothing here has been validated clinically.
"""
import math

import numpy as np
import torch

from ._lib import call
from .surface import _spacing, _stream, _volume

# The 13 lattice directions (dz, dy, dx), one of each pair +-v: 3 axes, 6 face diagonals, 4 space diagonals.  `crossings` and
# `crofton_weights` use this order.
DIRECTIONS = ((1, 0, 0), (0, 1, 0), (0, 0, 1),
              (1, 1, 0), (1, -1, 0), (1, 0, 1), (1, 0, -1), (0, 1, 1), (0, 1, -1),
              (1, 1, 1), (1, 1, -1), (1, -1, 1), (1, -1, -1))
MOMENT_KEYS = ("count", "z", "y", "x", "zz", "yy", "xx", "zy", "zx", "yx")


def _bit(c, dz, dy, dx):
    return (c >> (dz * 4 + dy * 2 + dx)) & 1


def _crossing_table():
    """table[i][c]: in a cell of configuration c, the instances (p, p + v_i), both ends corners of the cell, whose bits differ; and
    the number of cells that hold one lattice pair of direction i (4, 2 or 1)."""
    table, cells = [], []
    for v in DIRECTIONS:
        inst = [(p, tuple(a + b for a, b in zip(p, v))) for p in np.ndindex(2, 2, 2) if all(0 <= a + b <= 1 for a, b in zip(p, v))]
        table.append([sum(_bit(c, *p) != _bit(c, *q) for p, q in inst) for c in range(256)])
        cells.append(len(inst))
    return table, cells


def _euler_table():
    """1 - e(c) + f(c) - bit7(c): of the lattice vertex in the middle of a cell, the three edges and three faces that leave it
    towards +z, +y, +x and the voxel beyond them, those that belong to the union of the closed voxels."""
    out = []
    for c in range(256):
        corners = [p for p in np.ndindex(2, 2, 2) if _bit(c, *p)]
        e = sum(any(p[a] == 1 for p in corners) for a in range(3))
        f = sum(any(p[a] == 1 and p[b] == 1 for p in corners) for a, b in ((0, 1), (0, 2), (1, 2)))
        out.append((1 - e + f - _bit(c, 1, 1, 1)) if c else 0)
    return out


_CROSSING, _CROSSING_CELLS = _crossing_table()
_EULER = _euler_table()
_POPCOUNT = [bin(c).count("1") for c in range(256)]


def _row(cfg_row):
    row = [int(v) for v in np.asarray(cfg_row).reshape(-1)]
    if len(row) != 256:
        raise ValueError("a configuration row has 256 entries")
    return row


def crossings(cfg_row):
    """Per direction of `DIRECTIONS`, the number of lattice pairs (p, p + v) with exactly one end in the label, as 13 Python
    integers.  A pair of an axis direction lies in 4 cells, of a face diagonal in 2, of a space diagonal in 1, so the count is the
    sum over cells and instances of "the two bits differ" divided by that number; the division is exact."""
    row = _row(cfg_row)
    out = []
    for t, cells in zip(_CROSSING, _CROSSING_CELLS):
        total = sum(n * w for n, w in zip(row, t) if n)
        assert total % cells == 0, "a configuration table that no label volume produces"
        out.append(total // cells)
    return out


def euler_number(cfg_row):
    """The Euler characteristic of the label as a union of closed voxels (26-adjacency), a Python integer: components - tunnels +
    cavities, so 1 - tunnels + cavities for one connected lesion."""
    return sum(n * w for n, w in zip(_row(cfg_row), _EULER) if n)


def crofton_weights(spacing):
    """The 13 direction weights of `DIRECTIONS` under the voxel spacing (z, y, x), summing to 1: the areas of the spherical Voronoi
    cells of the 26 unit vectors +-(v * spacing) / |v * spacing|, over 4 pi, each pair +-v merged.  Isotropic spacing gives
    0.0915558, 0.0739613 and 0.0703913 for the three classes (Ohser and Muecklich)."""
    from scipy.spatial import SphericalVoronoi
    sp = np.asarray(_spacing(spacing, "crofton_weights"))
    v = np.asarray(DIRECTIONS, dtype=np.float64) * sp[None, :]
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    areas = SphericalVoronoi(np.concatenate((v, -v))).calculate_areas()
    w = (areas[:13] + areas[13:]) / (4.0 * math.pi)
    return w / w.sum()


def _empty_tables(n):
    return {"cfg": np.zeros((n, 256), np.int64), "mom": np.zeros((n, 10), np.int64)}


def label_shape(labels, n):
    """The exact integer tables of dram_label_shape per label k = 1..n of a uint8 or int32 [D,H,W] label volume as host numpy arrays
    from one device buffer and one read-back: {"cfg": int64 [n,256], the cells of the zero-padded volume per 2x2x2 configuration
    (bit dz*4 + dy*2 + dx), "mom": int64 [n,10], `MOMENT_KEYS` = count and the sums of z, y, x, z^2, y^2, x^2, zy, zx, yx}."""
    n = int(n)
    labels = _volume(labels, "label_shape")
    if labels.dtype not in (torch.uint8, torch.int32):
        raise ValueError("label_shape: labels must be uint8 or int32")
    if n <= 0 or labels.numel() == 0:
        return _empty_tables(max(n, 0))
    if not labels.is_cuda:
        labels = labels.to(torch.device("cuda", torch.cuda.current_device()))
    labels = labels.contiguous()
    buf = torch.empty(n * 266, dtype=torch.int64, device=labels.device)
    with torch.cuda.device(labels.device):
        call("dram_label_shape", labels.data_ptr(), 0 if labels.dtype == torch.uint8 else 1, n, buf[:n * 256].data_ptr(),
             buf[n * 256:].data_ptr(), *labels.shape, _stream())
    host = buf.cpu().numpy()
    return {"cfg": host[:n * 256].reshape(n, 256).copy(), "mom": host[n * 256:].reshape(n, 10).copy()}


def _nan_row(voxels, faces, sp):
    nan3 = np.full(3, np.nan)
    return {"voxels": voxels, "volume_mm3": 0.0, "faces": faces, "area_faces_mm2": 0.0, "area_mm2": 0.0, "euler": 0,
            "equivalent_diameter_mm": 0.0, "sphericity": float("nan"), "centroid": nan3.copy(), "centroid_mm": nan3.copy(),
            "covariance_mm2": np.full((3, 3), np.nan), "axes_mm": nan3.copy(), "axis_directions": np.full((3, 3), np.nan),
            "elongation": float("nan"), "flatness": float("nan")}


def rows_from_tables(tables, spacing):
    """One dict per label from the integer tables alone, in fp64 on the host:
        voxels (sum_c popcount(c) * cfg[c] / 8, exact), volume_mm3, faces (the exposed voxel faces per axis z, y, x: the three axis
        crossing counts), area_faces_mm2 (the staircase area, exact), area_mm2 (the 13-direction Crofton estimate
        4 * sum_i w_i * (crossings_i / 2) * V_vox / |v_i * spacing|), euler, equivalent_diameter_mm ((6 V / pi)^(1/3)), sphericity
        (pi^(1/3) (6 V)^(2/3) / area_mm2, not clipped: the estimate may pass 1 for lesions of a few voxels), centroid (z, y, x in
        voxel indices) and centroid_mm, covariance_mm2 ([3,3]; entry (a, b) = s_a s_b (c * sum ab - sum a * sum b) / c^2, the
        bracket in exact integers, plus s_a^2 / 12 on the diagonal for the voxel's own extent), axes_mm (2 sqrt(5 lambda_i),
        descending: the axes of the ellipsoid with the same second moments), axis_directions ([3,3], row i the unit vector
        (z, y, x) of axis i, its largest-magnitude component positive), elongation (sqrt(lambda_2 / lambda_1)) and flatness
        (sqrt(lambda_3 / lambda_1)).
    A label without voxels has NaN wherever a quotient would divide by zero."""
    sp = np.asarray(_spacing(spacing, "rows_from_tables"))
    cfg = np.asarray(tables["cfg"], dtype=np.int64).reshape(-1, 256)
    mom = np.asarray(tables["mom"], dtype=np.int64).reshape(-1, 10)
    if len(cfg) != len(mom):
        raise ValueError("rows_from_tables: cfg and mom must have one row per label each")
    if len(cfg) == 0:
        return []
    v_vox = float(sp[0] * sp[1] * sp[2])
    weights = crofton_weights(sp)
    step = np.linalg.norm(np.asarray(DIRECTIONS, dtype=np.float64) * sp[None, :], axis=1)
    rows = []
    for k in range(len(cfg)):
        row = _row(cfg[k])
        eight = sum(n * w for n, w in zip(row, _POPCOUNT) if n)
        assert eight % 8 == 0, "a configuration table that no label volume produces"
        voxels = eight // 8
        cross = crossings(row)
        faces = tuple(cross[:3])
        if voxels == 0:
            rows.append(_nan_row(voxels, faces, sp))
            continue
        volume = voxels * v_vox
        area_faces = sum(faces[a] * v_vox / sp[a] for a in range(3))
        area = 4.0 * sum(weights[i] * (cross[i] / 2.0) * v_vox / step[i] for i in range(13))
        c, s1 = int(mom[k, 0]), [int(v) for v in mom[k, 1:4]]
        s2 = {(0, 0): int(mom[k, 4]), (1, 1): int(mom[k, 5]), (2, 2): int(mom[k, 6]), (0, 1): int(mom[k, 7]), (0, 2): int(mom[k, 8]),
              (1, 2): int(mom[k, 9])}
        centroid = np.array([s / c for s in s1], dtype=np.float64)
        cov = np.zeros((3, 3), dtype=np.float64)
        for a in range(3):
            for b in range(a, 3):
                bracket = c * s2[(a, b)] - s1[a] * s1[b]
                cov[a, b] = cov[b, a] = sp[a] * sp[b] * (bracket / (c * c)) + (sp[a] * sp[a] / 12.0 if a == b else 0.0)
        lam, vec = np.linalg.eigh(cov)
        lam, vec = lam[::-1], vec[:, ::-1].T                              # descending; row i = direction i
        for i in range(3):
            if vec[i, np.argmax(np.abs(vec[i]))] < 0:
                vec[i] = -vec[i]
        rows.append({"voxels": voxels, "volume_mm3": volume, "faces": faces, "area_faces_mm2": float(area_faces), "area_mm2": float(area),
                     "euler": euler_number(row), "equivalent_diameter_mm": (6.0 * volume / math.pi) ** (1.0 / 3.0),
                     "sphericity": float(math.pi ** (1.0 / 3.0) * (6.0 * volume) ** (2.0 / 3.0) / area), "centroid": centroid,
                     "centroid_mm": centroid * sp, "covariance_mm2": cov, "axes_mm": 2.0 * np.sqrt(5.0 * lam),
                     "axis_directions": np.ascontiguousarray(vec), "elongation": float(math.sqrt(lam[1] / lam[0])),
                     "flatness": float(math.sqrt(lam[2] / lam[0]))})
    return rows


def lesion_shape(labels, n, spacing):
    """`rows_from_tables(label_shape(labels, n), spacing)`: the shape report of the labels 1..n of a uint8 or int32 [D,H,W] label
    volume under the voxel spacing (z, y, x) in mm, one dict per label.  n == 0: an empty list without a launch."""
    _spacing(spacing, "lesion_shape")
    if int(n) <= 0:
        return []
    return rows_from_tables(label_shape(labels, n), spacing)
