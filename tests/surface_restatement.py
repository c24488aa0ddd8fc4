"""numpy fp64 restatements of csrc/distance.hip and dram_amd/surface.py, and the cases both test files share.

(a) `edt_brute`: the definition -- d2[v] = min over features f of fl(fl(fl(dx^2 wx) + fl(dy^2 wy)) + fl(dz^2 wz)), every
    operation a rounded fp64 numpy operation (numpy never fuses a product with a sum), the minimum over all features in chunks;
(b) `edt_passes`: the three separable passes in the device's order (x: integer distance to the nearest feature of the row;
    y, z: the plain minimum over the line), `edt_passes_d2` without the final square root;
(c) `surface`, `surface_metrics`: the 6-neighbour surface, the two directed distance sets from (a) and the four metrics.
Results are cached per case: a reference is computed once, shared and never written to."""
import functools

import numpy as np

ANISO = (2.5, 0.7, 0.8)


def weights(spacing):
    sz, sy, sx = (np.float64(s) for s in spacing)
    return sz * sz, sy * sy, sx * sx


def edt_brute_d2(feature, spacing, chunk=256):
    wz, wy, wx = weights(spacing)
    D, H, W = feature.shape
    d2 = np.full(feature.shape, np.inf)
    f = np.argwhere(feature != 0)
    z = np.arange(D, dtype=np.int64)[:, None, None, None]
    y = np.arange(H, dtype=np.int64)[None, :, None, None]
    x = np.arange(W, dtype=np.int64)[None, None, :, None]
    for k in range(0, len(f), chunk):
        fz, fy, fx = (f[k:k + chunk, a][None, None, None, :] for a in range(3))
        tx = ((x - fx) ** 2).astype(np.float64) * wx
        ty = ((y - fy) ** 2).astype(np.float64) * wy
        tz = ((z - fz) ** 2).astype(np.float64) * wz
        d2 = np.minimum(d2, ((tx + ty) + tz).min(axis=3))
    return d2


def edt_brute(feature, spacing):
    """(a): float32, +inf everywhere without a feature."""
    return np.sqrt(edt_brute_d2(feature, spacing)).astype(np.float32)


def _line_min(g, w, axis):
    """out[i] = min_j fl(g[j] + fl((i - j)^2 w)) along `axis`."""
    g = np.moveaxis(g, axis, 0)
    n = g.shape[0]
    i = np.arange(n, dtype=np.int64)
    cost = ((i[:, None] - i[None, :]) ** 2).astype(np.float64) * w                     # [i, j]
    out = (g[None, ...] + cost.reshape(n, n, *([1] * (g.ndim - 1)))).min(axis=1)
    return np.moveaxis(out, 0, axis)


def edt_passes_d2(feature, spacing):
    wz, wy, wx = weights(spacing)
    D, H, W = feature.shape
    x = np.arange(W, dtype=np.int64)
    set_ = feature != 0
    # x: |dx| to the nearest feature of the row, -1 for none
    dist = np.where(set_[:, :, None, :], np.abs(x[:, None] - x[None, :])[None, None], np.iinfo(np.int64).max).min(axis=3)
    dx = np.where(set_.any(axis=2, keepdims=True), dist, -1)
    g1 = np.where(dx < 0, np.inf, (np.maximum(dx, 0) ** 2).astype(np.float64) * wx)
    return _line_min(_line_min(g1, wy, 1), wz, 0)


def edt_passes(feature, spacing):
    """(b)"""
    return np.sqrt(edt_passes_d2(feature, spacing)).astype(np.float32)


def surface(mask):
    """(c): set voxels with a face neighbour that is unset or outside the volume, as uint8."""
    m = np.pad(mask != 0, 1)
    inner = m[1:-1, 1:-1, 1:-1]
    all_six = m[:-2, 1:-1, 1:-1] & m[2:, 1:-1, 1:-1] & m[1:-1, :-2, 1:-1] & m[1:-1, 2:, 1:-1] & m[1:-1, 1:-1, :-2] & m[1:-1, 1:-1, 2:]
    return (inner & ~all_six).astype(np.uint8)


def surface_metrics(pred, ref, spacing, q=95.0, tolerances=()):
    """(c): the dictionary of dram_amd.surface.surface_distances, with `within` = the integer counts behind nsd."""
    sp, sr = surface(pred), surface(ref)
    n_p, n_r = int(sp.sum()), int(sr.sum())
    name = "hd" + (str(int(q)) if q == int(q) else str(q))
    out = {"n_pred_surface": n_p, "n_ref_surface": n_r}
    if n_p == 0 or n_r == 0:
        bad = np.nan if n_p == n_r else np.inf
        out.update({"hd": bad, name: bad, "assd": bad, "nsd": {t: np.nan if n_p == n_r else 0.0 for t in tolerances}, "within": {}})
        return out
    a = edt_brute(sr, spacing)[sp != 0].astype(np.float64)
    b = edt_brute(sp, spacing)[sr != 0].astype(np.float64)
    both = np.sort(np.concatenate((a, b)))
    within = {t: int(np.count_nonzero(both <= t)) for t in tolerances}
    out.update({"hd": float(both[-1]), name: float(np.percentile(both, q)), "assd": float((a.sum() + b.sum()) / (n_p + n_r)),
                "nsd": {t: within[t] / (n_p + n_r) for t in tolerances}, "within": within})
    return out


# ---- the shared cases: name -> (feature builder, spacing)
def _random(shape, p, seed):
    return (np.random.default_rng(seed).random(shape) < p).astype(np.uint8)


def _at(shape, *points, value=1):
    f = np.zeros(shape, np.uint8)
    for p in points:
        f[p] = value
    return f


def _plane(shape, z, p, seed):
    f = np.zeros(shape, np.uint8)
    f[z] = _random(shape[1:], p, seed)
    return f


# One more than what one lap of a pass handles (csrc/distance.hip): edt_x takes a row in ballots of 64 voxels (one wave);
# a block of edt_axis produces EDT_OC = EDT_TY * EDT_R = 4 * 16 = 64 outputs per lap and stages EDT_SC = 64 sources per LDS chunk.
LONG = 65

CASES = {
    "one_voxel_set": (lambda: _at((1, 1, 1), (0, 0, 0)), (1.0, 1.0, 1.0)),
    "one_voxel_unset": (lambda: np.zeros((1, 1, 1), np.uint8), (1.0, 1.0, 1.0)),
    "row_70_both_ends": (lambda: _at((1, 1, 70), (0, 0, 0), (0, 0, 69)), (1.0, 1.0, 1.0)),
    "random_3x67x130": (lambda: _random((3, 67, 130), 0.02, 11), ANISO),
    "single_plane_6x40x40": (lambda: _plane((6, 40, 40), 4, 0.01, 12), (1.3, 0.9, 2.1)),
    "no_feature_5x7x9": (lambda: np.zeros((5, 7, 9), np.uint8), (1.0, 1.0, 1.0)),
    "corner_9x33x70": (lambda: _at((9, 33, 70), (8, 32, 69), value=255), (3.3, 0.61, 1.7)),
    "ties_5x8x12": (lambda: _at((5, 8, 12), (0, 1, 2), (4, 6, 9)), (0.7, 1.1, 0.3)),
}
for _name, _shape in (("long_x", (2, 3, LONG)), ("long_y", (2, LONG, 3)), ("long_z", (LONG, 2, 3))):
    CASES[_name + "_unit"] = (functools.partial(_random, _shape, 0.03, 21), (1.0, 1.0, 1.0))
    CASES[_name + "_aniso"] = (functools.partial(_random, _shape, 0.03, 22), ANISO)
    # features at the far end only: the minimum of the first lap's outputs comes from the second chunk of sources
    CASES[_name + "_far_end"] = (functools.partial(_at, _shape, tuple(s - 1 for s in _shape)), ANISO)
UNIT_CASES = [n for n, (_, sp) in CASES.items() if sp == (1.0, 1.0, 1.0)]


@functools.lru_cache(maxsize=None)
def feature_of(name):
    f = CASES[name][0]()
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def brute_d2_of(name):
    d2 = edt_brute_d2(feature_of(name), CASES[name][1])
    d2.setflags(write=False)
    return d2


def expected(name):
    return np.sqrt(brute_d2_of(name)).astype(np.float32)


def blobs(shape, centres, radii):
    z, y, x = np.meshgrid(*(np.arange(s, dtype=np.float64) for s in shape), indexing="ij")
    m = np.zeros(shape, bool)
    for (cz, cy, cx), (rz, ry, rx) in zip(centres, radii):
        m |= ((z - cz) / rz) ** 2 + ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0
    return m.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def blob_pair():
    """Two overlapping blobby masks at (9, 70, 67), the second one touching a face of the volume."""
    shape = (9, 70, 67)
    pred = blobs(shape, [(4, 20, 20), (3, 45, 40), (6, 60, 10)], [(3.2, 9.5, 11.0), (2.5, 12.0, 8.0), (1.5, 4.0, 5.0)])
    ref = blobs(shape, [(4, 23, 18), (4, 44, 44), (0, 10, 60)], [(3.0, 8.0, 12.5), (3.5, 10.0, 9.0), (2.0, 6.0, 5.5)])
    pred.setflags(write=False)
    ref.setflags(write=False)
    return pred, ref


TOLERANCES = (0.0, 0.8, 1.0, 2.5, 0.1)


@functools.lru_cache(maxsize=None)
def blob_metrics():
    pred, ref = blob_pair()
    return surface_metrics(pred, ref, ANISO, 95.0, TOLERANCES)
