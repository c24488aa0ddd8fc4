"""The lesion distribution report restated in plain numpy from the definition in include/dram_hip.h (dram_label_depth) and the
docstrings of dram_amd/distribution.py: what csrc/distribution.hip and the Python report are held against bit for bit.  The
depth map comes from surface_restatement.edt_passes, the percentiles and bands from density_restatement.summary.  Itself held
against a brute-force loop and scipy by tests/test_distribution_cpu.py."""
import math
import struct

import numpy as np

import density_restatement as DR
import surface_restatement as SR

INF_BITS = 0x7f800000
KEYS = ("count", "qsum", "dmin", "dmax", "possum", "hist", "zones")


def lung_depth(lobe, spacing):
    """The distance in mm from every voxel to the nearest voxel with lobe == 0 (float32)."""
    return SR.edt_passes((np.asarray(lobe) == 0).astype(np.uint8), spacing)


def axis_zone(i, a0, a1, nzones):
    i = np.clip(np.asarray(i, dtype=np.int64), a0, a1 - 1)
    return ((i - a0) * nzones) // (a1 - a0)


def bin_of(d, bins_per_mm, nbins):
    """Entry nbins + 1 if fl32(d * bins_per_mm) >= nbins (+inf too), else 1 + trunc of it."""
    with np.errstate(over="ignore"):
        b = np.asarray(d, dtype=np.float32) * np.float32(bins_per_mm)
    over = b >= np.float32(nbins)
    return np.where(over, nbins + 1, 1 + np.where(over, 0, b).astype(np.int64))


def q_of(d):
    return (np.minimum(np.asarray(d, dtype=np.float32), np.float32(2097152.0)) * np.float32(1024.0)).astype(np.int64)


def tables(depth, labels, n, mask=None, bins_per_mm=4, nbins=0, zones=None, box=None):
    """{"count", "qsum": int64 [n], "dmin", "dmax": uint32 [n], "possum": int64 [n,3], "hist": int64 [n, nbins + 2] | None,
    "zones": int64 [n, nz*ny*nx] | None (zones = (nz, ny, nx) or None; box None: the whole volume)}."""
    depth = np.ascontiguousarray(depth, dtype=np.float32)
    D, H, W = depth.shape
    d = depth.reshape(-1)
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    sel = (lab >= 1) & (lab <= n)
    if mask is not None:
        sel &= np.asarray(mask).reshape(-1) != 0
    with np.errstate(invalid="ignore"):
        sel &= d >= np.float32(0.0)                       # NaN and negative depths out; -0.0 and +inf in
    v = np.nonzero(sel)[0]
    k, dv = lab[v] - 1, d[v]
    count = np.bincount(k, minlength=n).astype(np.int64)
    qsum = np.zeros(n, np.int64)
    np.add.at(qsum, k, q_of(dv))
    bits = dv.view(np.uint32).astype(np.int64)
    dmin, dmax = np.full(n, INF_BITS, np.int64), np.zeros(n, np.int64)
    np.minimum.at(dmin, k, bits)
    np.maximum.at(dmax, k, bits)
    z, y, x = v // (H * W), (v // W) % H, v % W
    possum = np.zeros((n, 3), np.int64)
    for a, idx in enumerate((z, y, x)):
        np.add.at(possum[:, a], k, idx)
    hist = None
    if nbins:
        hist = np.zeros((n, nbins + 2), np.int64)
        np.add.at(hist, (k, bin_of(dv, bins_per_mm, nbins)), 1)
    zt = None
    if zones is not None:
        nz, ny, nx = zones
        b = (0, D, 0, H, 0, W) if box is None else tuple(int(t) for t in box)
        zone = (axis_zone(z, b[0], b[1], nz) * ny + axis_zone(y, b[2], b[3], ny)) * nx + axis_zone(x, b[4], b[5], nx)
        zt = np.zeros((n, nz * ny * nx), np.int64)
        np.add.at(zt, (k, zone), 1)
    return {"count": count, "qsum": qsum, "dmin": dmin.astype(np.uint32), "dmax": dmax.astype(np.uint32), "possum": possum,
            "hist": hist, "zones": zt}


def tables_brute(depth, labels, n, mask=None, bins_per_mm=4, nbins=0, zones=None, box=None):
    """The same, voxel by voxel in Python, fp32 arithmetic through struct."""
    f32 = lambda v: struct.unpack("f", struct.pack("f", v))[0]
    D, H, W = depth.shape
    t = {"count": [0] * n, "qsum": [0] * n, "dmin": [INF_BITS] * n, "dmax": [0] * n, "possum": [[0, 0, 0] for _ in range(n)],
         "hist": [[0] * (nbins + 2) for _ in range(n)] if nbins else None,
         "zones": [[0] * (zones[0] * zones[1] * zones[2]) for _ in range(n)] if zones is not None else None}
    b = (0, D, 0, H, 0, W) if box is None else box
    for z in range(D):
        for y in range(H):
            for x in range(W):
                k, d = int(labels[z, y, x]), float(depth[z, y, x])
                if not 1 <= k <= n or (mask is not None and mask[z, y, x] == 0) or not d >= 0.0:
                    continue
                k -= 1
                t["count"][k] += 1
                t["qsum"][k] += int(f32(min(d, 2097152.0) * 1024.0))
                bits = struct.unpack("I", struct.pack("f", d))[0]
                t["dmin"][k], t["dmax"][k] = min(t["dmin"][k], bits), max(t["dmax"][k], bits)
                for a, i in enumerate((z, y, x)):
                    t["possum"][k][a] += i
                if nbins:
                    prod = f32(d * bins_per_mm) if math.isfinite(d) else d
                    t["hist"][k][nbins + 1 if prod >= nbins else 1 + int(prod)] += 1
                if zones is not None:
                    zn = [((min(max(i, b[2 * a]), b[2 * a + 1] - 1) - b[2 * a]) * zones[a]) // (b[2 * a + 1] - b[2 * a]) for a, i in enumerate((z, y, x))]
                    t["zones"][k][(zn[0] * zones[1] + zn[1]) * zones[2] + zn[2]] += 1
    return t


# ---- the report
def shell_bins(shells_mm, bins_per_mm, nbins):
    out = []
    for e in shells_mm:
        j = e * bins_per_mm
        if j != int(j) or not 0 <= j <= nbins:
            raise ValueError("off the bin grid")
        out.append(int(j))
    return out


def peripheral_share(par_hist, les_hist):
    p, les = np.asarray(par_hist, dtype=np.int64), np.asarray(les_hist, dtype=np.int64)
    if p.sum() == 0 or les.sum() == 0:
        return float("nan")
    e = int(np.nonzero(3 * np.cumsum(p) >= p.sum())[0][0])            # the entry that holds the end of the outer third
    return int(les[:e + 1].sum()) / int(les.sum())


def row(t, k, spacing, bins_per_mm=4, nbins=0, percentiles_permille=(), shells_mm=()):
    """One row of the report from the tables, in Python scalars."""
    c = int(t["count"][k])
    nan = float("nan")
    out = {"voxels": np.int64(c), "depth_mean_mm": np.float64(float(int(t["qsum"][k])) / 1024.0 / float(c) if c else nan),
           "depth_min_mm": np.uint32(t["dmin"][k]).view(np.float32), "depth_max_mm": np.uint32(t["dmax"][k]).view(np.float32),
           "centroid": np.array([float(int(t["possum"][k][a])) / float(c) if c else nan for a in range(3)])}
    out["centroid_mm"] = np.array([out["centroid"][a] * float(spacing[a]) for a in range(3)])
    if t["hist"] is not None:
        edges = shell_bins(shells_mm, bins_per_mm, nbins)
        pct, bands = DR.summary(t["hist"][k:k + 1], 0, 1, nbins, percentiles_permille, edges)
        out["percentiles_mm"] = np.array([(math.inf if p == DR.INT32_MAX else int(p) / float(bins_per_mm)) if c else nan for p in pct[0]])
        below = [int(bands[0, :i + 1].sum()) for i in range(len(edges))]
        out["shell_voxels"] = np.array(below, dtype=np.int64)
        out["shell_fraction"] = np.array([b / float(c) if c else nan for b in below], dtype=np.float64)
    if t["zones"] is not None:
        out["zone_voxels"] = np.asarray(t["zones"][k], dtype=np.int64)
        out["zone_fraction"] = np.array([int(v) / float(c) if c else nan for v in t["zones"][k]], dtype=np.float64)
    return out


def total(t):
    one = lambda key: None if t[key] is None else t[key].sum(axis=0, keepdims=True)
    return {"count": one("count"), "qsum": one("qsum"), "dmin": t["dmin"].min(keepdims=True), "dmax": t["dmax"].max(keepdims=True),
            "possum": one("possum"), "hist": one("hist"), "zones": one("zones")}


def entry(whole, inside, k, spacing, **kw):
    p, les = row(whole, k, spacing, **kw), row(inside, k, spacing, **kw)
    a, b = float(les["depth_mean_mm"]), float(p["depth_mean_mm"])
    return {"parenchyma": p, "lesion": les, "peripheral_share": peripheral_share(whole["hist"][k], inside["hist"][k]),
            "depth_ratio": a / b if (a == a and b == b and b != 0.0) else float("nan")}


def centroid_zone(possum, count, box, zones):
    c = int(count)
    if c == 0:
        return None
    zn = [int(axis_zone((2 * int(possum[a]) + c) // (2 * c), box[2 * a], box[2 * a + 1], zones[a])) for a in range(3)]
    return (zn[0] * zones[1] + zn[1]) * zones[2] + zn[2]


def lesion_distribution(mask, lobe, spacing, labels=None, n=0, shells_mm=(5.0, 10.0, 20.0), zones=(3, 2, 1), box=None,
                        percentiles_permille=(150, 500, 850), subpleural_mm=3.0, bins_per_mm=4, nbins=1024):
    """The "lobes", "lungs" and "lesions" entries of dram_amd.distribution.lesion_distribution composed on the CPU."""
    lobe = np.asarray(lobe)
    depth = lung_depth(lobe, spacing)
    present = [int(v) for v in np.unique(lobe) if v != 0]
    if box is None:
        idx = np.argwhere(lobe > 0)
        lo, hi = idx.min(axis=0), idx.max(axis=0) + 1
        box = (lo[0], hi[0], lo[1], hi[1], lo[2], hi[2])
    box = tuple(int(b) for b in box)
    kw = dict(bins_per_mm=bins_per_mm, nbins=nbins, percentiles_permille=percentiles_permille, shells_mm=shells_mm)
    top = max(present)
    whole = tables(depth, lobe, top, None, bins_per_mm, nbins, zones, box)
    inside = tables(depth, lobe, top, mask, bins_per_mm, nbins, zones, box)
    out = {"lobes": {v: entry(whole, inside, v - 1, spacing, **kw) for v in present},
           "lungs": entry(total(whole), total(inside), 0, spacing, **kw), "box": box}
    if labels is not None:
        t = tables(depth, labels, n, None, bins_per_mm, 0, zones, box) if n else None
        rows = [row(t, k, spacing) for k in range(n)]
        keys = ("voxels", "depth_mean_mm", "depth_min_mm", "depth_max_mm", "centroid", "centroid_mm", "zone_voxels", "zone_fraction")
        shapes = {"centroid": (0, 3), "centroid_mm": (0, 3), "zone_voxels": (0, zones[0] * zones[1] * zones[2]),
                  "zone_fraction": (0, zones[0] * zones[1] * zones[2])}
        dtypes = {"voxels": np.int64, "depth_min_mm": np.float32, "depth_max_mm": np.float32, "zone_voxels": np.int64}
        les = {key: (np.stack([r[key] for r in rows]) if n else np.zeros(shapes.get(key, (0,)), dtypes.get(key, np.float64))) for key in keys}
        les["subpleural"] = np.array([float(r["depth_min_mm"]) <= subpleural_mm for r in rows], dtype=bool)
        les["zone"] = [centroid_zone(t["possum"][k], t["count"][k], box, zones) for k in range(n)]
        out["lesions"] = les
    return out
