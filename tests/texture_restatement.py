"""The lesion texture tables restated in plain numpy (nothing of dram_amd.texture is imported): per direction two shifted views of
the grey-level volume and of the label volume, the validity predicate, and a bincount of the packed key; and the Haralick
features from a table, written on their own."""
import numpy as np

# (dz, dy, dx) of the half 26-neighbourhood in lexicographic order, the first non-zero component positive
OFFSETS = ((0, 0, 1), (0, 1, -1), (0, 1, 0), (0, 1, 1), (1, -1, -1), (1, -1, 0), (1, -1, 1), (1, 0, -1), (1, 0, 0), (1, 0, 1),
           (1, 1, -1), (1, 1, 0), (1, 1, 1))
FEATURES = ("asm", "entropy", "contrast", "dissimilarity", "homogeneity", "correlation", "max_probability", "mean_level")


def grey_levels(scan, lo, width, levels):
    """min(max((v - lo) / width, 0), levels - 1): the sign of the quotient is all that matters below lo, so floor division
    serves."""
    v = np.asarray(scan).astype(np.int64)
    return np.clip((v - int(lo)) // int(width), 0, int(levels) - 1)


def _views(a, off):
    """(a[p], a[p + off]) over every p for which both lie inside the volume."""
    lo = [max(0, -s) for s in off]
    hi = [dim - max(0, s) for s, dim in zip(off, a.shape)]
    if any(h <= l for l, h in zip(lo, hi)):
        return a[:0, :0, :0], a[:0, :0, :0]
    p = a[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
    q = a[lo[0] + off[0]:hi[0] + off[0], lo[1] + off[1]:hi[1] + off[1], lo[2] + off[2]:hi[2] + off[2]]
    return p, q


def glcm(scan, labels, n, mask=None, levels=16, lo=-1000, width=75, distance=1):
    """int64 [n, 13, levels, levels] of include/dram_hip.h (dram_label_glcm)."""
    g = grey_levels(scan, lo, width, levels)
    lab = np.asarray(labels).astype(np.int64)
    lab = np.where((lab >= 1) & (lab <= n), lab, 0)
    if mask is not None:
        lab = np.where(np.asarray(mask) != 0, lab, 0)
    out = np.zeros((n, 13, levels, levels), dtype=np.int64)
    for i, off in enumerate(OFFSETS):
        off = tuple(distance * s for s in off)
        lp, lq = _views(lab, off)
        gp, gq = _views(g, off)
        ok = (lp > 0) & (lp == lq)
        key = ((lp[ok] - 1) * levels + gp[ok]) * levels + gq[ok]
        out[:, i] = np.bincount(key, minlength=n * levels * levels).reshape(n, levels, levels)
    return out


def features_of(table):
    """The features of one [levels, levels] count table in fp64, or None for a table without pairs."""
    c = np.asarray(table, dtype=np.int64)
    total = int(c.sum())
    if total == 0:
        return None
    sym = (c + c.T).astype(np.float64)
    p = sym / sym.sum()
    levels = c.shape[0]
    i, j = np.meshgrid(np.arange(levels, dtype=np.float64), np.arange(levels, dtype=np.float64), indexing="ij")
    marginal = p.sum(axis=1)
    mu = float((np.arange(levels) * marginal).sum())
    var = float((((np.arange(levels) - mu) ** 2) * marginal).sum())
    nz = p[p > 0]
    return {"pairs": total, "asm": float((p * p).sum()), "entropy": float(-(nz * np.log2(nz)).sum()),
            "contrast": float(((i - j) ** 2 * p).sum()), "dissimilarity": float((np.abs(i - j) * p).sum()),
            "homogeneity": float((p / (1.0 + (i - j) ** 2)).sum()),
            "correlation": float(((i - mu) * (j - mu) * p).sum() / var) if var > 0 else float("nan"),
            "max_probability": float(p.max()), "mean_level": mu}


def features(tables):
    """{"pairs": int64 [n] (summed over the directions), feature: fp64 [n]}: each feature the mean over the directions that have
    pairs (correlation: over those where it is not NaN); NaN for a label without pairs."""
    tables = np.asarray(tables)
    n = tables.shape[0]
    out = {"pairs": np.zeros(n, dtype=np.int64)}
    out.update({f: np.full(n, np.nan) for f in FEATURES})
    for k in range(n):
        rows = [features_of(tables[k, d]) for d in range(tables.shape[1])]
        rows = [r for r in rows if r is not None]
        out["pairs"][k] = sum(r["pairs"] for r in rows)
        for f in FEATURES:
            vals = [r[f] for r in rows if not np.isnan(r[f])]
            if vals:
                out[f][k] = sum(vals) / len(vals)
    return out
