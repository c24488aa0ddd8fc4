"""Lesion texture report on the device: what a lesion looks like inside -- Haralick's second-order statistics from grey-level
co-occurrence matrices (GLCM), the core of every radiomics toolkit -- without 13 shifted host copies of the scan and a
scatter-add per label.

    t = label_glcm(scan, labels, n)                                     # int64 [n, 13, levels, levels], exact
    f = glcm_features(t)                                                # fp64 arithmetic on those integers
    rows = lesion_texture(scan, labels, n)                              # the two together
    rep = lesion_report(mask, lobe, spacing, scan=scan, texture=True)   # lesions.lesion_report with a `texture` entry

Kernel: csrc/texture.hip, one pass over scan and labels (include/dram_hip.h has the definition).  Only the tables travel to the
host, where everything else is arithmetic on them.

The 13 directions (`OFFSETS`) are VOXEL offsets, multiplied by `distance`.  With anisotropic spacing they have different
physical lengths (a step along z of a 2.5 x 0.7 x 0.7 mm scan is 3.5 times a step along x), and the report does nothing about
it: no resampling, no spacing-weighted mean.  The default window, -1000 .. 200 HU in 16 levels of 75 HU, is stated here and
untuned; values outside it fall in the first or the last level.  Nothing here has been validated clinically.
"""
import numpy as np
import torch

from ._lib import call
from .density import _scan_and_labels
from .surface import _stream

# (dz, dy, dx) of the half 26-neighbourhood in lexicographic order, the first non-zero component positive: the table's second axis
OFFSETS = ((0, 0, 1), (0, 1, -1), (0, 1, 0), (0, 1, 1), (1, -1, -1), (1, -1, 0), (1, -1, 1), (1, 0, -1), (1, 0, 0), (1, 0, 1),
           (1, 1, -1), (1, 1, 0), (1, 1, 1))
LEVELS, LO_HU, WIDTH_HU = 16, -1000, 75
FEATURES = ("asm", "entropy", "contrast", "dissimilarity", "homogeneity", "correlation", "max_probability", "mean_level")


def label_glcm(scan, labels, n, mask=None, levels=LEVELS, lo=LO_HU, width=WIDTH_HU, distance=1):
    """The co-occurrence tables of dram_label_glcm per label k = 1..n of a uint8 or int32 [D,H,W] label volume (taken as it is: a
    lobe map is not widened) over an int16 scan, over the voxels with `mask` set when a mask is given, as one host numpy int64
    array [n, 13, levels, levels] from one device buffer and one read-back.  Entry [k-1, d, i, j] counts the ordered pairs
    (p, p + distance * OFFSETS[d]) inside label k with grey levels i at p and j at the far end, the level of a value v being
    min(max((v - lo) // width, 0), levels - 1).  Not symmetrised: `glcm_features` adds the transpose.  levels in 2..32, distance
    in 1..4, width >= 1.  n == 0: an empty table without a launch."""
    n, levels, lo, width, distance = int(n), int(levels), int(lo), int(width), int(distance)
    if not 2 <= levels <= 32:
        raise ValueError("label_glcm: levels must be in 2..32")
    if not 1 <= distance <= 4:
        raise ValueError("label_glcm: distance must be in 1..4")
    if width < 1:
        raise ValueError("label_glcm: width must be at least 1")
    if not -2 ** 31 <= lo < 2 ** 31:
        raise ValueError("label_glcm: lo must fit in 32 bits")
    if n <= 0 or np.prod(np.shape(labels)) == 0:
        return np.zeros((max(n, 0), 13, levels, levels), np.int64)
    scan, labels, mask = _scan_and_labels(scan, labels, mask, "label_glcm")
    if labels.dim() != 3:
        raise ValueError("label_glcm: scan and labels must be [D,H,W] volumes")
    out = torch.empty((n, 13, levels, levels), dtype=torch.int64, device=labels.device)
    with torch.cuda.device(labels.device):
        call("dram_label_glcm", scan.data_ptr(), labels.data_ptr(), 0 if labels.dtype == torch.uint8 else 1,
             None if mask is None else mask.data_ptr(), n, lo, width, levels, distance, out.data_ptr(), *labels.shape, _stream())
    return out.cpu().numpy()


def glcm_features(tables, per_direction=False):
    """Haralick features from co-occurrence tables [n, 13, levels, levels] (any integer counts), pure host fp64.  Per label and
    direction with C the table: P = C + C^T, p = P / P.sum(), p_i the marginal, mu = sum_i i p_i, var = sum_i (i - mu)^2 p_i and
        pairs            C.sum(), the number of unordered pairs
        asm              sum p^2                       (angular second moment, "energy")
        entropy          -sum p log2 p                 (0 log 0 = 0)
        contrast         sum (i - j)^2 p
        dissimilarity    sum |i - j| p
        homogeneity      sum p / (1 + (i - j)^2)       (inverse difference moment)
        correlation      sum (i - mu)(j - mu) p / var  (NaN when var == 0: a single grey level)
        max_probability  max p
        mean_level       mu
    Returns {"pairs": int64 [n], the pairs of all directions together, feature: fp64 [n]}, each feature the mean over the
    directions that have pairs (`correlation`: over those where it is not NaN) -- the usual radiomics convention; a label
    without any pair gets NaN features and pairs 0.  With `per_direction` also "per_direction": {"pairs": int64 [n, 13],
    feature: fp64 [n, 13]}, NaN where a direction has no pairs."""
    c = np.asarray(tables)
    if c.ndim != 4 or c.shape[2] != c.shape[3]:
        raise ValueError("glcm_features: tables [n, directions, levels, levels]")
    c = c.astype(np.int64)
    n, nd, levels = c.shape[0], c.shape[1], c.shape[2]
    pairs = c.sum(axis=(2, 3))
    sym = (c + c.transpose(0, 1, 3, 2)).astype(np.float64)
    total = sym.sum(axis=(2, 3))
    some = pairs > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        p = sym / total[:, :, None, None]                                 # NaN where a direction has no pairs
        lv = np.arange(levels, dtype=np.float64)
        diff = lv[:, None] - lv[None, :]
        marginal = p.sum(axis=3)
        mu = (marginal * lv).sum(axis=2)
        dev = lv[None, None, :] - mu[:, :, None]
        var = (marginal * dev * dev).sum(axis=2)
        cov = (p * dev[:, :, :, None] * dev[:, :, None, :]).sum(axis=(2, 3))
        plogp = np.where(p > 0, p * np.log2(np.where(p > 0, p, 1.0)), 0.0)
        per = {"asm": (p * p).sum(axis=(2, 3)), "entropy": -plogp.sum(axis=(2, 3)), "contrast": (p * diff * diff).sum(axis=(2, 3)),
               "dissimilarity": (p * np.abs(diff)).sum(axis=(2, 3)), "homogeneity": (p / (1.0 + diff * diff)).sum(axis=(2, 3)),
               "correlation": np.where(var > 0, cov / np.where(var > 0, var, 1.0), np.nan),
               "max_probability": p.max(axis=(2, 3)), "mean_level": mu}
    out = {"pairs": pairs.sum(axis=1)}
    for f in FEATURES:
        v = np.where(some, per[f], np.nan)
        per[f] = v
        ok = ~np.isnan(v)
        cnt = ok.sum(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            out[f] = np.where(cnt > 0, np.where(ok, v, 0.0).sum(axis=1) / np.maximum(cnt, 1), np.nan)
    if per_direction:
        out["per_direction"] = {"pairs": pairs, **{f: per[f] for f in FEATURES}}
    return out


def lesion_texture(scan, labels, n, mask=None, levels=LEVELS, lo=LO_HU, width=WIDTH_HU, distance=1, per_direction=False):
    """`glcm_features(label_glcm(scan, labels, n, ...))`: the texture report of the labels 1..n of a uint8 or int32 [D,H,W] label
    volume over an int16 scan, one dict of arrays with rows in label order.  n == 0: empty arrays without a launch."""
    return glcm_features(label_glcm(scan, labels, n, mask=mask, levels=levels, lo=lo, width=width, distance=distance),
                         per_direction=per_direction)
