"""Heat-map evaluation curves on the device: voxel-wise ROC and precision / recall, the Dice / IoU sweep over the threshold and a
calibration table of a probability map against a reference mask, per region (lobe) and pooled -- without pulling the fp32 map and
three uint8 volumes to the host for sklearn.

    c = heatmap_curves(htp, lesion, regions=lobe, n_regions=5)          # c["auc_roc"][-1]: the whole lungs; c["best_dice"], c["ece"]
    t = score_tables(htp, lesion, lobe, 5); ...                          # tables of several scans add: pool a data set, then
    c = curves_from_tables(sum_hist, sum_conf)                           # one set of curves for it

Kernel: csrc/curves.hip, one pass that builds the joint histogram of score bin x class x region (`score_tables`).  Only that table
-- a few thousand integers -- travels to the host; every curve is then exact integer arithmetic on it (`curves_from_tables`,
which needs no GPU).

The score axis is cut at t_j = j / nbins, j = 0..nbins-1.  A voxel is predicted at cut j iff its score is >= t_j and the gate
(if any) is on; a voxel with the gate off, a negative or a NaN score is never predicted (bin 0).  Scores are therefore resolved to
1 / nbins: ROC-AUC and average precision are those of the binned score (ties inside a bin count half, as sklearn counts ties).
"""
import numpy as np
import torch

from ._lib import call
from .surface import _device_u8, _stream

CONF_ONE = 1 << 24          # the fixed-point unit of the confidence sums (csrc/curves.hip: curves_q)


def _check_bins(nbins, who):
    nbins = int(nbins)
    if nbins < 2 or nbins > 4096 or nbins & (nbins - 1):
        raise ValueError(f"{who}: nbins must be a power of two in 2..4096")
    return nbins


def score_tables(score, reference, regions=None, n_regions=1, gate=None, nbins=1024, conf=True):
    """The joint histogram of a score map [any shape, float32] against `reference` (non-zero = positive) as host numpy arrays:
    {"hist": int64 [n_regions, 2, nbins + 1], "conf": the same shape or None}.  hist[r-1, c, b] counts the voxels of region r
    (`regions`: a uint8 label map; labels 0 and above n_regions are skipped; None = one region holding every voxel), class c and
    bin b: 0 where `gate` (optional, non-zero = on) is off or the score is negative or NaN, nbins where it is >= 1, else
    1 + floor(score * nbins).  conf[r-1, c, b] is the sum of floor(min(score, 1) * 2^24) over the same voxels (0 for b = 0).
    Inputs may live on the host or the device; only the tables come back.  Tables of different scans add."""
    nbins = _check_bins(nbins, "score_tables")
    n_regions = int(n_regions)
    if not 1 <= n_regions <= 255:
        raise ValueError("score_tables: n_regions must be in 1..255")
    if regions is None and n_regions != 1:
        raise ValueError("score_tables: without a region map there is one region (n_regions = 1)")
    score = torch.as_tensor(score)
    if score.dtype != torch.float32:
        raise ValueError("score_tables: the score map must be float32")
    reference = torch.as_tensor(reference)
    others = [t for t in (reference, regions, gate) if isinstance(t, torch.Tensor) and t.is_cuda]
    dev = score.device if score.is_cuda else (others[0].device if others else torch.device("cuda", torch.cuda.current_device()))
    score = score.to(dev).contiguous()
    reference = _device_u8(reference, dev)
    if regions is not None:
        regions = torch.as_tensor(regions)
        if regions.dtype != torch.uint8:
            raise ValueError("score_tables: the region map must be uint8")
        regions = regions.to(dev).contiguous()
    gate = None if gate is None else _device_u8(gate, dev)
    for name, t in (("reference", reference), ("regions", regions), ("gate", gate)):
        if t is not None and t.shape != score.shape:
            raise ValueError(f"score_tables: {name} and score must have the same shape")
    shape = (n_regions, 2, nbins + 1)
    if score.numel() == 0:
        return {"hist": np.zeros(shape, np.int64), "conf": np.zeros(shape, np.int64) if conf else None}
    # one buffer, one read-back: hist | conf
    buf = torch.empty((2 if conf else 1,) + shape, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        call("dram_score_hist", score.data_ptr(), reference.data_ptr(), None if regions is None else regions.data_ptr(),
             None if gate is None else gate.data_ptr(), n_regions, nbins, buf[0].data_ptr(), buf[1].data_ptr() if conf else None,
             score.numel(), _stream())
    host = buf.cpu().numpy()
    return {"hist": host[0].copy(), "conf": host[1].copy() if conf else None}


def _ratio(num, den):
    """num / den in fp64, NaN where den == 0."""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    out = np.full(np.broadcast(num, den).shape, np.nan)
    np.divide(num, den, out=out, where=den != 0)
    return out


def curves_from_tables(hist, conf=None, n_cal=16, smooth=1e-5):
    """Every curve from the tables of `score_tables` (host arithmetic only).  One row per region plus a last row for the regions
    pooled (their sum).  Per cut j = 0..nbins-1, threshold t_j = j / nbins, predicted = bin >= j + 1:
        thresholds [nbins]; tp, fp, fn, tn (int64 [rows, nbins]); tpr, fpr, precision (fp64, NaN where the denominator is 0);
        dice, iou with the reference's smooth term: inference.dice / iou of ((score >= t_j) & gate) against the reference mask;
        best_dice, best_dice_threshold [rows]: the first of equal maxima (the lowest threshold).
    Over the nbins + 1 levels, bin 0 the lowest:
        auc_roc [rows]: the Mann-Whitney statistic with ties counted half, formed in Python integers and divided once (equal to
            sklearn.metrics.roc_auc_score(reference, bin)); NaN if a class is empty.
        average_precision [rows]: sklearn's step sum, sum over the levels of (recall gained at the level) * (precision at the
            level) (equal to average_precision_score(reference, bin)); NaN without a positive.
    With `conf` and n_cal (a power of two dividing nbins; None = skip), over the bins >= 1 in n_cal groups of equal width:
        cal_count, cal_positive (int64 [rows, n_cal]); cal_confidence = sum of scores / count (the fixed-point sums / (count * 2^24));
        cal_frequency = positive / count (both NaN for an empty group); ece = sum_i count_i / total * |frequency_i - confidence_i|
        (NaN when no voxel is in a bin >= 1)."""
    hist = np.asarray(hist)
    if hist.ndim != 3 or hist.shape[1] != 2 or hist.dtype.kind not in "iu":
        raise ValueError("curves_from_tables: hist must be an integer [regions, 2, nbins + 1] table")
    nbins = _check_bins(hist.shape[2] - 1, "curves_from_tables")
    hist = hist.astype(np.int64)
    hist = np.concatenate([hist, hist.sum(axis=0, keepdims=True)], axis=0)
    neg, pos = hist[:, 0, :], hist[:, 1, :]
    rows = hist.shape[0]
    P, N = pos.sum(axis=1), neg.sum(axis=1)
    # predicted at cut j: the bins j + 1 .. nbins
    tp = np.cumsum(pos[:, :0:-1], axis=1)[:, ::-1]
    fp = np.cumsum(neg[:, :0:-1], axis=1)[:, ::-1]
    fn, tn = P[:, None] - tp, N[:, None] - fp
    out = {"thresholds": np.arange(nbins, dtype=np.float64) / nbins, "tp": tp, "fp": fp, "fn": fn, "tn": tn,
           "tpr": _ratio(tp, P[:, None]), "fpr": _ratio(fp, N[:, None]), "precision": _ratio(tp, tp + fp)}
    out["dice"] = (2.0 * tp + smooth) / ((tp + fp) + P[:, None] + smooth)
    out["iou"] = (tp + smooth) / ((tp + fp + fn) + smooth)
    best = np.argmax(out["dice"], axis=1)
    out["best_dice"] = out["dice"][np.arange(rows), best]
    out["best_dice_threshold"] = out["thresholds"][best]
    auc, ap = np.full(rows, np.nan), np.full(rows, np.nan)
    for k in range(rows):
        if P[k] and N[k]:
            # 2U = sum_b pos[b] * (2 * neg_below[b] + neg[b]); the products leave int64 on a pooled data set: Python integers
            weight = 2 * (np.cumsum(neg[k]) - neg[k]) + neg[k]
            two_u = int(np.dot(pos[k].astype(object), weight.astype(object)))
            auc[k] = two_u / (2 * int(P[k]) * int(N[k]))
        if P[k]:
            # level b predicts the bins >= b: precision there, weighted by the recall gained there
            tp_at = np.cumsum(pos[k, ::-1])[::-1]
            all_at = tp_at + np.cumsum(neg[k, ::-1])[::-1]
            hit = pos[k] > 0
            ap[k] = float(np.sum((pos[k, hit] / float(P[k])) * (tp_at[hit] / all_at[hit].astype(np.float64))))
    out["auc_roc"], out["average_precision"] = auc, ap
    if conf is not None and n_cal is not None:
        n_cal = int(n_cal)
        if n_cal < 1 or n_cal & (n_cal - 1) or nbins % n_cal:
            raise ValueError("curves_from_tables: n_cal must be a power of two that divides nbins")
        conf = np.asarray(conf)
        if conf.shape != (rows - 1, 2, nbins + 1):
            raise ValueError("curves_from_tables: conf must have the shape of hist")
        conf = conf.astype(np.int64)
        conf = np.concatenate([conf, conf.sum(axis=0, keepdims=True)], axis=0)
        grouped = lambda t: t[:, 1:].reshape(rows, n_cal, nbins // n_cal).sum(axis=2)
        count, positive, csum = grouped(pos + neg), grouped(pos), grouped(conf[:, 0, :] + conf[:, 1, :])
        confidence = _ratio(csum, count.astype(np.float64) * CONF_ONE)
        frequency = _ratio(positive, count)
        total = count.sum(axis=1)
        gap = np.where(count > 0, np.abs(frequency - confidence), 0.0)
        ece = _ratio((count * gap).sum(axis=1), total)
        out.update(cal_count=count, cal_positive=positive, cal_confidence=confidence, cal_frequency=frequency, ece=ece)
    return out


def heatmap_curves(score, reference, regions=None, n_regions=1, gate=None, nbins=1024, n_cal=16):
    """`curves_from_tables` of `score_tables`: the curves of one heat map in one call."""
    t = score_tables(score, reference, regions, n_regions, gate, nbins, conf=n_cal is not None)
    return curves_from_tables(t["hist"], t["conf"], n_cal)
