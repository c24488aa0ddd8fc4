"""Plain numpy restatement of the heat-map evaluation curves, written from the definitions in include/dram_hip.h ("heat-map
evaluation curves") and in the docstrings of dram_amd/curves.py, not from their code: the voxel -> (region, class, bin) rule, the
fixed-point confidence sums, and every curve from the counts.  tests/test_curves_cpu.py holds it against sklearn and against
inference.dice / iou.

Everything that is an integer is computed in integers (int64, or Python integers where a product can leave int64)."""
import numpy as np

TWO24 = 16777216


def bin_index(score, gate, nbins):
    """Per voxel: 0 if the gate is off or not (score >= 0); nbins if score >= 1; else 1 + floor(score * nbins), the product taken
    in fp64 (it is exact in fp32 as well: nbins is a power of two)."""
    s = np.asarray(score, dtype=np.float32).reshape(-1)
    out = np.zeros(s.size, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        ok = s >= np.float32(0.0)                              # False for NaN
        if gate is not None:
            ok &= np.asarray(gate).reshape(-1) != 0
        top = ok & (s >= np.float32(1.0))
        mid = ok & ~top
    out[top] = nbins
    out[mid] = 1 + np.floor(s[mid].astype(np.float64) * nbins).astype(np.int64)
    return out


def confidence_q(score):
    """floor(min(score, 1) * 2^24) per voxel as int64 (0 where the score is NaN or negative: such voxels are in bin 0 anyway)."""
    s = np.asarray(score, dtype=np.float32).reshape(-1).astype(np.float64)
    with np.errstate(invalid="ignore"):
        good = s >= 0.0
    q = np.zeros(s.size, dtype=np.int64)
    q[good] = np.floor(np.minimum(s[good], 1.0) * TWO24).astype(np.int64)
    return q


def tables(score, ref, region, nregions, gate, nbins, with_conf=True):
    """(hist, conf | None): int64 [nregions, 2, nbins + 1]."""
    b = bin_index(score, gate, nbins)
    c = (np.asarray(ref).reshape(-1) != 0).astype(np.int64)
    r = np.ones(b.size, dtype=np.int64) if region is None else np.asarray(region).reshape(-1).astype(np.int64)
    keep = (r >= 1) & (r <= nregions)
    flat = ((r[keep] - 1) * 2 + c[keep]) * (nbins + 1) + b[keep]
    size = nregions * 2 * (nbins + 1)
    hist = np.bincount(flat, minlength=size).astype(np.int64).reshape(nregions, 2, nbins + 1)
    conf = None
    if with_conf:
        q = np.where(b > 0, confidence_q(score), 0)[keep]
        conf = np.zeros(size, dtype=np.int64)
        np.add.at(conf, flat, q)
        conf = conf.reshape(nregions, 2, nbins + 1)
    return hist, conf


def _div(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(b != 0, a / np.where(b != 0, b, 1.0), np.nan)


def curves(hist, conf=None, n_cal=16, smooth=1e-5):
    """The curves of one table, rows = the regions and then their sum.  See curves_from_tables' docstring for the definitions."""
    hist = np.asarray(hist, dtype=np.int64)
    full = np.concatenate([hist, hist.sum(axis=0)[None]], axis=0)
    rows, nbins = full.shape[0], full.shape[2] - 1
    out = {k: [] for k in ("tp", "fp", "fn", "tn", "tpr", "fpr", "precision", "dice", "iou", "best_dice", "best_dice_threshold",
                           "auc_roc", "average_precision")}
    out["thresholds"] = np.array([j / nbins for j in range(nbins)], dtype=np.float64)
    for k in range(rows):
        neg, pos = full[k, 0], full[k, 1]
        P, N = int(pos.sum()), int(neg.sum())
        # cut j predicts the bins > j: what is not predicted are the bins 0..j
        fn = np.cumsum(pos)[:nbins]
        tn = np.cumsum(neg)[:nbins]
        tp, fp = P - fn, N - tn
        dice = (2.0 * tp + smooth) / (tp + fp + P + smooth)
        iou = (tp + smooth) / (tp + fp + fn + smooth)
        j_best = int(np.flatnonzero(dice == dice.max())[0])
        for key, v in (("tp", tp), ("fp", fp), ("fn", fn), ("tn", tn), ("tpr", _div(tp, P)), ("fpr", _div(fp, N)),
                       ("precision", _div(tp, tp + fp)), ("dice", dice), ("iou", iou), ("best_dice", dice[j_best]),
                       ("best_dice_threshold", j_best / nbins)):
            out[key].append(v)
        # Mann-Whitney with ties counted half: pairs (positive, negative) with the positive in the higher level, plus half the
        # pairs in the same level
        if P and N:
            twice, seen = 0, 0
            for b in range(nbins + 1):
                twice += int(pos[b]) * (2 * seen + int(neg[b]))
                seen += int(neg[b])
            out["auc_roc"].append(twice / (2 * P * N))
        else:
            out["auc_roc"].append(np.nan)
        # sklearn's average precision: walk the occupied levels from the highest down; each adds its gain in recall times the
        # precision reached
        if P:
            ap, tps, fps = 0.0, 0, 0
            for b in range(nbins, -1, -1):
                if pos[b] or neg[b]:
                    tps, fps = tps + int(pos[b]), fps + int(neg[b])
                    ap += (int(pos[b]) / P) * (tps / (tps + fps))
            out["average_precision"].append(ap)
        else:
            out["average_precision"].append(np.nan)
    res = {k: np.array(v) for k, v in out.items()}
    for key in ("tp", "fp", "fn", "tn"):
        res[key] = res[key].astype(np.int64)
    if conf is not None and n_cal is not None:
        conf = np.asarray(conf, dtype=np.int64)
        cfull = np.concatenate([conf, conf.sum(axis=0)[None]], axis=0)
        w = nbins // n_cal
        count, positive, csum = (np.zeros((rows, n_cal), dtype=np.int64) for _ in range(3))
        for i in range(n_cal):
            sl = slice(1 + i * w, 1 + (i + 1) * w)
            count[:, i] = full[:, :, sl].sum(axis=(1, 2))
            positive[:, i] = full[:, 1, sl].sum(axis=1)
            csum[:, i] = cfull[:, :, sl].sum(axis=(1, 2))
        confidence = _div(csum, count.astype(np.float64) * TWO24)
        frequency = _div(positive, count)
        ece = np.full(rows, np.nan)
        for k in range(rows):
            total = int(count[k].sum())
            if total:
                ece[k] = sum(int(count[k, i]) * abs(frequency[k, i] - confidence[k, i]) for i in range(n_cal) if count[k, i]) / total
        res.update(cal_count=count, cal_positive=positive, cal_confidence=confidence, cal_frequency=frequency, ece=ece)
    return res


def heatmap_curves(score, ref, region=None, nregions=1, gate=None, nbins=1024, n_cal=16):
    hist, conf = tables(score, ref, region, nregions, gate, nbins, with_conf=n_cal is not None)
    return curves(hist, conf, n_cal)
