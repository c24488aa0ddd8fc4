"""numpy restatement of what the finalise step of csrc/loss.hip's regression-target kernel computes per sample
(dram_intreg_targets): the lesion-ratio upper bound as ONE fp32 division of the two mask sums, the band of
IntRegLoss.get_labels (reference dram/metrics.py:122-138) in fp64 on that value, rounded once to fp32.  Written with
selects instead of the host loop's max / min / if so that it reads like the kernel; the CPU test holds it against
dram_amd.train_step.regression_targets bit for bit, the GPU test uses `branch` to know which case a sample exercises."""
import numpy as np

C_LO = np.array([0.0, 0.001, 0.01, 0.05, 0.35, 0.5])
C_HI = np.array([0.001, 0.01, 0.05, 0.35, 0.5, 1.00001])
OVERLAP, BELOW, ABOVE = 0, 1, 2       # the band meets the class interval / lies wholly below it / wholly above it


def ratio(sum_lesion_in_lobe, sum_lobe):
    """fp32(sum) / fp32(sum): the sums are integers for 0/1 masks."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.float32(sum_lesion_in_lobe) / np.float32(sum_lobe)


def band(ctss, ratio_f32, band_width):
    """-> (targets float32 [N,2], branch int [N]) for integer scores 0..5 and fp32 ratios."""
    c = np.asarray(ctss, dtype=np.int64)
    r = np.asarray(ratio_f32, dtype=np.float32)
    lp = r.astype(np.float64)
    bw = float(band_width)
    lb = np.where(lp - bw > 0.0, lp - bw, 0.0)
    ub = np.where(lp + bw < 1.0, lp + bw, 1.0)
    c_lo, c_hi = C_LO[c], C_HI[c]
    b0 = np.where(lb > c_lo, lb, c_lo)
    b1 = np.where(ub < c_hi, ub, c_hi)
    apart = b1 < b0
    below = apart & (ub <= c_lo)
    above = apart & ~below
    assert np.all(lb[above] >= c_hi[above])          # the third case of the host loop cannot occur
    lo = np.where(below, lb, np.where(above, c_lo, b0))
    hi = np.where(below, ub, np.where(above, c_hi, b1))
    nan = np.isnan(lp)
    lo, hi = np.where(nan, np.nan, lo), np.where(nan, np.nan, hi)
    branch = np.where(below, BELOW, np.where(above, ABOVE, OVERLAP))
    return np.stack([lo, hi], axis=-1).astype(np.float32), branch


def weight_keep(ctss, freq):
    """clamp(fp32(freq[ctss]), 0.2, 0.8) and ctss > 0 (metrics.py:172-174, 326-327)."""
    c = np.asarray(ctss, dtype=np.int64)
    f = np.asarray([freq[k] for k in range(6)], dtype=np.float32)[c]
    return np.minimum(np.maximum(f, np.float32(0.2)), np.float32(0.8)), (c > 0).astype(np.float32)
