"""numpy fp64 restatement of the reference's two voxel-wise segmentation losses (dram/metrics.py:10-72) and of their
gradients with respect to p, written from the formulas of include/dram_hip.h -- the sums-only form the kernels use:

    BootBinCrossEntropy(s)(p, t, voi), eps = 1e-7
        pt = p t + (1 - p)(1 - t),  nll = -log(clamp(pt, eps, 1 - eps)),  nll_hat the same with t_hat = [p > 0.5]
        out = {voi < 1e-7}, in = {voi > 0};  T = sum_in t,  A = sum_in t nll,  B = sum_in (1 - t) nll
        alpha = clamp(1 - T / n_in, .25, .75),  W = alpha T + (1 - alpha)(n_in - T)
        loss = sum_out nll / n_out + [n_in > 0] ((1 - s)(alpha A + (1 - alpha) B) / W + s sum_in nll_hat / n_in)
    BinaryCrossEntropySmooth(s)(p, t), pc = clamp(p, 1e-6, 1 - 1e-6)
        T = sum t,  alpha = clamp(1 - T / n, .3, .7),  W = alpha T + (1 - alpha)(n - T)
        loss = -s (alpha sum t log pc + (1 - alpha) sum (1 - t) log(1 - pc)) / W

The clamp's gradient is torch's: 1 where lo <= x <= hi (bounds included), 0 outside.  t_hat and alpha are constants.
tests/test_seg_loss_cpu.py pins this file to torch's fp64 evaluation of oracle.dram_oracle.boot_bce, to a direct torch
transcription of BinaryCrossEntropySmooth and to the reference's own classes (tests/golden/segloss.npz).

`eps`, `lo` and `hi` default to the fp64 constants; a caller whose inputs sit on a bound may pass the fp32-rounded ones.
"""
import numpy as np
import torch

BOOT_EPS = 1e-7
SMOOTH_EPS = 1e-6


def _f64(a):
    return np.asarray(a, dtype=np.float64).reshape(-1)


def boot_bce_sums(p, t, voi, eps=BOOT_EPS, hi=None):
    """The seven totals in the kernels' order: n_out, sum_out nll, n_in, T, A, B, sum_in nll_hat."""
    p, t, voi = _f64(p), _f64(t), _f64(voi)
    hi = 1.0 - eps if hi is None else hi
    nll = -np.log(np.clip(p * t + (1.0 - p) * (1.0 - t), eps, hi))
    nll_hat = -np.log(np.clip(np.where(p > 0.5, p, 1.0 - p), eps, hi))
    out, ins = voi < 1e-7, voi > 0
    return np.array([out.sum(), nll[out].sum(), ins.sum(), t[ins].sum(), (t * nll)[ins].sum(), ((1.0 - t) * nll)[ins].sum(),
                     nll_hat[ins].sum()], dtype=np.float64)


def boot_bce_from_sums(sums, smoothing):
    """(loss, alpha, W) from the seven totals alone -- the finish kernel's arithmetic."""
    n_out, s_out, n_in, T, A, B, H = (float(v) for v in sums)
    with np.errstate(invalid="ignore", divide="ignore"):
        loss = np.float64(s_out) / np.float64(n_out)           # 0 / 0 = nan: torch's mean of an empty tensor
    if not n_in > 0:
        return float(loss), 0.0, 0.0
    alpha = min(max(1.0 - T / n_in, 0.25), 0.75)
    W = alpha * T + (1.0 - alpha) * (n_in - T)
    return float(loss + (1.0 - smoothing) * (alpha * A + (1.0 - alpha) * B) / W + smoothing * H / n_in), alpha, W


def boot_bce(p, t, voi, smoothing=0.1, eps=BOOT_EPS, hi=None):
    return boot_bce_from_sums(boot_bce_sums(p, t, voi, eps, hi), smoothing)[0]


def boot_bce_grad(p, t, voi, smoothing=0.1, eps=BOOT_EPS, hi=None):
    """d loss / d p, in p's shape."""
    shape = np.shape(p)
    p, t, voi = _f64(p), _f64(t), _f64(voi)
    hi = 1.0 - eps if hi is None else hi
    sums = boot_bce_sums(p, t, voi, eps, hi)
    _, alpha, W = boot_bce_from_sums(sums, smoothing)
    n_out, n_in = sums[0], sums[2]
    pt = p * t + (1.0 - p) * (1.0 - t)
    dnll = np.where((pt >= eps) & (pt <= hi), -(2.0 * t - 1.0) / pt, 0.0)
    up = p > 0.5
    ph = np.where(up, p, 1.0 - p)
    dhat = np.where((ph >= eps) & (ph <= hi), np.where(up, -1.0, 1.0) / ph, 0.0)
    g = np.zeros_like(p)
    out, ins = voi < 1e-7, voi > 0
    g[out] += dnll[out] / n_out if n_out > 0 else 0.0
    if n_in > 0:
        w = alpha * t + (1.0 - alpha) * (1.0 - t)
        g[ins] += ((1.0 - smoothing) * w * dnll / W + smoothing * dhat / n_in)[ins]
    return g.reshape(shape)


def bce_smooth_sums(p, t, lo=SMOOTH_EPS, hi=None):
    """T, sum t log pc, sum (1 - t) log(1 - pc)."""
    p, t = _f64(p), _f64(t)
    pc = np.clip(p, lo, 1.0 - lo if hi is None else hi)
    return np.array([t.sum(), (t * np.log(pc)).sum(), ((1.0 - t) * np.log(1.0 - pc)).sum()], dtype=np.float64)


def bce_smooth_from_sums(sums, n, smooth):
    T, P1, P2 = (float(v) for v in sums)
    with np.errstate(invalid="ignore", divide="ignore"):
        a = np.float64(1.0) - np.float64(T) / np.float64(n)
    alpha = float(a) if np.isnan(a) else min(max(float(a), 0.3), 0.7)
    W = alpha * T + (1.0 - alpha) * (n - T)
    with np.errstate(invalid="ignore", divide="ignore"):
        loss = np.float64(-smooth * (alpha * P1 + (1.0 - alpha) * P2)) / np.float64(W)
    return float(loss), alpha, W


def bce_smooth(p, t, smooth, lo=SMOOTH_EPS, hi=None):
    return bce_smooth_from_sums(bce_smooth_sums(p, t, lo, hi), _f64(p).size, smooth)[0]


def bce_smooth_grad(p, t, smooth, lo=SMOOTH_EPS, hi=None):
    shape = np.shape(p)
    p, t = _f64(p), _f64(t)
    hi = 1.0 - lo if hi is None else hi
    _, alpha, W = bce_smooth_from_sums(bce_smooth_sums(p, t, lo, hi), p.size, smooth)
    w = alpha * t + (1.0 - alpha) * (1.0 - t)
    live = (p >= lo) & (p <= hi)
    pc = np.clip(p, lo, hi)
    return np.where(live, -smooth * w * (t / pc - (1.0 - t) / (1.0 - pc)) / W, 0.0).reshape(shape)


def torch_bce_smooth(probs, targets, smooth, eps=1e-6):
    """BinaryCrossEntropySmooth.__call__ (dram/metrics.py:60-72) transcribed for torch tensors of any float dtype: the
    yardstick of bce_smooth above in fp64, and torch's own fp32 evaluation in the GPU tests."""
    p, t = probs.reshape(-1), targets.reshape(-1).to(probs.dtype)
    alpha = (1.0 - t.sum() / t.shape[0]).clamp(0.3, 0.7)
    p = p.clamp(eps, 1.0 - eps)
    w = alpha * t + (1.0 - alpha) * (1.0 - t)
    return (-smooth * (torch.log(p) * t + torch.log(1.0 - p) * (1.0 - t)) * w).sum() / w.sum()
