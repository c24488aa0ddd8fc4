"""The SegOverlap loss of include/dram_hip.h (per-sample Tversky + focal on logits, target given) restated in numpy fp64
from the header's text, its closed-form gradient, and the same formula in torch (for autograd, on any device and dtype).
A plain module: tests/test_seg_overlap_cpu.py pins the gradient to torch's autograd, the GPU tests hold the kernels to it.

z: [N, ...] logits; t, voi: the same shape, "set" means non-zero; voi None: every voxel."""
import numpy as np
import torch


def _flat(z, t, voi):
    z = np.asarray(z, dtype=np.float64)
    N = z.shape[0]
    z = z.reshape(N, -1)
    t = np.asarray(t).reshape(N, -1) != 0
    v = np.ones_like(t) if voi is None else np.asarray(voi).reshape(N, -1) != 0
    return z, t, v


def softplus(x):
    return np.logaddexp(0.0, x)


def voxel_terms(z, t, alpha, gamma):
    """p, q = 1 - p (both to full relative accuracy), the focal term -alpha_t (1 - p_t)^gamma log p_t and the argument
    x = -gamma log(1 - p_t) >= 0 of its exponential, for every voxel (the voi is not applied here)."""
    p, q = np.exp(-softplus(-z)), np.exp(-softplus(z))
    nlp = np.where(t, softplus(-z), softplus(z))           # -log p_t
    nlq = np.where(t, softplus(z), softplus(-z))           # -log(1 - p_t)
    x = gamma * nlq
    f = np.where(t, alpha, 1.0 - alpha) * np.exp(-x) * nlp
    return p, q, f, x


def totals(z, t, voi=None, alpha=0.5, gamma=2.0):
    """[N, 5]: TP, SP, ST, M and the sum of the focal terms of every sample."""
    z, t, v = _flat(z, t, voi)
    p, _, f, _ = voxel_terms(z, t, alpha, gamma)
    cols = [np.where(v & t, p, 0.0), np.where(v, p, 0.0), (v & t).astype(np.float64), v.astype(np.float64), np.where(v, f, 0.0)]
    return np.stack([c.sum(-1) for c in cols], -1)


def sample_terms(tot, a, b, s):
    """(1 - TI_n, F_n) of every sample from its totals; an empty volume of interest gives (0, 0)."""
    TP, SP, ST, M, FS = (tot[:, k] for k in range(5))
    ti = (TP + s) / ((1.0 - a - b) * TP + a * SP + b * ST + s)
    return np.where(M > 0, 1.0 - ti, 0.0), np.where(M > 0, FS / np.maximum(M, 1.0), 0.0)


def seg_overlap(z, t, voi=None, a=0.5, b=0.5, s=1.0, alpha=0.5, gamma=2.0):
    """out[2] = (sum_n (1 - TI_n), mean_n F_n)."""
    one_minus_ti, F = sample_terms(totals(z, t, voi, alpha, gamma), a, b, s)
    return np.array([one_minus_ti.sum(), F.sum() / max(len(F), 1)])


def tversky_coefficients(tot, a, b, s):
    """d(1 - TI_n) / dz_v = p q c with c = c_set where t is set and c_unset elsewhere: ([N] c_set, [N] c_unset)."""
    TP, SP, ST = tot[:, 0], tot[:, 1], tot[:, 2]
    num, den = TP + s, (1.0 - a - b) * TP + a * SP + b * ST + s
    return -(den - num * (1.0 - b)) / den ** 2, num * a / den ** 2


def seg_overlap_grad_parts(z, t, voi=None, a=0.5, b=0.5, s=1.0, alpha=0.5, gamma=2.0):
    """(d out[0] / dz, d out[1] / dz, x) in closed form, each of z's shape and 0 outside the volume of interest; x is the
    argument of the focal term's exponential (voxel_terms)."""
    shape = np.shape(z)
    z, t, v = _flat(z, t, voi)
    N = z.shape[0]
    tot = totals(z, t, v, alpha, gamma)
    p, q, _, x = voxel_terms(z, t, alpha, gamma)
    cs, cu = tversky_coefficients(tot, a, b, s)
    d0 = np.where(v, p * q * np.where(t, cs[:, None], cu[:, None]), 0.0)
    nlp = np.where(t, softplus(-z), softplus(z))
    pt, qt = np.where(t, p, q), np.where(t, q, p)          # p_t, 1 - p_t
    dfu = np.where(t, alpha, 1.0 - alpha) * np.exp(-x) * (gamma * pt * nlp + qt)
    M = tot[:, 3]
    cf = np.where(M > 0, 1.0 / (N * np.maximum(M, 1.0)), 0.0)
    d1 = np.where(v, np.where(t, -dfu, dfu) * cf[:, None], 0.0)
    return d0.reshape(shape), d1.reshape(shape), x.reshape(shape)


def seg_overlap_grad(z, t, voi=None, a=0.5, b=0.5, s=1.0, alpha=0.5, gamma=2.0, gout=(1.0, 1.0)):
    d0, d1, _ = seg_overlap_grad_parts(z, t, voi, a, b, s, alpha, gamma)
    return gout[0] * d0 + gout[1] * d1


def torch_seg_overlap(z, t, voi=None, a=0.5, b=0.5, s=1.0, alpha=0.5, gamma=2.0):
    """The definition in torch ops, in z's dtype and on its device: a [2] tensor, differentiable in z."""
    sp = lambda x: torch.logaddexp(torch.zeros_like(x), x)       # (F.softplus switches to the identity above 20)
    N = z.shape[0]
    z = z.reshape(N, -1)
    t = (t.reshape(N, -1) != 0).to(z.dtype)
    v = torch.ones_like(t) if voi is None else (voi.reshape(N, -1) != 0).to(z.dtype)
    logp, logq = -sp(-z), -sp(z)
    p = torch.exp(logp)
    TP, SP, ST, M = (p * t * v).sum(-1), (p * v).sum(-1), (t * v).sum(-1), v.sum(-1)
    ti = (TP + s) / ((1.0 - a - b) * TP + a * SP + b * ST + s)
    foc = -(t * alpha * torch.exp(gamma * logq) * logp + (1.0 - t) * (1.0 - alpha) * torch.exp(gamma * logp) * logq)
    Fn = (foc * v).sum(-1) / M.clamp_min(1.0)
    live = (M > 0).to(z.dtype)
    return torch.stack([((1.0 - ti) * live).sum(), (Fn * live).sum() / N])
