"""numpy restatement of global-norm gradient clipping (torch.nn.utils.clip_grad_norm_) as csrc/optim.hip evaluates it, and
the bound on what the device's norm may differ from it by.

Definitions, over all gradient elements g_i of all tensors together:
  total_norm = sqrt(sum g_i^2)  (kind 2)   or   max |g_i|, NaN if any g_i is  (kind inf)
  clip_coef  = min(1, max_norm / (total_norm + 1e-6)), a NaN kept (torch.clamp(max=1) keeps it)
  g_i       <- clip_coef g_i
tests/test_clip_cpu.py holds these against torch's own function in fp64.

`total_norm` evaluates the norm from fp32 gradients with every square exact in fp64 (the product of two fp32 numbers has at
most 48 significant bits) and the sum by math.fsum, which rounds the exact sum once.  `clip_coef` evaluates the coefficient
from a given norm in the number format asked for: in np.float32 its three operations (one sum, one quotient, one comparison)
are the three IEEE fp32 operations the finishing kernel performs, so the device's coefficient must equal it BIT FOR BIT when
it is fed the device's own norm.

Bound on the norm (NORM_BOUND_DERIVATION).  The device adds the exact squares in fp64, N elements into B per-block partials
and the B partials into one sum: N + B additions at most (those inside a block by lane, by wave shuffle and over four LDS
words; their order is fixed but does not enter the bound).  Every term is >= 0, so every intermediate sum is <= the exact
total S, and each addition errs by at most 2^-53 of its own result:  |S' - S| <= (N + B) 2^-53 S  (first order; the dropped
second-order terms are (N + B)^2 2^-106 S, below 2^-53 S for N + B < 2^26, and one more 2^-53 is added for them).
sqrt(S (1 + d)) = sqrt(S) (1 + d / 2 + ...): half of that carries onto the root.  The fp64 root rounds once (2^-53), the
restatement's own sum and root twice more (2 x 2^-53), and the cast to fp32 once (u = 2^-24 of the result, or 2^-149 absolute
where the result is subnormal):
    |norm_device - norm| <= norm (u (1 + 2^-10) + ((N + B) / 2 + 4) 2^-53) + 2^-149.
Squares of 1e20 (1e40 < 1.8e308) do not overflow and squares of 1e-30 (1e-60 > 2.2e-308) do not vanish, so the bound holds
for them unchanged.  A norm above the largest fp32 number becomes +inf on both sides.  The inf-norm is exact: max |g_i| is one
of the inputs.

The update needs no bound of its own: the kernels' scaled gradient is the single IEEE product np.float32(c) * g, which the
tests feed to optim_restatement.AdamRun / SgdRun with c read back from the device, under that file's bound.
"""
import math

import numpy as np

U = 2.0 ** -24
UE = U * (1.0 + 2.0 ** -10)
OCHUNK = 4096                     # elements per block of csrc/optim.hip
KINDS = {2.0: 2, math.inf: 0}     # norm_type -> DRAM_OPTIM_NORM_2 / DRAM_OPTIM_NORM_INF of include/dram_hip.h


def partial_count(sizes):
    """Blocks (= partials) the norm kernel takes over tensors of these element counts."""
    return sum((int(n) + OCHUNK - 1) // OCHUNK for n in sizes)


def total_norm(grads, norm_type):
    """fp64 norm over all elements of the arrays `grads` (any float dtype; fp32 inputs give exact squares)."""
    flat = [np.asarray(g, dtype=np.float64).reshape(-1) for g in grads]
    flat = np.concatenate(flat) if flat else np.zeros(0)
    if float(norm_type) == math.inf:
        if flat.size == 0:
            return 0.0
        return float("nan") if np.isnan(flat).any() else float(np.abs(flat).max())
    assert float(norm_type) == 2.0
    with np.errstate(over="ignore", invalid="ignore"):
        sq = flat * flat
    if not np.isfinite(sq).all():
        return float("nan") if np.isnan(sq).any() else float("inf")
    return math.sqrt(math.fsum(sq.tolist()))


def clip_coef(norm, max_norm, dtype=np.float32):
    """min(1, max_norm / (norm + 1e-6)) with each operation rounded to `dtype`; NaN stays NaN."""
    t = dtype
    with np.errstate(all="ignore"):
        c = t(max_norm) / (t(norm) + t(1e-6))
    return t(1.0) if c > t(1.0) else c


def clipped(grads, max_norm, norm_type):
    """(norm, coefficient, scaled gradients) in fp64."""
    norm = total_norm(grads, norm_type)
    c = clip_coef(norm, max_norm, np.float64)
    return norm, c, [np.asarray(g, dtype=np.float64) * c for g in grads]


def norm_bound(norm, sizes, norm_type):
    """Absolute bound on |fp32 device norm - norm| for a finite `norm` over tensors of `sizes` elements."""
    if float(norm_type) == math.inf:
        return 0.0
    n, b = sum(int(s) for s in sizes), partial_count(sizes)
    return abs(norm) * (UE + (0.5 * (n + b) + 4.0) * 2.0 ** -53) + 2.0 ** -149


def norm_within(got, want, sizes, norm_type):
    """Whether the fp32 device norm `got` is the fp64 norm `want` within the bound; non-finite values must match in kind."""
    got, want = float(got), float(want)
    if math.isnan(want):
        return math.isnan(got)
    if want > float(np.finfo(np.float32).max):
        return got == math.inf or got == float(np.finfo(np.float32).max)
    return abs(got - want) <= norm_bound(want, sizes, norm_type)


def torch_fp32_norm_bound(norm, sizes):
    """Bound for torch's OWN fp32 evaluation of the 2-norm (per tensor a norm, then the norm of those norms), which
    tests/test_clip_cpu.py holds it to.  Per level over n terms: every square rounds once (u on the sum of non-negative terms),
    the fp32 sum is a cascade / pairwise one of depth <= ceil(log2 n) + 3 (the +3 for the vector lanes and unrolled
    accumulators it starts from), u per level of depth; half of both carries onto the root, which rounds once:
    ((1 + ceil(log2 n) + 3) / 2 + 1) u.  The two levels chain, their relative errors add.  For 4099 elements in 5 tensors that
    is 9.5 u + 5 u: a few ulps, where the fp64-accumulating kernel is held to ONE."""
    def level(n):
        return (1 + math.ceil(math.log2(max(n, 2))) + 3) / 2.0 + 1.0
    return abs(norm) * UE * (level(max(sizes)) + level(len(sizes)))
