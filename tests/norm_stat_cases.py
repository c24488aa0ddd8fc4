"""Cases, inputs and float64 references for the per-op norm statistic kernels of csrc/norm.hip (host only: torch on the CPU).

dram_norm_fwd_train / dram_bn_fwd_eval / dram_norm_bwd / dram_bn_stats / dram_bn_bwd_sums / dram_bn_bwd_apply_sums run, between
their row kernels, a handful of small kernels that turn per (row, chunk) partials into statistics and per-row coefficients:
norm_finalize, bn_stats_finalize, row_sum_chunks, bn_bwd_finalize, gn_bwd_finalize_rows, gn_bwd_finalize_params, bn_bwd_sums,
bn_pqr_from_sums, bn_eval_coef.  CASES takes each of them past one lap of its 256-thread loop and past one block.

Three things live here, shared by tests/test_norm_stats_cpu.py and tests/test_gpu_norm_stats.py:
  * the inputs: every (row, chunk) work item carries an offset of its own, so that a lost, doubled or mis-weighted item moves
    the statistic it belongs to (asserted on the CPU for every case);
  * the reference: plain float64 from the float32 inputs, restated from the definitions of BatchNorm / GroupNorm (+ReLU);
  * mutated references: the same statistics with one work item left out, counted twice, ... -- what a finalizer that loses a
    lap or a block would produce, written as weights on the float64 per-item moments."""
from collections import namedtuple
from functools import lru_cache

import numpy as np
import torch

BATCH, GROUP = 0, 1       # DRAM_NORM_BATCH / DRAM_NORM_GROUP (include/dram_hip.h)
CHUNK = 4096              # floats per (row, chunk) work item of the row kernels
EPS = float(np.float32(1e-5))
MOMENTUM = float(np.float32(0.1))
TOL = 1e-4                # tests/test_gpu_parity.py TOL: what the norm modules are held to
U = 2.0 ** -24

Case = namedtuple("Case", "id kind G N C S")
CASES = [
    # 300 items per statistic, one chunk each, scalar rows; 900 rows: 4 blocks of row_sum_chunks and bn_eval_coef
    Case("bn_n300", BATCH, 1, 300, 3, 97),
    # 350 items per statistic, member/chunk decode (it / 5, it % 5), last chunk of 100, 16-byte rows
    Case("bn_n70_5ch_vec", BATCH, 1, 70, 2, 4 * CHUNK + 100),
    # the same through the scalar row kernels
    Case("bn_n70_5ch_odd", BATCH, 1, 70, 2, 4 * CHUNK + 101),
    # 3 blocks of the 64-thread finalizers, the last with 2 live threads; 260 rows
    Case("bn_c130", BATCH, 1, 2, 130, 132),
    # 300 members: second lap of the rowcoef loop; 5 blocks of gn_bwd_finalize_params
    Case("gn_g1_c300", GROUP, 1, 2, 300, 97),
    # 360 items decoded over members and chunks (it / 9, it % 9), ragged last chunk of 36
    Case("gn_g1_c40_9ch", GROUP, 1, 1, 40, 8 * CHUNK + 36),
    # 99 statistics: 2 blocks of gn_bwd_finalize_rows, cpg = 2
    Case("gn_g33_stats99", GROUP, 33, 3, 66, 260),
    # 270 statistics and 270 rows, cpg = 1
    Case("gn_gC_stats270", GROUP, 90, 3, 90, 64),
    # total == 1: the `unb = var` branch; rstd = 1/sqrt(eps)
    Case("bn_one_value", BATCH, 1, 1, 2, 1),
]
CASE = {c.id: c for c in CASES}
BATCH_IDS = [c.id for c in CASES if c.kind == BATCH]
assert max(c.N * c.C * c.S for c in CASES) < 2.4e6


def nchunks(S):
    return -(-S // CHUNK)


def chunk_lens(S):
    return [min(CHUNK, S - k * CHUNK) for k in range(nchunks(S))]


def gen(seed):
    return torch.Generator().manual_seed(seed)


class Layout:
    """Index tables of a case: rows are (n, c) in memory order; a statistic is a channel (BatchNorm) or a (sample, group)."""

    def __init__(self, c):
        self.rows, self.nch = c.N * c.C, nchunks(c.S)
        r = torch.arange(self.rows)
        self.chan, self.sample = r % c.C, r // c.C
        cpg = c.C // c.G
        if c.kind == BATCH:
            self.nstat, self.members = c.C, c.N
            self.stat, self.member = self.chan, self.sample
        else:
            self.nstat, self.members = c.N * c.G, cpg
            self.stat, self.member = self.sample * c.G + self.chan // cpg, self.chan % cpg
        self.count = float(self.members) * float(c.S)
        # position of item (row, chunk) in the finalize kernels' `it` order of its statistic
        self.it = self.member[:, None] * self.nch + torch.arange(self.nch)[None, :]

    def per_stat(self, per_row):
        return torch.zeros(self.nstat, dtype=torch.float64).index_add_(0, self.stat, per_row)

    def per_chan(self, per_row, C):
        return torch.zeros(C, dtype=torch.float64).index_add_(0, self.chan, per_row)


@lru_cache(maxsize=None)
def layout(case_id):
    return Layout(CASE[case_id])


# ------------------------------------------------------------------------------------------------------------ inputs
# Offsets: |offset| runs over a grid of distinct values on [OFF_LO, OFF_HI], one per (row, chunk), in a fixed random order.  Two
# things are arranged so that the sensitivity condition of tests/test_norm_stats_cpu.py holds (that file asserts it):
#   * the grid leaves out (-OFF_LO, OFF_LO): an item whose mean sat at 0 could be lost without moving a sum;
#   * the items of a ragged last chunk (100, 101 or 36 elements against 4096) take the largest magnitudes, and inside every
#     statistic the signs alternate along a random order of its items, so that the full chunks nearly cancel in a per-channel
#     sum and the short ones stay visible in it.
OFF_LO, OFF_HI = 2.0, 8.0


def item_offsets(c, seed):
    L = layout(c.id)
    g = gen(seed)
    items = L.rows * L.nch
    ragged = torch.zeros(L.rows, L.nch, dtype=torch.bool)
    if L.nch > 1 and c.S % CHUNK:
        ragged[:, -1] = True
    order = torch.randperm(items, generator=g)
    order = torch.cat([order[~ragged.view(-1)[order]], order[ragged.view(-1)[order]]])      # ragged items last
    mag = torch.empty(items, dtype=torch.float64)
    mag[order] = torch.linspace(OFF_LO, OFF_HI, items, dtype=torch.float64) if items > 1 else torch.tensor([OFF_HI])
    sign = torch.empty(items, dtype=torch.float64)
    stat_of_item = L.stat[:, None].expand(L.rows, L.nch).reshape(-1)
    for s in range(L.nstat):
        mine = torch.nonzero(stat_of_item == s).view(-1)
        mine = mine[torch.randperm(len(mine), generator=g)]
        pm = torch.tensor([1.0, -1.0] if s % 2 == 0 else [-1.0, 1.0], dtype=torch.float64)
        sign[mine] = pm.repeat(len(mine) // 2 + 1)[:len(mine)]
    return (mag * sign).view(L.rows, L.nch)


def with_offsets(c, seed):
    L = layout(c.id)
    t = torch.randn(L.rows, c.S, generator=gen(seed), dtype=torch.float32).double()
    off = item_offsets(c, seed + 1)
    t += off.repeat_interleave(torch.tensor(chunk_lens(c.S)), dim=1)
    return t.float().view(c.N, c.C, c.S)


@lru_cache(maxsize=None)
def inputs(case_id):
    """float32 tensors: x, dy [N, C, S]; gamma (non-zero, both signs), beta, running mean / variance, distinct per channel."""
    c = CASE[case_id]
    seed = 1000 + 10 * [k.id for k in CASES].index(case_id)
    ch = torch.arange(c.C, dtype=torch.float64)
    gamma = torch.where(ch % 2 == 0, 1.0, -1.0) * (0.5 + ch / c.C)
    I = {
        "x": with_offsets(c, seed), "dy": with_offsets(c, seed + 2),
        "gamma": gamma.float(),
        "beta": torch.linspace(-0.7, 0.9, c.C),
        "running_mean": torch.linspace(-0.6, 0.8, c.C),
        "running_var": torch.linspace(2.0, 3.5, c.C),
    }
    if c.S > 1:
        move_off_the_relu_threshold(c, I)
    return I


def move_off_the_relu_threshold(c, I):
    """Among 2.3 M elements a few have a pre-activation gamma * xhat + beta within fp32 rounding of 0, where the kernels' fp32
    mask and the reference's float64 one may differ and dx of that element with them.  Such elements (training statistics, and
    running statistics for BatchNorm) are moved by 1/64 until none is left within 64 * 2^-24 of the magnitudes involved:
    tests/test_norm_stats_cpu.py asserts 16 * 2^-24 with mask_margin below."""
    L = layout(c.id)
    gamma, beta = I["gamma"].double()[L.chan][:, None], I["beta"].double()[L.chan][:, None]
    x32 = I["x"].view(L.rows, c.S)
    for _ in range(8):
        x = x32.double()
        mean = (L.per_stat(x.sum(1)) / L.count)[L.stat][:, None]
        rstd = (1.0 / torch.sqrt(L.per_stat(((x - mean) ** 2).sum(1)) / L.count + EPS))[L.stat][:, None]
        stats = [(mean, rstd)]
        if c.kind == BATCH:
            stats.append((I["running_mean"].double()[L.chan][:, None],
                          (1.0 / torch.sqrt(I["running_var"].double() + EPS))[L.chan][:, None]))
        close = torch.zeros_like(x, dtype=torch.bool)
        for m, r in stats:
            a = gamma * r
            close |= (a * (x - m) + beta).abs() < 64 * U * ((a * x).abs() + beta.abs() + (m * a).abs())
        if not bool(close.any()):
            return
        x32[close] += 1.0 / 64
    raise AssertionError(f"{c.id}: elements stay at the ReLU threshold")


def rows64(case_id, name):
    c = CASE[case_id]
    return inputs(case_id)[name].double().view(c.N * c.C, c.S)


# --------------------------------------------------------------------------------------------------------- reference
@lru_cache(maxsize=None)
def forward_ref(case_id):
    """Training-mode forward in float64.  Statistics two-pass (mean, then squared deviations); y from gamma * xhat + beta."""
    c, L, I = CASE[case_id], layout(case_id), inputs(case_id)
    x = rows64(case_id, "x")
    gamma, beta = I["gamma"].double()[L.chan], I["beta"].double()[L.chan]
    mean = L.per_stat(x.sum(1)) / L.count
    dev = x - mean[L.stat][:, None]
    m2 = L.per_stat((dev * dev).sum(1))
    var = m2 / L.count
    rstd = 1.0 / torch.sqrt(var + EPS)
    xhat = dev * rstd[L.stat][:, None]
    a = gamma * rstd[L.stat]
    out = {
        "save_mean": mean, "save_rstd": rstd, "m2": m2,
        "rowcoef": torch.stack([a, beta - mean[L.stat] * a], 1),
        "xhat": xhat, "pre": gamma[:, None] * xhat + beta[:, None],
        "sum_abs_over_count": L.per_stat(x.abs().sum(1)) / L.count,
    }
    if c.kind == BATCH:
        unb = m2 / (L.count - 1.0) if L.count > 1.0 else var
        out["running_mean"] = (1.0 - MOMENTUM) * I["running_mean"].double() + MOMENTUM * mean
        out["running_var"] = (1.0 - MOMENTUM) * I["running_var"].double() + MOMENTUM * unb
    return out


def y_of(pre, relu):
    return pre.clamp_min(0.0) if relu else pre


def _backward(case_id, relu, xhat, pre, rstd_row, batch_stats):
    c, L, I = CASE[case_id], layout(case_id), inputs(case_id)
    d = rows64(case_id, "dy")
    if relu:
        d = d * (pre > 0)
    gamma = I["gamma"].double()[L.chan]
    s1, s2 = d.sum(1), (d * xhat).sum(1)
    out = {"dbeta": L.per_chan(s1, c.C), "dgamma": L.per_chan(s2, c.C)}
    if batch_stats:
        A, B = L.per_stat(gamma * s1) / L.count, L.per_stat(gamma * s2) / L.count
        out["dx"] = rstd_row[:, None] * (gamma[:, None] * d - A[L.stat][:, None] - xhat * B[L.stat][:, None])
    else:
        out["dx"] = (gamma * rstd_row)[:, None] * d
    return out


@lru_cache(maxsize=None)
def backward_ref(case_id, relu):
    """dx, dgamma, dbeta of norm (+ReLU, mask a*x + b > 0) for the gradient dy, training statistics."""
    f, L = forward_ref(case_id), layout(case_id)
    return _backward(case_id, relu, f["xhat"], f["pre"], f["save_rstd"][L.stat], True)


@lru_cache(maxsize=None)
def eval_ref(case_id, relu):
    """Eval-mode BatchNorm (running statistics) forward and backward in float64."""
    c, L, I = CASE[case_id], layout(case_id), inputs(case_id)
    assert c.kind == BATCH
    gamma, beta = I["gamma"].double()[L.chan], I["beta"].double()[L.chan]
    mean, rstd = I["running_mean"].double(), 1.0 / torch.sqrt(I["running_var"].double() + EPS)
    xhat = (rows64(case_id, "x") - mean[L.chan][:, None]) * rstd[L.chan][:, None]
    pre = gamma[:, None] * xhat + beta[:, None]
    a = gamma * rstd[L.chan]
    out = _backward(case_id, relu, xhat, pre, rstd[L.chan], False)
    out.update({"save_mean": mean, "save_rstd": rstd, "rowcoef": torch.stack([a, beta - mean[L.chan] * a], 1), "pre": pre})
    return out


def mask_margin(case_id, pre, mean_row, a):
    """min over the elements of |pre| / (|a*x| + |beta| + |mean*a|): how far, in units of the magnitudes that enter
    fmaf(a, x, b) with b = beta - mean*a, the nearest pre-activation is from the ReLU threshold."""
    L, I = layout(case_id), inputs(case_id)
    x = rows64(case_id, "x")
    scale = (a[:, None] * x).abs() + (I["beta"].double()[L.chan].abs() + (mean_row * a).abs())[:, None]
    return (pre.abs() / scale).min().item()


# ------------------------------------------------------------------------------------------- the bound on a float32 mean
# row_moments_kernel forms a chunk's mean in fp32.  Longest chain of roundings a term passes through:
#   scalar instantiation: a thread accumulates s += v[q] over q = 0..31 with element q * 256 + thread, but a chunk has at most
#     CHUNK = 4096 elements, so only q = 0..15 can hold a value and the other sixteen add an exact 0.f: 16 roundings; then 6
#     levels of the 64-lane butterfly, 3 additions of the 4 wave sums, 1 division by len        -> 16 + 6 + 3 + 1 = 26
#   16-byte instantiation: per float4 two levels of (v0 + v1) + (v2 + v3) and one s +=, four float4 per thread -> 12, then the
#     same 6 + 3 + 1                                                                             -> 22
# The larger one holds for both: k = 26.  Each rounding is at most U = 2^-24 of a partial sum that is itself <= sum |x| of the
# chunk, so |mean_chunk - exact| <= ((1 + U)^26 - 1) * sum |x_chunk| / len.  The finalize kernels weight the chunk means by
# len / M and add them in fp64 (M = elements per statistic), which turns the right-hand sides into 26 U * sum |x| / M; the result
# is rounded to fp32 once (U * |ref|).  One spare U holds (1 + U)^26 - 1 - 26 U, the fp64 additions and U * (|got| - |ref|):
#       |got - ref| <= (26 + 1) * U * sum |x| / M + U * |ref|
K_MEAN = CHUNK // 256 + 6 + 3 + 1
assert K_MEAN == 26


def mean_bound(sum_abs_over_count, ref):
    """Elementwise bound on |got - ref| of save_mean / dram_bn_stats' mean; both arguments float64 tensors."""
    return (K_MEAN + 1) * U * sum_abs_over_count + U * ref.abs()


# ------------------------------------------------------------------------------------------------- mutated references
@lru_cache(maxsize=None)
def item_tables(case_id):
    """float64 per (row, chunk): length, mean and M2 of x; {sum dy, sum dy * xhat} (no ReLU, true statistics)."""
    c, L, f = CASE[case_id], layout(case_id), forward_ref(case_id)
    x, d = rows64(case_id, "x"), rows64(case_id, "dy")
    lens = torch.tensor(chunk_lens(c.S), dtype=torch.float64)
    T = {k: torch.empty(L.rows, L.nch, dtype=torch.float64) for k in ("mean", "m2", "s1", "s2")}
    for k in range(L.nch):
        sl = slice(k * CHUNK, min(c.S, (k + 1) * CHUNK))
        T["mean"][:, k] = x[:, sl].mean(1)
        T["m2"][:, k] = ((x[:, sl] - T["mean"][:, k:k + 1]) ** 2).sum(1)
        T["s1"][:, k] = d[:, sl].sum(1)
        T["s2"][:, k] = (d[:, sl] * f["xhat"][:, sl]).sum(1)
    T["len"] = lens
    return T


FWD_MUTATIONS = ["drop_item", "double_item", "ragged_as_full", "items_from_256", "rowcoef_from_256", "gamma_at_row"]
BWD_MUTATIONS = ["drop_item", "double_item", "rows_from_256", "channels_from_64"]


def applies(case_id, side, mutation):
    """Whether the mutation changes anything for the case (a table row with 40 members has no member 256)."""
    c, L = CASE[case_id], layout(case_id)
    if side == "fwd":
        return {"drop_item": True, "double_item": True, "ragged_as_full": c.S % CHUNK != 0,
                "items_from_256": L.members * L.nch > 256, "rowcoef_from_256": L.members > 256,
                "gamma_at_row": c.N > 1}[mutation]
    return {"drop_item": True, "double_item": True, "rows_from_256": L.rows > 256, "channels_from_64": c.C > 64}[mutation]


def forward_small(case_id, mutation=None, item=None):
    """The small outputs of the training forward, combined from the per-item moments the way the definition of a pooled mean
    and M2 says (Chan); `mutation` (FWD_MUTATIONS) applied, `item` = (row, chunk) for drop_item / double_item.  The element
    count of a statistic stays what it is: a kernel that loses an item still divides by members * S."""
    c, L, I, T = CASE[case_id], layout(case_id), inputs(case_id), item_tables(case_id)
    w = torch.ones(L.rows, L.nch, dtype=torch.float64)
    lens = T["len"].clone()
    if mutation == "drop_item":
        w[item] = 0.0
    elif mutation == "double_item":
        w[item] = 2.0
    elif mutation == "ragged_as_full":
        lens[-1] = CHUNK
    elif mutation == "items_from_256":
        w[L.it >= 256] = 0.0
    mean = L.per_stat((w * lens * T["mean"]).sum(1)) / L.count
    dm = T["mean"] - mean[L.stat][:, None]
    m2 = L.per_stat((w * (T["m2"] + lens * dm * dm)).sum(1))
    var = m2 / L.count
    rstd = 1.0 / torch.sqrt(var + EPS)
    gi = torch.arange(L.rows).clamp_max(c.C - 1) if mutation == "gamma_at_row" else L.chan   # past gamma's end: its last value
    a = I["gamma"].double()[gi] * rstd[L.stat]
    coef = torch.stack([a, I["beta"].double()[L.chan] - mean[L.stat] * a], 1)
    if mutation == "rowcoef_from_256":
        coef[L.member >= 256] = 0.0
    out = {"save_mean": mean, "save_rstd": rstd, "rowcoef": coef}
    if c.kind == BATCH:
        unb = m2 / (L.count - 1.0) if L.count > 1.0 else var
        out["running_mean"] = (1.0 - MOMENTUM) * I["running_mean"].double() + MOMENTUM * mean
        out["running_var"] = (1.0 - MOMENTUM) * I["running_var"].double() + MOMENTUM * unb
        out["stats_mean"], out["stats_m2"] = mean, m2
    return out


def backward_small(case_id, mutation=None, item=None):
    """dgamma / dbeta without ReLU from the per-item sums (under ReLU a masked item contributes nothing, and nothing could
    notice its loss); `mutation` from BWD_MUTATIONS."""
    c, L, T = CASE[case_id], layout(case_id), item_tables(case_id)
    w = torch.ones(L.rows, L.nch, dtype=torch.float64)
    if mutation == "drop_item":
        w[item] = 0.0
    elif mutation == "double_item":
        w[item] = 2.0
    r1, r2 = (w * T["s1"]).sum(1), (w * T["s2"]).sum(1)
    if mutation == "rows_from_256":
        r1[256:], r2[256:] = 0.0, 0.0
    out = {"dbeta": L.per_chan(r1, c.C), "dgamma": L.per_chan(r2, c.C)}
    if mutation == "channels_from_64":
        out["dbeta"][64:], out["dgamma"][64:] = 0.0, 0.0
    return out


def tolerance_of(case_id, name, ref):
    """The tolerance output `name` is held to on the GPU, as a fraction of max |ref| (the measure of test_gpu_parity.check)."""
    if name in ("save_mean", "stats_mean"):
        f = forward_ref(case_id)
        return (mean_bound(f["sum_abs_over_count"], f["save_mean"]).max() / ref.abs().max().clamp_min(1e-30)).item()
    return TOL


def movement(case_id, mutated, true):
    """max over the outputs of (max |mutated - true| / max |true|) / tolerance: how many tolerances the mutation is away."""
    worst = 0.0
    for name, ref in true.items():
        moved = ((mutated[name] - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()
        worst = max(worst, moved / tolerance_of(case_id, name, ref))
    return worst
