"""Host-side references for tests/test_gpu_onload.py (the fused engine's normalise-on-load kernels and the producers of
their per-row coefficients {a, b}); torch on the CPU in fp64, nothing here touches a device.
tests/test_onload_reference_cpu.py pins the two statistics helpers to torch's own mean / var.

  make_parts / combine   synthetic {mean, M2, count} partials of the layout dram_conv3d_k3_fwd_fused writes
                         (stats[N*C][nparts][3]) and Chan's combine of them in fp64: the reference of
                         dram_norm_finalize_parts and dram_bn_parts_stats
  random_cuts            cut points with empty pieces at the front, in the middle and as a tail
  coef_table             a coefficient table [rows][2] with the rows an on-load consumer can get wrong
  act64                  act(a * x + b) per row, everything widened to fp64
"""
import torch

BATCH, GROUP = 0, 1          # DRAM_NORM_BATCH, DRAM_NORM_GROUP of include/dram_hip.h


def random_cuts(S, nparts, gen):
    """nparts - 1 sorted cut points in [0, S].  From four parts on the first piece, one inner piece and the last piece are
    empty (the zero-filled slots a conv launch leaves when its boxing needs fewer partials than the buffer holds)."""
    cuts = torch.sort(torch.randint(0, S + 1, (nparts - 1,), generator=gen)).values
    if nparts >= 4:
        cuts[0] = 0
        cuts[-1] = S
        cuts[nparts // 2 - 1] = cuts[nparts // 2]
        cuts = torch.sort(cuts).values
    return [int(c) for c in cuts]


def make_parts(y, cuts):
    """y: fp64 [N, C, S]; cuts: sorted cut points in [0, S] (repeats give empty pieces).  Every row is split into
    len(cuts) + 1 pieces; returns float32 [N*C, nparts, 3] = {mean, M2, count} of each piece, computed in fp64 (two-pass)
    and rounded to float32; an empty piece is {0, 0, 0}."""
    assert y.dtype == torch.float64 and y.dim() == 3
    N, C, S = y.shape
    edges = [0] + [int(c) for c in cuts] + [S]
    assert all(a <= b for a, b in zip(edges, edges[1:])), "cut points must be sorted and inside [0, S]"
    rows = y.reshape(N * C, S)
    out = torch.zeros(N * C, len(edges) - 1, 3, dtype=torch.float64)
    for i, (a, b) in enumerate(zip(edges, edges[1:])):
        if b > a:
            piece = rows[:, a:b]
            mean = piece.mean(1)
            out[:, i, 0] = mean
            out[:, i, 1] = ((piece - mean[:, None]) ** 2).sum(1)
            out[:, i, 2] = b - a
    return out.float()


def combine(parts32, kind, G, N, C):
    """Chan's combine, in fp64, of float32 partials [N*C, nparts, 3] over the rows of each statistic (BATCH: statistic c =
    rows (n, c) of every n; GROUP: statistic (n, g) = the C / G rows of the group).  Returns a dict of fp64 vectors with one
    entry per statistic: count, mean, m2, var (biased) and var_unbiased."""
    p = parts32.double().reshape(N, C, -1, 3)
    if kind == BATCH:
        p = p.permute(1, 0, 2, 3).reshape(C, -1, 3)
    else:
        p = p.reshape(N * G, -1, 3)
    mean_i, m2_i, n_i = p[:, :, 0], p[:, :, 1], p[:, :, 2]
    count = n_i.sum(1)
    mean = (n_i * mean_i).sum(1) / count
    m2 = (m2_i + n_i * (mean_i - mean[:, None]) ** 2).sum(1)
    return {"count": count, "mean": mean, "m2": m2, "var": m2 / count, "var_unbiased": m2 / (count - 1.0).clamp_min(1.0)}


def stat_of_row(kind, G, N, C):
    """long [N*C]: the statistic each (n, c) row belongs to."""
    n = torch.arange(N * C) // C
    c = torch.arange(N * C) % C
    return c if kind == BATCH else n * G + c // (C // G)


def norm_reference(parts32, kind, G, N, C, gamma, beta, eps):
    """fp64 reference of dram_norm_finalize_parts: mean, rstd per statistic and rowcoef [N*C, 2] (a = gamma * rstd,
    b = beta - mean * a); gamma / beta: float32 [C] or None."""
    st = combine(parts32, kind, G, N, C)
    rstd = 1.0 / torch.sqrt(st["var"] + float(eps))
    s = stat_of_row(kind, G, N, C)
    c = torch.arange(N * C) % C
    g = gamma.double()[c] if gamma is not None else torch.ones(N * C, dtype=torch.float64)
    bt = beta.double()[c] if beta is not None else torch.zeros(N * C, dtype=torch.float64)
    a = g * rstd[s]
    return st, rstd, torch.stack([a, bt - st["mean"][s] * a], 1)


def coef_table(rows, gen):
    """float32 [rows, 2] = {a, b}, every row different (a in +-[0.5, 1.5], b ~ N(0, 0.5): for N(0, 1) data every such row has
    activated values of both signs), with the special rows written over it afterwards.  Returns (coef, special) with
    special = {name: row}: 'neg' a < 0, 'zero' a == 0 (b > 0), 'dead' a = 0.5 and b = -8 (every activated value of
    N(0, 1) data is negative: all 0 under ReLU; a larger |b| would only widen every max-relative tolerance without ReLU), 'mixed' a > 0 with b == 0.25.  With fewer rows than specials the later ones are
    left out (a table of one row keeps 'neg')."""
    a = (torch.rand(rows, generator=gen) + 0.5) * torch.where(torch.rand(rows, generator=gen) < 0.4, -1.0, 1.0)
    b = torch.randn(rows, generator=gen) * 0.5
    coef = torch.stack([a, b], 1).float()
    special = {}
    for name, row, val in (("neg", 0, (-1.25, 0.375)), ("zero", 1, (0.0, 0.75)), ("dead", 2, (0.5, -8.0)),
                           ("mixed", 3, (0.8125, 0.25))):
        if row < rows:
            coef[row, 0], coef[row, 1] = val
            special[name] = row
    return coef, special


def act64(raw, coef, relu):
    """act(a * x + b) in fp64: raw [rows, ...] float32, coef [rows, 2] float32; the product and the sum are both formed in
    fp64 (a * x is exact there: 24 + 24 significant bits)."""
    shape = (raw.shape[0],) + (1,) * (raw.dim() - 1)
    v = coef[:, 0].double().reshape(shape) * raw.double() + coef[:, 1].double().reshape(shape)
    return v.clamp_min(0.0) if relu else v


# name, kind, G, N, C, S, nparts, one channel at mean 50 / sigma 1.  PARTS_PER_GROUP of csrc/norm.hip is 2048: 2049 and 5000
# parts take two and three first-level groups with a ragged last one; 300 members per statistic are more than the 256
# threads of the block that writes their row coefficients.
STAT_CASES = [
    ("bn_p1", BATCH, 1, 2, 3, 6007, 1, False),
    ("bn_p7", BATCH, 1, 2, 3, 6007, 7, False),
    ("bn_p2048", BATCH, 1, 2, 3, 6007, 2048, False),
    ("bn_p2049", BATCH, 1, 2, 3, 6007, 2049, False),
    ("bn_p5000", BATCH, 1, 2, 3, 6007, 5000, False),
    ("bn_n300", BATCH, 1, 300, 3, 97, 3, False),
    ("gn_g1_c300", GROUP, 1, 1, 300, 97, 3, False),
    ("gn_gC_c6", GROUP, 6, 2, 6, 693, 7, False),
    ("gn_g2_c6", GROUP, 2, 2, 6, 693, 7, False),
    ("bn_mean50", BATCH, 1, 2, 3, 4100, 7, True),
    ("gn_gC_mean50", GROUP, 3, 2, 3, 4100, 7, True),
]


def stat_case_data(case):
    """(y fp64 [N, C, S], cuts) of a STAT_CASES entry: every channel with its own scale in [0.5, 2] and shift in [-1, 1];
    `offset` puts channel 1 at mean 50, sigma 1."""
    name, kind, G, N, C, S, nparts, offset = case
    gen = torch.Generator().manual_seed(1000 + [c[0] for c in STAT_CASES].index(name))
    scale = torch.rand(C, generator=gen, dtype=torch.float64) * 1.5 + 0.5
    shift = torch.rand(C, generator=gen, dtype=torch.float64) * 2.0 - 1.0
    if offset:
        scale[1], shift[1] = 1.0, 50.0
    y = torch.randn(N, C, S, generator=gen, dtype=torch.float64) * scale[None, :, None] + shift[None, :, None]
    return y, random_cuts(S, nparts, gen)


def moments_of(y, kind, G):
    """torch's own fp64 mean / biased / unbiased variance of y [N, C, S] per statistic, in the order `combine` uses."""
    N, C, S = y.shape
    v = y.permute(1, 0, 2).reshape(C, -1) if kind == BATCH else y.reshape(N * G, -1)
    return v.mean(1), v.var(1, unbiased=False), v.var(1, unbiased=True)
