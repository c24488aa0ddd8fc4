"""Cases, inputs, a float64 restatement and comparators for the three fused IntRegRefineLoss kernels of csrc/loss.hip
(loss_partial_kernel, loss_finalize_kernel, loss_bwd_kernel).  Host only: numpy and torch on the CPU.

Shared by tests/test_refine_loss_cases_cpu.py (which holds the restatement against oracle.dram_oracle, re-checks every input
condition and regime claim, and shows that the comparators catch a wrong kernel) and tests/test_gpu_refine_loss_kernels.py.

The restatement takes keep[N], targets[N, 2] and weight[N] as given -- train_step.Batch derives them from the masks, which
ties the hinge and alpha to whatever random masks produce -- so each case chooses its regime.  It is the fused formulation
of oracle.dram_oracle.fused_loss_math with "an empty sum contributes 0" (the comment above loss_finalize_kernel): no outside
voxel -> the outside mean is 0, a sample without a lobe adds nothing to reg, no inside voxel -> alpha = 0, wsum = 1.

Input conditions (asserted by build(), re-checked on the host), under which an fp32 kernel and an fp64 reference take the
same branches:
  * a logit is exactly 0 or has |d| >= 1e-3: sigmoid_pq rounds p to exactly 0.5 for a tiny positive d where fp64 has p > 0.5,
    and the pseudo label [p > 0.5] would differ.  Exact zeros ARE placed, on lesion voxels inside the lobe: both sides have
    p = 0.5, t = 0 and take the 1 - p side of the boot term;
  * no logit with 15.5 < |d| < 17 (ln 1e7 = 16.118: the eps clamp and its zero gradient); saturated voxels have |d| in
    {17, 20, 88, 1e4, FLT_MAX}, all others |d| <= 15.5;
  * the fp64 lobe mean r_n is at least 1e-3 away from both edges of its band, so the fp32 backward and the fp64 forward agree
    on whether the hinge is active;
  * masks hold exactly 0.0 and 1.0; every sample has an inside and an outside voxel except where the case says otherwise.
These are conditions on the inputs, not tolerances."""
from collections import namedtuple
from functools import lru_cache

import numpy as np
import torch

LCHUNK = 8192                     # csrc/loss.hip: elements per forward block
BWD_CAP, BWD_PER_BLOCK = 4096, 2048      # dram_intreg_loss_bwd: blocks per sample at most, elements each before the cap
EPS = 1e-7
SMOOTHING = 0.1
VALUE_TOL = 2e-5                  # |got - ref| <= VALUE_TOL * max(1, |ref|)   (tests/test_gpu_train_step.py)
GRAD_TOL = 1e-4                   # |got - ref| <= GRAD_TOL * max |ref|, here per voxel class
ZERO_MARGIN, LIVE_MAX, SAT_MIN, HINGE_MARGIN = 1e-3, 15.5, 17.0, 1e-3
FLT_MAX = float(np.finfo(np.float32).max)
SAT_VALUES = (17.0, 20.0, 88.0, 1e4, FLT_MAX)
GOUTS = ((2.0, 1.0), (1.0, 0.0), (0.0, 1.0), (-0.37, 3.0))
CLASSES = ("outside", "inside_t1", "inside_t0", "saturated")

Case = namedtuple("Case", "id N S seed lobe les pos sat keep hinge refined gouts shifts empty force scale high_last")


def _case(cid, N, S, seed, lobe=0.5, les=0.8, pos=0.7, sat=(0.0,), keep=(1.0, 0.0, 1.0), hinge=("below", "inside", "above"),
          refined=False, gouts=(GOUTS[0],), shifts=None, empty=(), force=True, scale=2.0, high_last=False):
    return Case(cid, N, S, seed, lobe, les, pos, sat, keep, hinge, refined, gouts, shifts, empty, force, scale, high_last)


_CASES = [
    # ---- shapes, N = 3: blockIdx.y = 0..2.  Forward: one block per LCHUNK of a sample; backward: one per 2048 elements
    _case("s1", 3, 1, 101, force=False),          # one voxel per sample: inside, outside, inside (sample 1 has no lobe)
    _case("s255", 3, 255, 102),                   # one thread idle in the only step of the only block
    _case("s257", 3, 257, 103),                   # a second step with one live thread
    _case("s8191", 3, 8191, 104),                 # one short of a chunk
    _case("s8192", 3, 8192, 105),                 # exactly one chunk
    _case("s8193", 3, 8193, 106),                 # the second chunk holds one element
    _case("s24581", 3, 3 * 8192 + 5, 107),        # three full chunks and a ragged fourth; 13 backward blocks
    # ---- regimes, at S = 8193 (a full chunk and a ragged one)
    _case("alpha_interior", 3, 8193, 111, pos=0.8, les=0.7, keep=(1.0,)),            # T / n_in about 0.56
    _case("alpha_clamped_75", 3, 8193, 112, pos=0.3, les=0.4, keep=(1.0,)),          # about 0.12: alpha = 0.75
    _case("alpha_clamped_25", 3, 8193, 113, pos=0.95, les=0.95, keep=(1.0,)),        # about 0.90: alpha = 0.25
    _case("hinge", 3, 8193, 114, keep=(1.0,), gouts=GOUTS),                          # below / inside / above, every gout
    _case("keep_mixed", 4, 8193, 115, keep=(1.0, 0.0, 0.0, 1.0)),
    _case("keep_none", 3, 8193, 116, keep=(0.0,)),                                   # T = 0, alpha = 0.75, all of the lobe in B
    _case("refined", 3, 8193, 117, refined=True),                                    # a distinct tensor, or the pointer of dense
    _case("refined_absent", 3, 8193, 117),                                           # the same inputs without it (same seed)
    _case("saturation", 4, 8193, 118, sat=(0.9, 0.9, 0.3, 0.05), keep=(1.0, 1.0, 0.0, 1.0), gouts=(GOUTS[0], GOUTS[2]),
          hinge=("below", "above", "inside", "below")),
    # few inside voxels (c_out << the inside coefficients) and few outside voxels (c_out >> them): where one max over the
    # whole tensor cannot see a coefficient of the smaller class
    _case("few_inside", 3, 8193, 119, lobe=0.004, keep=(1.0,)),
    _case("few_outside", 3, 8193, 120, lobe=0.9995, keep=(1.0,), gouts=(GOUTS[2], GOUTS[0])),
    # ---- N = 257: the second lap of `n += 256` in loss_finalize_kernel; sample 256 has an active hinge far from its band
    _case("n257", 257, 37, 121, keep=(1.0, 1.0, 0.0), high_last=True),
    # ---- one past the backward grid cap: block 0 of the sample takes a second lap of its grid-stride loop
    _case("cap", 1, BWD_CAP * BWD_PER_BLOCK + 300, 122, keep=(1.0,), hinge=("below",)),
    # ---- every tensor 1, 2 or 3 floats past a 16-byte boundary
    _case("unaligned", 3, 3 * 8192 + 5, 123, refined=True,
          shifts={"dense": 1, "refined": 2, "lobes": 3, "lesions": 1, "keep": 2, "targets": 3, "weight": 1, "gout": 2, "out": 3,
                  "state": 1, "ddense": 2, "drefined": 3}),
    # ---- edges: an empty sum contributes 0
    _case("no_outside", 3, 8193, 124, lobe=1.0, force=False),
    _case("empty_lobe", 3, 8193, 125, empty=(1,)),
]
CASES = {c.id: c for c in _CASES}
assert len(CASES) == len(_CASES)
SHAPE_CASES = ["s1", "s255", "s257", "s8191", "s8192", "s8193", "s24581"]
REGIME_CASES = ["alpha_interior", "alpha_clamped_75", "alpha_clamped_25", "hinge", "keep_mixed", "keep_none", "saturation",
                "few_inside", "few_outside"]
EDGE_CASES = ["no_outside", "empty_lobe"]
ALPHA_REGIME = {"alpha_interior": "interior", "alpha_clamped_75": 0.75, "alpha_clamped_25": 0.25, "keep_none": 0.75}

Inputs = namedtuple("Inputs", "dense refined lobes lesions keep targets weight")


# ------------------------------------------------------------------------------------------------ inputs
def _logits(rng, N, S, scale, pos, sat):
    """float32 [N, S]: |d| in [1e-3, 15.5] with a share `pos` positive; a share sat[n % len] of sample n is saturated, the
    magnitudes cycling through SAT_VALUES, either sign."""
    mag = np.clip(np.abs(rng.standard_normal((N, S), dtype=np.float32)) * np.float32(scale), ZERO_MARGIN, LIVE_MAX)
    sign = np.where(rng.random((N, S), dtype=np.float32) < pos, 1.0, -1.0)
    d = (mag * sign).astype(np.float32)
    for n in range(N):
        share = sat[n % len(sat)]
        if share > 0.0:
            idx = np.flatnonzero(rng.random(S) < share)
            vals = np.asarray(SAT_VALUES, dtype=np.float32)[np.arange(idx.size) % len(SAT_VALUES)]
            d[n, idx] = vals * np.where(rng.random(idx.size) < 0.5, 1.0, -1.0).astype(np.float32)
    return d


def lobe_mean(dense, lobes):
    """fp64 r_n (NaN for an empty lobe) and nm_n."""
    m = lobes > 0
    nm = m.sum(1).astype(np.float64)
    sp = np.where(m, _sigmoid64(dense.astype(np.float64)), 0.0).sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return sp / nm, nm


def _sigmoid64(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _band(kind, r):
    if kind == "below":         # r below its band
        return r + 0.1, r + 0.2
    if kind == "inside":
        return r - 0.05, r + 0.05
    if kind == "above":
        return r - 0.2, r - 0.1
    raise ValueError(kind)


@lru_cache(maxsize=None)
def build(cid):
    """The inputs of a case (float32 numpy, [N, S]); asserts the input conditions."""
    c = CASES[cid]
    rng = np.random.default_rng(c.seed)
    N, S = c.N, c.S
    lobes = (rng.random((N, S), dtype=np.float32) < c.lobe).astype(np.float32)
    if c.force:
        lobes[:, 0], lobes[:, -1] = 1.0, 0.0
    if S == 1:
        lobes[:, 0] = [1.0, 0.0, 1.0]
    for n in c.empty:
        lobes[n] = 0.0
    lesions = ((rng.random((N, S), dtype=np.float32) < c.les) & (lobes > 0)).astype(np.float32)
    dense = _logits(rng, N, S, c.scale, c.pos, c.sat)
    refined = _logits(rng, N, S, c.scale, 0.5, c.sat) if c.refined else None
    if c.high_last:             # the last sample: every live logit >= 4, so r is above 0.98 where the others stay below 0.8
        live = np.abs(dense[-1]) <= LIVE_MAX
        dense[-1, live] = np.minimum(np.abs(dense[-1, live]) + 4.0, LIVE_MAX)
    for n in range(N):          # exact zeros on lesion voxels inside the lobe (up to three per sample)
        idx = np.flatnonzero((lobes[n] > 0) & (lesions[n] > 0))[1:7:2]
        dense[n, idx] = 0.0
        if refined is not None:
            refined[n, idx[:1]] = 0.0
    keep = np.asarray([c.keep[n % len(c.keep)] for n in range(N)], dtype=np.float32)
    r, nm = lobe_mean(dense, lobes)
    targets = np.zeros((N, 2), dtype=np.float32)
    for n in range(N):
        rn = r[n] if nm[n] > 0 else 0.5
        targets[n] = _band(c.hinge[n % len(c.hinge)], rn)
    if c.high_last:
        targets[-1] = (0.1, 0.2)
    weight = (0.2 + 0.6 * ((np.arange(N) * 37) % 101) / 100.0).astype(np.float32)
    inp = Inputs(dense, refined, lobes, lesions, keep, targets, weight)
    cond = conditions(cid, inp)
    assert cond["ok"], (cid, cond)
    return inp


def conditions(cid, inp):
    """The input conditions of the module docstring as numbers, and `ok`."""
    c = CASES[cid]
    out = {}
    mags = [np.abs(t.astype(np.float64)) for t in (inp.dense, inp.refined) if t is not None]
    out["min_nonzero"] = min(float(a[a > 0].min()) for a in mags)
    out["in_gap"] = int(sum(((a > LIVE_MAX) & (a < SAT_MIN)).sum() for a in mags))
    out["finite"] = all(bool(np.isfinite(a).all()) for a in mags)
    m = inp.lobes > 0
    out["zeros_on_lesion_in_lobe"] = int(((inp.dense == 0) & m & (inp.lesions > 0)).sum())
    out["zeros_elsewhere"] = int(((inp.dense == 0) & ~(m & (inp.lesions > 0))).sum())
    out["binary_masks"] = all(bool(np.isin(t, (0.0, 1.0)).all()) for t in (inp.lobes, inp.lesions))
    out["lesion_outside_lobe"] = int(((inp.lesions > 0) & ~m).sum())
    r, nm = lobe_mean(inp.dense, inp.lobes)
    lo, hi = inp.targets[:, 0].astype(np.float64), inp.targets[:, 1].astype(np.float64)
    live = nm > 0
    out["hinge_margin"] = float(np.minimum(np.abs(r - lo), np.abs(r - hi))[live].min()) if live.any() else np.inf
    out["samples_without_inside"] = [int(n) for n in np.flatnonzero(~live)]
    out["samples_without_outside"] = [int(n) for n in np.flatnonzero(m.all(1))]
    out["max_count"] = int(max(m.sum(), (~m).sum()))
    expect_no_inside = list(c.empty) + ([1] if c.S == 1 else [])
    expect_no_outside = list(range(c.N)) if c.lobe >= 1.0 else ([0, 2] if c.S == 1 else [])
    out["ok"] = (out["min_nonzero"] >= ZERO_MARGIN and out["in_gap"] == 0 and out["finite"] and out["binary_masks"]
                 and out["zeros_elsewhere"] == 0 and out["lesion_outside_lobe"] == 0 and out["hinge_margin"] >= HINGE_MARGIN
                 and out["samples_without_inside"] == sorted(expect_no_inside)
                 and out["samples_without_outside"] == expect_no_outside and out["max_count"] < 2 ** 24
                 and (out["zeros_on_lesion_in_lobe"] > 0 or c.S < 8))
    return out


# ------------------------------------------------------------------------------------------------ the restatement
class _Sigmoid(torch.autograd.Function):
    """sigmoid with the derivative p * sigmoid(-x): torch's p * (1 - p) is exactly 0 in fp64 from |x| = 37 on, where the
    true derivative (and the kernel's, which keeps 1 - p to full relative accuracy) is not."""

    @staticmethod
    def forward(ctx, x):
        p, q = torch.sigmoid(x), torch.sigmoid(-x)
        ctx.save_for_backward(p, q)
        return p

    @staticmethod
    def backward(ctx, g):
        p, q = ctx.saved_tensors
        return g * p * q


def _nlog(v):
    return -torch.log(v.clamp(EPS, 1.0 - EPS))


PERTURBATIONS = ("c_out", "c_boot", "alpha", "drop_sample_256", "drop_last_element")


def restate(inp, smoothing=SMOOTHING, perturb=None):
    """The fused loss in fp64 on [N, S] inputs.  Returns a dict: reg, seg (floats); n_in, n_out, T (ints); alpha, wsum
    (floats, formed from the counts in the kernel's order); r, nm ([N] fp64, r NaN for an empty lobe); t ([N, S] bool, the
    pseudo label); dreg (d reg / d dense) and dseg (d seg / d refined, or d dense where refined is None), [N, S] fp64, from
    torch.autograd.  `perturb`: one of PERTURBATIONS, the wrong kernels of the sensitivity test."""
    assert perturb is None or perturb in PERTURBATIONS
    f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    d = f64(inp.dense).requires_grad_(True)
    x = d if inp.refined is None else f64(inp.refined).requires_grad_(True)
    m = torch.from_numpy(inp.lobes > 0)
    exists = torch.ones_like(m)
    if perturb == "drop_sample_256":
        exists[256] = False
    if perturb == "drop_last_element":
        exists[:, -1] = False
    inside, outside = m & exists, ~m & exists
    pd = _Sigmoid.apply(d)
    p = pd if x is d else _Sigmoid.apply(x)
    q = _Sigmoid.apply(-x)          # 1 - p without the cancellation
    nm = inside.sum(1).double()
    sp = (pd * inside).sum(1)
    live = nm > 0
    r = sp / nm.clamp_min(1.0)
    lo, hi, w = f64(inp.targets[:, 0]), f64(inp.targets[:, 1]), f64(inp.weight)
    K = (0.5 * (hi - lo)) ** 2
    hinge = torch.clamp((r - 0.5 * (hi + lo)) ** 2 - K, min=0.0) / w
    if perturb == "drop_sample_256":
        live = live.clone()
        live[256] = False
    reg = hinge[live].sum()
    kp = torch.from_numpy(inp.keep > 0).view(-1, 1)
    t = (pd.detach() > 0.5) & inside & torch.from_numpy(inp.lesions > 0) & kp
    n_in, n_out, T = int(inside.sum()), int(outside.sum()), int(t.sum())
    nlp, nlq = _nlog(p), _nlog(q)
    seg = x.sum() * 0.0
    if n_out > 0:
        seg = seg + (nlq * outside).sum() / n_out * (1.01 if perturb == "c_out" else 1.0)
    alpha, wsum = 0.0, 1.0
    if n_in > 0:
        alpha = min(max(1.0 - T / n_in, 0.25), 0.75) + (1e-3 if perturb == "alpha" else 0.0)
        wsum = alpha * T + (1.0 - alpha) * (n_in - T)
        A, B = (nlp * t).sum(), (nlq * (inside & ~t)).sum()
        boot = (torch.where(p > 0.5, nlp, nlq) * inside).sum() / n_in * (1.01 if perturb == "c_boot" else 1.0)
        seg = seg + (1.0 - smoothing) * (alpha * A + (1.0 - alpha) * B) / wsum + smoothing * boot
    dreg, = torch.autograd.grad(reg, d, retain_graph=True, allow_unused=True)
    dseg, = torch.autograd.grad(seg, x, allow_unused=True)
    zero = lambda g: np.zeros(inp.dense.shape) if g is None else g.numpy()
    rr = r.detach().numpy().copy()
    rr[nm.numpy() == 0] = np.nan
    return {"reg": float(reg.detach()), "seg": float(seg.detach()), "n_in": n_in, "n_out": n_out, "T": T, "alpha": alpha, "wsum": wsum,
            "r": rr, "nm": nm.numpy(), "t": t.numpy(), "dreg": zero(dreg), "dseg": zero(dseg)}


@lru_cache(maxsize=None)
def reference(cid):
    """restate(build(cid)), computed once and shared; nobody writes to it."""
    ref = restate(build(cid))
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def expected_grads(ref, gout, distinct):
    """The fp64 gradients the backward entry point owes for upstream gradients gout = (g0, g1): {"ddense": ...} alone when
    refined is absent or the same pointer (the sum goes to ddense), else ddense with the reg term and drefined with seg."""
    g0, g1 = (float(np.float32(g)) for g in gout)
    if distinct:
        return {"ddense": g0 * ref["dreg"], "drefined": g1 * ref["dseg"]}
    return {"ddense": g0 * ref["dreg"] + g1 * ref["dseg"]}


def expected_state(ref):
    """What the state vector must hold: exact integers, bit-exact alpha and wsum, r_n by value."""
    N = ref["nm"].size
    return {"alpha": np.float32(ref["alpha"]), "wsum": np.float32(ref["wsum"]), "n_in": np.float32(ref["n_in"]),
            "n_out": np.float32(ref["n_out"]), "r": ref["r"], "nm": ref["nm"].astype(np.float32), "floats": 4 + 2 * N}


# ------------------------------------------------------------------------------------------------ comparators
def value_ratio(got, ref):
    """|got - ref| over the value bound 2e-5 * max(1, |ref|)."""
    return abs(float(got) - float(ref)) / (VALUE_TOL * max(1.0, abs(float(ref))))


def voxel_classes(inp, ref, logit):
    """The four voxel classes of a gradient with respect to `logit` (dense or refined): saturated (|logit| >= 17) first,
    then outside the lobe, inside with t = 1, inside with t = 0."""
    sat = np.abs(logit.astype(np.float64)) >= SAT_MIN
    m = inp.lobes > 0
    return {"outside": ~m & ~sat, "inside_t1": m & ref["t"] & ~sat, "inside_t0": m & ~ref["t"] & ~sat, "saturated": sat}


def grad_report(got, ref, classes):
    """Per class with a voxel: (name, voxels, max |ref|, max |got - ref|, ratio to GRAD_TOL * max |ref|, ok).  A class whose
    reference is identically 0 must be exactly 0.0: its ratio is 0 where it is and inf where it is not."""
    rows = []
    err = np.abs(got.astype(np.float64) - ref)
    for name in CLASSES:
        sel = classes[name]
        if not sel.any():
            continue
        top, e = float(np.abs(ref[sel]).max()), float(np.nan_to_num(err[sel], nan=np.inf).max())
        if top == 0.0:
            ratio = 0.0 if bool((got[sel] == 0).all()) else float("inf")
        else:
            ratio = e / (GRAD_TOL * top)
        rows.append((name, int(sel.sum()), top, e, ratio, ratio <= 1.0))
    return rows


def grad_ok(got, ref, classes):
    return all(row[-1] for row in grad_report(got, ref, classes))


def old_bound_ok(got, ref):
    """The one bound of tests/test_gpu_train_step.py: max |got - ref| <= 1e-4 * max |ref| over the whole tensor."""
    return float(np.abs(got - ref).max()) <= GRAD_TOL * float(np.abs(ref).max())
