"""Inputs and host references of tests/test_gpu_row_kernels.py (checked against torch's CPU ops by
tests/test_row_kernels_cpu.py).  Host code only: numpy and torch on the CPU.

The row kernels (csrc/act.hip, the reductions of csrc/head.hip, the ReLU pair of csrc/norm.hip) walk (n, c) rows of S
contiguous floats in chunks of CHUNK = 8192 or in capped grid-stride loops.  The structural cases feed them numbers on which
fp32 addition is exact in ANY order, so the expected value is one integer and the check is bit equality:
  * data        non-zero integers in +-1 ... +-DATA_MAX  (a lost element is never a zero),
  * masks       0 / 1,
  * cotangents  non-zero integers in +-1 ... +-COT_MAX,
  * PReLU slopes powers of two.
Every partial sum of such terms is an integer of magnitude <= (largest term) * (number of terms); while that stays below
2^24 every fp32 addition and fused multiply-add on the way is exact.  worst_case() derives that product per chunk and per row
from these ranges and S alone; the CPU test asserts it for every table row."""
import numpy as np
import torch

CHUNK = 8192              # ACHUNK (csrc/act.hip) == CS_CHUNK (csrc/head.hip)
THREADS = 256             # block size of every chunk kernel
DATA_MAX = 8
COT_MAX = 4
EXACT_LIMIT = 2 ** 24     # integers below it are fp32 numbers, and so are their sums
U = 2.0 ** -24            # unit roundoff of fp32

S_CHUNKED = (CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 77)
S_MULTI = 3 * CHUNK + 77  # = 89 * 277: the multi-chunk S of the all-ones, per-channel-mask and real-valued cases
DHW_MULTI = (1, 89, 277)

# (id, N, C, S)
MASKED_MEAN_CASES = [(f"S{S}", 3, 23, S) for S in S_CHUNKED]        # 69 rows: the finalise kernel's 2nd block has 5 live threads
CHANNEL_SUM_CASES = [(f"S{S}", 2, 70, S) for S in S_CHUNKED]        # 70 channels: 2nd finalise block has 6 live threads
# (id, N, C, nparam, S)
PRELU_CHUNK_CASES = [(f"S{S}_a{k}", 2, 3, k, S) for S in S_CHUNKED for k in (1, 3)]
PRELU_DA_CASES = [
    ("one_slope_280_partials", 8, 5, 1, 6 * CHUNK + 5),             # 40 rows x 7 chunks > 256: prelu_da_kernel's strided loop
    ("per_channel_260_partials", 5, 2, 2, 52 * CHUNK - 3),          # N * nchunks = 260 > 256, rows r * C + p
    ("per_channel_C5_N3_3chunks", 3, 5, 5, 2 * CHUNK + 100),
]
# one row each, S past the block cap of the grid-stride loop
S_STREAM = 1024 * 2048 + 517        # stream_blocks(): <= 1024 blocks of 256 threads x 8 elements (PReLU fwd, global-max bwd)
S_MEAN_BWD = 1024 * 256 + 300       # masked_mean_bwd: <= 1024 blocks of 256
RELU_SIZES = (1, 255, 257, 8192 * 256 + 1000)   # relu_grid(): <= 8192 blocks of 256

SLOPES = (0.25, -0.5, 2.0, 0.125, -1.0)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(shape, hi, seed):
    """float32 tensor of non-zero integers, uniform over +-1 ... +-hi."""
    g = gen(seed)
    mag = torch.randint(1, hi + 1, shape, generator=g)
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (mag * sign).float()


def masks(N, S, seed):
    """(N, S) 0/1 masks, a different one per sample: n % 3 == 0 about half full, == 1 ONE voxel, the row's last (so it
    lies in the last chunk and every other chunk's partial is 0), == 2 about a quarter full."""
    g = gen(seed)
    m = torch.zeros(N, S)
    for n in range(N):
        if n % 3 == 1:
            m[n, S - 1] = 1.0
        else:
            m[n] = (torch.rand(S, generator=g) < (0.5 if n % 3 == 0 else 0.25)).float()
            m[n, n % S] = 1.0          # never empty
    return m


def slopes(nparam):
    return torch.tensor(SLOPES[:nparam], dtype=torch.float32)


def worst_case(kind, S, rows_per_sum=1):
    """(per chunk, per row) upper bounds of sum |term| for the exact inputs, from the builders' ranges and S alone.
    rows_per_sum: how many rows one fp32 result collects (channel sum: N) -- those are added in fp64, listed for the record."""
    term = {"masked_mean": DATA_MAX, "mask_count": 1, "channel_sum": DATA_MAX, "prelu_da": DATA_MAX * COT_MAX}[kind]
    return term * min(S, CHUNK), term * S * rows_per_sum


# ------------------------------------------------------------------------------------------------ references (numpy)
def masked_mean_ref(x, m, dout=None):
    """x (N, C, S), m (N, S) or (N, C, S), dout (N, C); integers held in float32.  out = float32(float64(sum x*m) /
    float64(sum m)), msum = the voxel count, dx = (float32 dout / float32 msum) * m with the division in fp32."""
    xi, mi = x.numpy().astype(np.int64), m.numpy().astype(np.int64)
    per_sample = mi.ndim == 2
    if per_sample:
        mi = np.broadcast_to(mi[:, None, :], xi.shape)
    s, cnt = (xi * mi).sum(-1), mi.sum(-1)
    out = (s.astype(np.float64) / cnt.astype(np.float64)).astype(np.float32)
    msum = cnt.astype(np.float32)
    res = {"out": torch.from_numpy(out), "msum": torch.from_numpy(msum[:, 0].copy() if per_sample else msum)}
    if dout is not None:
        g = dout.numpy().astype(np.float32) / msum
        assert g.dtype == np.float32
        res["dx"] = torch.from_numpy(g[..., None] * mi.astype(np.float32))
    return res


def channel_sum_ref(x):
    """x (N, C, S) of integers -> float32(exact sum over n and S)."""
    return torch.from_numpy(x.numpy().astype(np.int64).sum((0, 2)).astype(np.float32))


def prelu_ref(x, a, dy=None):
    """x, dy (N, C, S) integers, a (1,) or (C,) powers of two.  y and dx are exact products; da = float32(exact integer sum of
    dy * x over x <= 0) per parameter."""
    C = x.shape[1]
    ar = a.numpy().astype(np.float32)
    arow = (ar if ar.size == C else np.repeat(ar, C))[None, :, None]
    xn = x.numpy()
    res = {"y": torch.from_numpy(np.where(xn > 0, xn, arow * xn).astype(np.float32))}
    if dy is not None:
        gn = dy.numpy()
        res["dx"] = torch.from_numpy(np.where(xn > 0, gn, arow * gn).astype(np.float32))
        prod = np.where(xn > 0, 0, xn.astype(np.int64) * gn.astype(np.int64))
        tot = prod.sum((0, 2)) if ar.size == C else prod.sum(keepdims=True).reshape(1)
        res["da"] = torch.from_numpy(tot.astype(np.float32))
        res["da_exact"] = tot
    return res


def relu_input(n, seed):
    """Finite real values with exact zeros every 7th element, and a cotangent.  NaN handling of the fmaxf that every fused
    kernel shares is not this test's: there is no NaN here."""
    g = gen(seed)
    x = torch.randn(n, generator=g)
    x[::7] = 0.0
    return x, torch.randn(n, generator=g)


# ------------------------------------------------------------------------------------------------ global max
GMAX_S = (1, 255, 256, 257, 70001)
GMAX_ROWS = 5
GMAX_PATTERNS = ("first", "last", "tie_one_thread", "tie_two_threads", "all_equal", "all_neg_inf", "pos_inf", "two_nans")
# (higher index, lower index) of one maximum stored twice: threads 44 / 5, 4 / 5 (the lower index sits on the HIGHER thread),
# 255 / 0, 112 / 0 and 1 / 0 of global_max_kernel's 256
TIE_PAIRS = ((300, 5), (260, 5), (511, 256), (70000, 0), (4097, 4096))
# (first NaN, the larger finite value, last NaN) at S = 70001: two threads; neighbours; the FIRST NaN on the higher thread
# (200 vs 260 % 256 = 4); both NaNs on thread 7; the row's tail
NAN_TRIPLES = ((5, 300, 70000), (46, 47, 48), (200, 230, 260), (7, 100, 263), (69998, 69999, 70000))


def gmax_fits(pattern, S):
    """Whether the row pattern exists at this S (two elements 256 apart need S > 256, ...)."""
    return S >= {"tie_one_thread": 257, "tie_two_threads": 70001, "two_nans": 255}.get(pattern, 1)


GMAX_CASES = [(p, S) for p in GMAX_PATTERNS for S in GMAX_S if gmax_fits(p, S)]


def gmax_input(pattern, S):
    """x (1, GMAX_ROWS, 1, 1, S) and the expected flat index per row.  Every row has its own background of +-1 ... +-8 and its
    own planted maximum 9 + r, so that a value or an index taken from another row is a different number."""
    x = ints((1, GMAX_ROWS, 1, 1, S), DATA_MAX, 100 + S)
    rows = x.view(GMAX_ROWS, S)
    want = []
    for r in range(GMAX_ROWS):
        top = float(DATA_MAX + 1 + r)
        if pattern == "first":
            rows[r, 0] = top
            want.append(0)
        elif pattern == "last":
            rows[r, S - 1] = top
            want.append(S - 1)
        elif pattern == "tie_one_thread":           # e and e + 256 are both visited by thread e % 256
            e = (r * 12345) % (S - 256)
            rows[r, e] = rows[r, e + 256] = top
            want.append(e)
        elif pattern == "tie_two_threads":
            hi, lo = TIE_PAIRS[r]
            rows[r, hi] = rows[r, lo] = top
            want.append(lo)
        elif pattern == "all_equal":
            rows[r] = float(r - 2)                  # -2 ... 2, the zero row included
            want.append(0)
        elif pattern == "all_neg_inf":
            rows[r] = float("-inf")
            want.append(0)
        elif pattern == "pos_inf":
            e = (r * 7919 + 3) % S
            rows[r, e] = float("inf")
            rows[r, (e + 1) % S] = top if S > 1 else float("inf")
            want.append(e)
        elif pattern == "two_nans":                 # ATen keeps the LAST NaN of a window
            a, k, b = NAN_TRIPLES[r] if S == 70001 else (3 * r + 1, S // 2, S - 1 - 2 * r)
            assert 0 <= a < k < b < S
            rows[r, a] = rows[r, b] = float("nan")
            rows[r, k] = top
            want.append(b)
        else:
            raise KeyError(pattern)
    return x, torch.tensor(want, dtype=torch.int64).view(1, GMAX_ROWS)


def same_values(a, b):
    """Bit-for-bit agreement of two float tensors that may hold NaN: NaN in the same places, torch.equal everywhere else."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(a[~na], b[~nb])


# ------------------------------------------------------------------------------------------------ the real-valued bound
# A chunk kernel adds a chunk's terms in fp32: CHUNK / THREADS = 32 accumulations per thread (a fused multiply-add rounds
# once, like the addition it replaces), 6 levels of the 64-lane butterfly, 3 additions across the block's 4 waves.  So a term
# passes through at most 32 + 6 + 3 = 41 fp32 roundings, each of relative size <= U = 2^-24 of a partial sum that is itself
# <= sum |terms|: |partial - exact| <= ((1 + U)^41 - 1) * sum |terms of the chunk|.  The partials of a result are then added in
# fp64 (some hundred roundings of 2^-53) and rounded to fp32 once (U * |result|).  (1 + U)^41 - 1 < 41.0001 U; the two spare U
# hold that second-order term, the fp64 additions, masked mean's fp64 division and the difference between U * |got| and
# U * |ref| with room to spare.  Hence
#       |got - ref| <= (41 + 2) * U * sum |terms| + U * |ref|,      sum |terms| and ref evaluated in fp64.
FP32_ROUNDINGS = CHUNK // THREADS + 6 + 3
assert FP32_ROUNDINGS == 41


def sum_bound(sum_abs_terms, ref):
    """Elementwise bound on |got - ref| of an fp32 chunked sum; both arguments float64 tensors."""
    return (FP32_ROUNDINGS + 2) * U * sum_abs_terms + U * ref.abs()


def real_case(kind):
    """randn inputs at S = S_MULTI, the fp64 reference and sum |terms| of one reduction.
    Returns (inputs dict of float32 tensors, ref float64, sum_abs float64)."""
    S = S_MULTI
    if kind == "masked_mean":
        g = gen(41)
        x = torch.randn(3, 23, *DHW_MULTI, generator=g)
        m = (torch.rand(3, 1, *DHW_MULTI, generator=g) < 0.4).float()
        xm = (x.double() * m.double()).view(3, 23, S)
        cnt = m.double().view(3, 1, S).sum(-1)
        return {"x": x, "m": m}, xm.sum(-1) / cnt, xm.abs().sum(-1) / cnt
    if kind == "channel_sum":
        x = torch.randn(2, 70, S, generator=gen(42))
        return {"x": x}, x.double().sum((0, 2)), x.double().abs().sum((0, 2))
    if kind == "prelu_da":
        g = gen(43)
        x = torch.randn(3, 5, *DHW_MULTI, generator=g)
        dy = torch.randn(3, 5, *DHW_MULTI, generator=g)
        a = torch.tensor([0.25, -0.1, 0.3, 1.7, 0.01])
        t = torch.where(x > 0, torch.zeros((), dtype=torch.float64), x.double() * dy.double()).view(3, 5, S)
        return {"x": x, "dy": dy, "a": a}, t.sum((0, 2)), t.abs().sum((0, 2))
    raise KeyError(kind)
