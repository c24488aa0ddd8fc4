"""Inputs, tile constants and the written-out tolerance for tests/test_guided_cpu.py and tests/test_gpu_guided.py.  Everything is
generated from seeds; nothing here touches the GPU.  The shared arrays are read-only."""
import functools

import numpy as np

import guided_restatement as GR

# tile constants of csrc/guided.hip
GX_T = 256          # x pass: outputs along x per wave (a block holds GX_ROWS rows)
GX_ROWS = 4
GA_TX = 128         # axis passes: columns per block
GA_LT = 32          # axis passes: outputs along the summed axis per block
MAX_RADIUS = 16     # dram_guided_max_radius()

WINDOW = (-1150.0, 350.0)
EPS = 1e-3
U24, U53 = 2.0 ** -24, 2.0 ** -53

# name: (shape, radius (rz, ry, rx), guide dtype, mask kind)
#   tiles:  x pass 524 = 2 * 256 + 12 along x and 67 * 69 rows;  y pass 69 = 2 * 32 + 5 along y, 524 = 4 * 128 + 12 columns;
#           z pass 67 = 2 * 32 + 3 along z, 69 * 524 columns.  W % 4 == 0: the 16-byte paths.
#   odd_w:  W = 261 = 128 * 2 + 5 = 256 + 5 is odd and H * W is odd: the element-wise paths of all three passes, past one tile.
CASES = {
    "ragged_i16": ((19, 23, 37), (2, 3, 5), np.int16, "ellipsoid"),
    "ragged_f32": ((19, 23, 37), (2, 3, 5), np.float32, "ellipsoid"),
    "ragged_iso": ((19, 23, 37), (2, 2, 2), np.int16, "ellipsoid"),
    "tiles": ((67, 69, 524), (3, 2, 5), np.int16, "random"),
    "odd_w": ((34, 35, 261), (2, 2, 2), np.float32, "random"),
    "w_mod4": ((6, 9, 42), (1, 2, 3), np.float32, "random"),
    "length1": ((1, 21, 40), (2, 2, 2), np.int16, "random"),
    "short_z": ((3, 40, 40), (5, 2, 2), np.float32, "random"),
    "radius0": ((12, 13, 16), (2, 0, 3), np.int16, "ellipsoid"),
    "cap": ((20, 20, 40), (16, 16, 16), np.float32, "random"),
    "island": ((12, 14, 20), (2, 2, 2), np.int16, "island"),
    "faces": ((9, 10, 12), (1, 2, 2), np.float32, "full"),
}


def _seed(name):
    return sorted(CASES).index(name) + 101


def make_mask(shape, kind, rng):
    D, H, W = shape
    if kind == "full":
        return np.ones(shape, dtype=np.uint8)
    if kind == "random":                                          # ragged, touches every face, values other than 1 count as inside
        return (rng.integers(0, 5, size=shape) > 0).astype(np.uint8) * rng.integers(1, 256, size=shape).astype(np.uint8)
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij", sparse=True)
    ell = (((z - (D - 1) / 2) / (0.45 * D)) ** 2 + ((y - (H - 1) / 2) / (0.4 * H)) ** 2 + ((x - (W - 1) / 2) / (0.42 * W)) ** 2) < 1.0
    if kind == "island":                                          # a small blob and one voxel far from it
        ell = (((z - 3) / 2.5) ** 2 + ((y - 4) / 3.0) ** 2 + ((x - 5) / 4.0) ** 2) < 1.0
        ell = ell | np.zeros(shape, dtype=bool)
        ell[D - 2, H - 3, W - 2] = True
    return ell.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(guide, p, mask): int16 HU on both sides of the window or float32 in [0, 1); p float32 in [0, 1); mask uint8."""
    shape, _, dtype, kind = CASES[name]
    rng = np.random.default_rng(_seed(name))
    if dtype == np.int16:
        guide = np.rint(rng.uniform(-1400.0, 600.0, size=shape)).astype(np.int16)
    else:
        guide = rng.random(size=shape).astype(np.float32)
    p = rng.random(size=shape).astype(np.float32)
    mask = make_mask(shape, kind, rng)
    for a in (guide, p, mask):
        a.setflags(write=False)
    return guide, p, mask


def window_of(name):
    return WINDOW if CASES[name][2] == np.int16 else None


@functools.lru_cache(maxsize=None)
def expected(name):
    guide, p, mask = inputs(name)
    ref = GR.guided_filter(guide, p, mask, CASES[name][1], EPS, window_of(name))
    for a in ref.values():
        a.setflags(write=False)
    return ref


def fp64_terms(radius, eps, g_max, p_max):
    """The fp64 share of |device - restatement|, for a, b and q: bounds that hold for ANY order of the window sums.

    u = 2^-53.  A window sum is three separable passes of direct sums, so a term passes through at most K = 2 (rz + ry + rx)
    additions and the sum carries at most K u times the sum of the magnitudes; divided by N that is K u times a mean, at most
    K u G for g, K u P for p, K u G^2 and K u G P for the products (G = max |g|, P = max |p| on the region).  With the rounding
    of the product itself (an int16 guide's g has 53 bits), of the division by N, of mg * mp and of the subtraction,
        d_cov <= (3 K + 8) u G P        d_var <= (3 K + 8) u G^2
    (the two means enter mg * mp with (K + 1) u each).  a = cov / (var + eps), var + eps >= eps, and by Cauchy-Schwarz and
    var + eps >= 2 sqrt(var eps):  |a| <= a_max = P / (2 sqrt(eps)).  Hence
        d_a <= (d_cov + a_max d_var) / eps + u a_max            -- the  k 2^-53 (summed magnitudes) / eps  term
        d_b <= (K + 3) u P + d_a G + a_max (K + 3) u G          (b = mp - a mg, |b| <= b_max = P + a_max G)
    and the second stage adds its own sums and the final multiply-add:
        d_A <= d_a + (K + 1) u a_max      d_B <= d_b + (K + 1) u b_max      d_q <= d_A G + d_B + 4 u (a_max G + b_max)."""
    K = 2 * int(sum(radius))
    G, P = float(g_max), float(p_max)
    a_max = P / (2.0 * np.sqrt(eps))
    b_max = P + a_max * G
    c = (3 * K + 8) * U53
    d_a = (c * G * P + a_max * c * G * G) / eps + U53 * a_max
    d_b = (K + 3) * U53 * P + d_a * G + a_max * (K + 3) * U53 * G
    d_A = d_a + (K + 1) * U53 * a_max
    d_B = d_b + (K + 1) * U53 * b_max
    d_q = d_A * G + d_B + 4 * U53 * (a_max * G + b_max)
    return {"a": d_a, "b": d_b, "q": d_q}


def magnitudes(guide, p, mask, window):
    m = np.asarray(mask) != 0
    if not m.any():
        return 0.0, 0.0
    return float(np.abs(GR.guide_values(guide, window)[m]).max()), float(np.abs(np.asarray(p, dtype=np.float64)[m]).max())


def check(tag, got_q, got_ab, ref, terms):
    """|q - q64| <= 2^-24 |q64| + d_q (q64: the restatement before its one rounding to fp32), |a - a_ref| <= d_a, |b - b_ref| <=
    d_b; prints the measured maxima next to the bounds; returns the three ratios measured / allowed."""
    e_q = np.abs(got_q.astype(np.float64) - ref["q64"])
    tol_q = U24 * np.abs(ref["q64"]) + terms["q"]
    out = [float((e_q / tol_q).max())]
    line = f"{tag}: q max error {e_q.max():.3e} (fp64 term {terms['q']:.3e}, one fp32 half-ulp at 1: {U24:.3e})"
    if got_ab is not None:
        for k, key in enumerate("ab"):
            e = float(np.abs(got_ab[k] - ref[key]).max())
            out.append(e / terms[key])
            line += f"; {key} max error {e:.3e} (bound {terms[key]:.3e})"
    print(line)
    return out
