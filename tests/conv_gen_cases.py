"""Case table of tests/test_gpu_conv_gen_tiles.py and a plain-Python restatement of the host-side plans of
csrc/conv3d_gen.hip (launch_fwd, make_phase, the phase loop of dram_conv3d_bwd_data, wgrad_plan).  Host code only.

The restatement says, for a geometry (N, Cin, Cout, size, k, s, p), which block decode every launch of the three
general-conv kernels takes: the x / y block counts and the WQ instantiation of the forward-shaped kernel (forward and every
backward-data phase), and the box / split / channel-group counts and LDS bytes of backward-weights.  Each table row names
the conditions it exists for; tests/test_conv_gen_plan_cpu.py asserts them on the restated plan and ties the restatement
to the library through dram_conv3d_wgrad_ws_bytes (= nsplit * Cout * Cin * T * 4), so that the GPU test cannot pass
while missing the branch a row was written for."""
from collections import namedtuple

KC = 4                      # input channels per K step of the forward-shaped kernel
NQ = 6                      # staged input elements per thread and channel: PS <= 256 * NQ
TYX_MAX = 49
WG_BOX = (2, 4, 32)         # backward-weights voxel box (z, y, x)
WG_PA = 257
WG_NT = 4
WG_HALO_MAX = 12288
LDS_STATIC_LIMIT = 65536    # above it the host asks for dynamic LDS (ensure_dynamic_lds)


def cdiv(a, b):
    return -(-a // b)


def out_size(size, k, s, p):
    return tuple((i + 2 * pp - kk) // ss + 1 for i, kk, ss, pp in zip(size, k, s, p))


# ------------------------------------------------------------------------------------------------ forward-shaped launch
def fwd_launch(M, Q, T, istride):
    """launch_fwd for an output grid Q = (QD, QH, QW) of M channels, T = (Tz, Ty, Tx) taps per grid point and input
    stride istride (z, y, x).  None for an empty grid (no launch)."""
    QD, QH, QW = Q
    if QD <= 0 or QH <= 0 or QW <= 0:
        return None
    BX = 16 if QW <= 16 else 32
    BY = 256 // BX
    HX = (BX - 1) * istride[2] + T[2]
    HY = (BY - 1) * istride[1] + T[1]
    PS = HX * HY
    Tyx = T[1] * T[2]
    assert PS <= 256 * NQ and Tyx <= TYX_MAX
    wq = (Tyx + 1) // 2
    nbx, nby, co_tiles = cdiv(QW, BX), cdiv(QH, BY), cdiv(M, 32)
    return dict(BX=BX, BY=BY, QD=QD, QH=QH, QW=QW, HX=HX, HY=HY, PS=PS, Tyx=Tyx, WQ=5 if wq <= 5 else 13 if wq <= 13 else 25,
                nbx=nbx, nby=nby, co_tiles=co_tiles, lds=2 * (KC * PS + Tyx * KC * 32) * 4,
                blocks=QD * nby * nbx * co_tiles)   # per sample


# ------------------------------------------------------------------------------------------------ backward-data phases
def make_phase(size, k, s, p, r):
    """Phase r of backward-data along one axis: dx positions oo + os * q, q in [0, Q); grid point q reads dy at
    q + ib + u with the filter tap kb + ks * u, u in [0, T)."""
    T = (k - r + s - 1) // s if r < k else 0
    m0 = -((r - p) // s)                    # ceil((p - r) / s); Python's // floors like the library's floordiv
    m1 = (size - 1 - r + p) // s
    return dict(r=r, T=T, m0=m0, Q=max(m1 - m0 + 1, 0), os=s, oo=s * m0 + r - p, ib=m0 - T + 1, kb=r + s * (T - 1), ks=-s)


def phase_positions(ph):
    return [ph["oo"] + ph["os"] * q for q in range(ph["Q"])]


def phase_pairs(ph, q, out):
    """(dy index, filter tap) pairs that grid point q of the phase multiplies, dy indices outside [0, out) read as 0."""
    pairs = [(q + ph["ib"] + u, ph["kb"] + ph["ks"] * u) for u in range(ph["T"])]
    return sorted((o, t) for o, t in pairs if 0 <= o < out)


def transposed_pairs(i, out, k, s, p):
    """Brute force: dx[i] = sum of dy[o] * w[t] over every (o, t) with o * s - p + t == i."""
    return sorted((o, t) for o in range(out) for t in range(k) if o * s - p + t == i)


def bwd_data_plan(Cin, size, k, s, p):
    """The launches of dram_conv3d_bwd_data, in its order, and whether it zero-fills dx first (a phase without taps)."""
    ax = [[make_phase(size[a], k[a], s[a], p[a], r) for r in range(s[a])] for a in range(3)]
    memset = any(ph["Q"] > 0 and ph["T"] == 0 for phases in ax for ph in phases)
    launches = []
    for pz in ax[0]:
        for py in ax[1]:
            for px in ax[2]:
                if 0 in (pz["T"], py["T"], px["T"]):
                    continue
                la = fwd_launch(Cin, (pz["Q"], py["Q"], px["Q"]), (pz["T"], py["T"], px["T"]), (1, 1, 1))
                if la is not None:
                    launches.append(dict(la, phase=(pz, py, px)))
    return dict(axes=ax, memset=memset, launches=launches)


# ------------------------------------------------------------------------------------------------ backward-weights
def wgrad_plan(N, Cin, Cout, size, k, s, p):
    O = out_size(size, k, s, p)
    T = k[0] * k[1] * k[2]
    HZ, HY, HX = ((WG_BOX[a] - 1) * s[a] + k[a] for a in range(3))
    HV = HX * HY * HZ
    CIB = max(min((4 * WG_NT * 32) // T, WG_HALO_MAX // HV, Cin), 1)
    nci, co_tiles = cdiv(Cin, CIB), cdiv(Cout, 32)
    nbz, nby, nbx = (cdiv(O[a], WG_BOX[a]) for a in range(3))
    per_sample = nbx * nby * nbz
    nboxes = N * per_sample
    nsplit = min(cdiv(1024, nci * co_tiles), nboxes)
    bps = cdiv(nboxes, nsplit)
    nsplit = cdiv(nboxes, bps)
    return dict(T=T, HX=HX, HY=HY, HZ=HZ, HV=HV, CIB=CIB, nci=nci, co_tiles=co_tiles, nbx=nbx, nby=nby, nbz=nbz,
                boxes_per_sample=per_sample, nboxes=nboxes, boxes_per_split=bps, nsplit=nsplit,
                last_split=nboxes - (nsplit - 1) * bps, lds=(32 * WG_PA + CIB * HV) * 4, ws_bytes=nsplit * Cout * Cin * T * 4)


def plan(case):
    c = case
    O = out_size(c.size, c.k, c.s, c.p)
    assert min(O) >= 1
    return dict(out=O, fwd=fwd_launch(c.Cout, O, c.k, c.s), dx=bwd_data_plan(c.Cin, c.size, c.k, c.s, c.p),
                wgrad=wgrad_plan(c.N, c.Cin, c.Cout, c.size, c.k, c.s, c.p))


def geom_args(case):
    """The 15 integers every entry point of the general conv takes."""
    return (case.N, case.Cin, case.Cout) + tuple(case.size) + tuple(case.k) + tuple(case.s) + tuple(case.p)


# ------------------------------------------------------------------------------------------------ conditions
def _fwd_wide(wq):
    def cond(c, pl):
        f = pl["fwd"]
        return (f["WQ"] == wq and f["BX"] == 32 and f["nbx"] >= 3 and f["QW"] % 32 not in (0, 1)
                and f["nby"] >= 2 and f["QH"] % f["BY"] != 0 and f["co_tiles"] >= 2 and c.Cout % 32 != 0
                and c.Cin % KC != 0 and c.N >= 2)
    return cond


def _decode_distinct(c, pl):
    f = pl["fwd"]
    return len({c.N, f["QD"], f["nby"], f["nbx"], f["co_tiles"]}) == 5


def _dx_s1_wide(c, pl):
    la = pl["dx"]["launches"]
    return tuple(c.s) == (1, 1, 1) and len(la) == 1 and la[0]["BX"] == 32 and la[0]["nbx"] >= 3


def _dx_s2_wide(c, pl):
    xph = pl["dx"]["axes"][2]
    return (c.s[2] == 2 and c.size[2] >= 66 and c.size[2] % 2 == 1 and all(ph["Q"] > 32 and ph["T"] > 0 for ph in xph)
            and xph[0]["Q"] != xph[1]["Q"] and any(ph["m0"] != 0 for ph in xph)
            and all(la["BX"] == 32 and la["nbx"] == 2 for la in pl["dx"]["launches"]))


def _dx_zero_phase(c, pl):
    xph = pl["dx"]["axes"][2]
    return (c.k[2] == 1 and c.s[2] == 2 and c.size[2] > 32 and pl["dx"]["memset"] and xph[1]["T"] == 0 and xph[1]["Q"] > 32
            and all(la["nbx"] >= 2 for la in pl["dx"]["launches"]))


def _w(fn):
    return lambda c, pl: fn(c, pl["wgrad"])


CONDITIONS = {
    # forward
    "fwd_wide_wq5": _fwd_wide(5),
    "fwd_wide_wq13": _fwd_wide(13),
    "fwd_wide_wq25": _fwd_wide(25),
    "fwd_decode_distinct": _decode_distinct,       # N, QD, nby, nbx, co_tiles pairwise different
    # backward-data
    "dx_s1_nbx3": _dx_s1_wide,
    "dx_s2_two_x_blocks": _dx_s2_wide,
    "dx_zero_phase_wide": _dx_zero_phase,
    # backward-weights
    "wg_boxes_per_split_3": _w(lambda c, w: w["boxes_per_split"] >= 3),
    "wg_split_spans_samples": _w(lambda c, w: c.N >= 2 and w["boxes_per_split"] >= 2
                                 and w["boxes_per_sample"] % w["boxes_per_split"] != 0),
    "wg_short_last_split": _w(lambda c, w: w["nsplit"] >= 2 and 0 < w["last_split"] < w["boxes_per_split"]),
    "wg_ow_over_64_ragged": lambda c, pl: pl["out"][2] > 64 and pl["out"][2] % 32 != 0,
    "wg_stride2_ow_over_32": lambda c, pl: c.s[2] == 2 and pl["out"][2] > 32,
    "wg_short_channel_group": _w(lambda c, w: c.Cin % w["CIB"] != 0),
    "wg_cout_tail": lambda c, pl: c.Cout % 32 != 0,
    "wg_lds_dynamic": _w(lambda c, w: w["lds"] > LDS_STATIC_LIMIT),
    "wg_lds_static": _w(lambda c, w: w["lds"] < LDS_STATIC_LIMIT),
    # placement
    "unaligned_base": lambda c, pl: c.shift % 16 != 0 and c.shift % 4 == 0,
}

# shift: bytes every placed tensor's base pointer is off a 16-byte boundary.  bias: forward adds one.
Case = namedtuple("Case", "name N Cin Cout size k s p shift bias conds")

CASES = [
    # fwd blocks (n 2, qz 6, by 3, bx 4, co 5), rows of 100 = 3 * 32 + 4, 20 = 2 * 8 + 4 rows; dX is one launch of the same
    # shape with 130 -> 6 channels
    Case("k3_wide", 2, 6, 130, (6, 20, 100), (3, 3, 3), (1, 1, 1), (1, 1, 1), 4, True,
         ("fwd_wide_wq5", "fwd_decode_distinct", "dx_s1_nbx3", "wg_ow_over_64_ragged", "wg_cout_tail", "wg_lds_static",
          "unaligned_base")),
    # 10 y x x taps over two z taps: fwd blocks (n 4, qz 5, by 2, bx 3, co 6)
    Case("k255_wide", 4, 5, 163, (4, 11, 70), (2, 5, 5), (1, 1, 1), (1, 2, 2), 0, False,
         ("fwd_wide_wq13", "fwd_decode_distinct", "wg_ow_over_64_ragged", "wg_cout_tail")),
    # 49 y x x taps, y stride 2: fwd blocks (n 3, qz 2, by 4, bx 5, co 6), forward LDS above 64 KiB
    Case("k177_wide_sy2", 3, 3, 165, (2, 52, 131), (1, 7, 7), (1, 2, 1), (0, 3, 3), 8, True,
         ("fwd_wide_wq25", "fwd_decode_distinct", "wg_ow_over_64_ragged", "wg_cout_tail")),
    # 135 boxes, 45 per sample, two per split: split 22 takes the last box of sample 0 and the first of sample 1; the 68th
    # split has one box; 64 = 4 * 15 + 4 input channels
    Case("k3_64to70_splits", 3, 64, 70, (9, 11, 70), (3, 3, 3), (1, 1, 1), (1, 1, 1), 12, False,
         ("wg_split_spans_samples", "wg_short_last_split", "wg_ow_over_64_ragged", "wg_short_channel_group", "wg_cout_tail",
          "wg_lds_dynamic", "dx_s1_nbx3")),
    # 16 channel groups x 2 co tiles leave 32 splits for 90 boxes: three boxes per split
    Case("k5_64to64_three_boxes", 3, 64, 64, (10, 10, 40), (5, 5, 5), (1, 1, 1), (2, 2, 2), 0, True,
         ("wg_boxes_per_split_3", "wg_lds_static")),
    # stride 2 on every axis, W = 75 odd: the x phases of dX have 38 and 37 grid points and start at m0 = 2 and 1
    Case("k7_s2_w75", 2, 9, 33, (9, 13, 75), (7, 7, 7), (2, 2, 2), (3, 3, 3), 4, True,
         ("dx_s2_two_x_blocks", "wg_stride2_ow_over_32", "wg_cout_tail", "unaligned_base")),
    # stride 2 on every axis with output rows of 65 = 2 * 32 + 1: 27 boxes per sample, two per split (split 13 spans both
    # samples); 42 = 10 * 4 + 2 input channels
    Case("k3_s2_splits", 2, 42, 96, (12, 20, 130), (3, 3, 3), (2, 2, 2), (1, 1, 1), 4, False,
         ("wg_stride2_ow_over_32", "wg_split_spans_samples", "wg_short_channel_group", "wg_lds_dynamic", "wg_ow_over_64_ragged",
          "unaligned_base")),
    # kernel 1, stride 2 along x: the odd x positions of dX are the zero fill, under NaN before the call
    Case("k331_sx2_zero_phase", 2, 5, 7, (4, 9, 81), (3, 3, 1), (1, 1, 2), (1, 1, 0), 8, False,
         ("dx_zero_phase_wide", "wg_stride2_ow_over_32", "wg_cout_tail")),
    # single sample, one channel tile, 4 x blocks
    Case("k133_w100", 1, 5, 7, (5, 9, 100), (1, 3, 3), (1, 1, 1), (0, 1, 1), 12, True,
         ("dx_s1_nbx3", "wg_ow_over_64_ragged", "wg_cout_tail", "unaligned_base")),
    # anisotropic kernel and stride, padding 5 of 6 along x: output rows of 42
    Case("k426_s221", 3, 48, 96, (8, 14, 37), (4, 2, 6), (2, 2, 1), (3, 1, 5), 0, False,
         ("wg_lds_dynamic",)),
]
