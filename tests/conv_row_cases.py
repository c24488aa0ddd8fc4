"""One launch per row of the nine 3x3x3 conv kernel tables of csrc/conv3d_k3.hip / conv3d_k3_wgrad_wzy.hip, keyed by the exact
name the library reports for the row (dram_conv3d_k3_kernel_rows; the spelling of the two choice queries).  Pure data: nothing
here touches the library or a device.  tests/test_conv_rows_cpu.py keeps the table equal to the library's list of rows and asks
the library's own choice for every case; tests/test_gpu_conv_rows.py launches every case against an fp64 convolution.

Every shape is the smallest one found that the plan (fwd_choice / wgrad_plan) sends to the row in-process -- no DRAM_*
switch -- and that still has what shows a wrong geometry constant of that instantiation:

  * more than one box along an axis, with a ragged last box on every axis the row's rule leaves free (the z-only and 16-byte
    backward-weights rows take full boxes along x only; the (z,y) rows even H and D only);
  * a channel tail in the K direction (forward: K is no multiple of the KC = 4 channels of an LDS chunk, csrc/conv_device.h, in
    every family; a concat boundary lies inside a chunk; backward-weights: tails in both tile directions, and more than one tile);
  * at least two K chunks per block (forward) / two boxes per block (backward-weights: `pipeline`), the `has_next` arm;
  * fused / lazy rows: coefficient rows from onload_reference.coef_table (a < 0, a == 0, an all-zero row under ReLU); with a
    second source that one goes without ReLU, so that a * 0 + b != 0 and an activated zero padding would show.

How a row is reached (csrc/conv3d_k3.hip):
  direct forward         Cin < 8, or D == 1; pick_box takes the box that pads least: (1, 6, 40) -> 32x4x2, (3, 6, 44) -> 16x4x4,
                         (3, 14, 20) -> 8x8x4.  COT 2 from Cout > 32 (backward-data: C1 + C2 > 32).
  z-only forward         Cin >= 8, D >= 2, Cout % 64 != 0; wz_best_box counts boxes per plane: (3, 60) -> 32x4, (12, 12) -> 16x8,
                         (20, 6) -> 8x16, (18, 9) -> 10x10.
  first layer            Cin == 1; the wide form from W % 4 == 0 and W >= 96.
  (z,y) forward          Cout % 64 == 0, W % 4 == 0: (4, 8, 60) pads 1.07x on 32x4x2 boxes; (4, 7, 44) pads 1.25x on 16x4x4 ones,
                         within 1.3x of the z-only kernel's best.
  direct backward-w.     W % 4 != 0: (3, ., 54) -> 32x2x1, (3, ., 42) -> 16x2x2 (a tie with 32x2x1: the first listed wins),
                         (5, 15, 22) -> 8x4x2.  The 128 co x 16 ci tile from Cout > 64.
  16-byte staging        D == 1 and full boxes along x: W = 64 -> 32x2x1, W = 16 -> 16x2x2 (tie), W = 8 -> 8x4x2.
  z-only backward-w.     D = 3 (odd: the (z,y) kernel is out); W % 16 / 8 / 4 == 0 -> 16x2 / 8x4 / 4x8 positions.  The 64 co x 32 ci
                         tile for one tensor or a concat boundary at 32, whatever Cout is; the 128 x 16 tile only for 16 ++ k
                         with Cout > 64.
  (z,y) backward-w.      D, H even, D >= 4, W % 4 == 0 with at most 1.6x padding along x: (6, 10, 40).

A backward-weights block walks more than one box only when tiles x boxes exceeds the 1024 blocks wzy_split hands out at most,
hence the 100 to 220 boxes (N x boxes of the volume) of these cases with their 6 to 10 channel tiles.
"""
from collections import namedtuple

# mode: "fwd" (plain sources, bias), "fused" (lazy sources, statistics epilogue), "fwd+fused" (rows without a FUSED template
#       argument: once with bias, once through the fused entry point), "bwd-data" (the backward-data launch of a conv
#       C1 + C2 -> Cout: Cout -> C1 + C2 into a split destination), "wgrad"
# C1, C2, excess: channels of the two tensors of the virtual concat and what the second one's (D, H, W) exceed dhw by (None: one tensor)
# lazy: backward-weights only -- x normalised on load (forward: mode "fused");  off: bytes off 16-byte alignment of the
#       launch's first source (forward: x1 / dy; backward-weights: x1 and dy)
# pipeline: backward-weights only -- the library's workspace proves fewer blocks per tile than boxes
Case = namedtuple("Case", "mode N C1 C2 excess Cout dhw lazy off pipeline", defaults=(False, 0, False))

E = (2, 3, 3)       # centre-crop offsets (1, 2, 2): the window starts at an odd x, rows of W + 3 floats
FWD, WZ, WGRAD, VEC, WGWZ = ("conv3d_k3_fwd_kernel", "conv3d_k3_fwd_wz_kernel", "conv3d_k3_wgrad_kernel",
                             "conv3d_k3_wgrad_vec_kernel", "conv3d_k3_wgrad_wz_kernel")
D32, D16, D8 = (1, 6, 40), (3, 6, 44), (3, 14, 20)                      # direct forward boxes 32x4x2, 16x4x4, 8x8x4
Z32, Z16, Z8, Z10 = (3, 3, 60), (3, 12, 12), (3, 20, 6), (3, 18, 9)     # z-only forward positions 32x4, 16x8, 8x16, 10x10

CASES = {
    # ---- direct forward / backward-data
    FWD + "<32, 4, 2, 1, false>": Case("fwd", 2, 10, 0, None, 24, D32),
    FWD + "<32, 4, 2, 1, true>": Case("fused", 2, 6, 5, E, 20, D32),
    FWD + "<32, 4, 2, 2, false>": Case("fwd", 2, 10, 0, None, 40, D32, off=4),
    FWD + "<32, 4, 2, 2, true>": Case("fused", 2, 10, 0, None, 72, D32),
    FWD + "<16, 4, 4, 1, false>": Case("fwd", 2, 3, 4, E, 24, D16),
    FWD + "<16, 4, 4, 1, true>": Case("fused", 2, 7, 0, None, 20, D16),
    FWD + "<16, 4, 4, 2, false>": Case("bwd-data", 2, 30, 10, E, 6, D16),
    FWD + "<16, 4, 4, 2, true>": Case("fused", 2, 3, 4, E, 40, D16),
    FWD + "<8, 8, 4, 1, false>": Case("bwd-data", 2, 5, 3, E, 6, D8),
    FWD + "<8, 8, 4, 1, true>": Case("fused", 2, 6, 0, None, 24, D8),
    FWD + "<8, 8, 4, 2, false>": Case("fwd", 2, 7, 0, None, 40, D8),
    FWD + "<8, 8, 4, 2, true>": Case("fused", 2, 3, 4, E, 72, D8),
    # ---- z-only Winograd forward / backward-data: K = 18, 22 or 10 ++ 8 (a chunk across the two sources); odd D (half-empty
    # last plane pair)
    WZ + "<32, 4, 1, false>": Case("fwd", 2, 18, 0, None, 24, Z32, off=4),
    WZ + "<32, 4, 1, true>": Case("fused", 2, 10, 8, E, 24, Z32),
    WZ + "<32, 4, 2, false>": Case("fwd", 2, 18, 0, None, 40, Z32),
    WZ + "<32, 4, 2, true>": Case("fused", 2, 22, 0, None, 72, Z32),
    WZ + "<16, 8, 1, false>": Case("bwd-data", 2, 8, 8, E, 18, Z16),
    WZ + "<16, 8, 1, true>": Case("fused", 2, 18, 0, None, 24, Z16),
    WZ + "<16, 8, 2, false>": Case("fwd", 2, 10, 8, E, 40, Z16),
    WZ + "<16, 8, 2, true>": Case("fused", 2, 10, 8, E, 40, Z16),
    WZ + "<8, 16, 1, false>": Case("fwd", 2, 18, 0, None, 24, Z8),
    WZ + "<8, 16, 1, true>": Case("fused", 2, 10, 8, E, 32, Z8),
    WZ + "<8, 16, 2, false>": Case("bwd-data", 2, 24, 16, E, 22, Z8),
    WZ + "<8, 16, 2, true>": Case("fused", 2, 18, 0, None, 72, Z8),
    WZ + "<10, 10, 1, false>": Case("fwd", 2, 10, 8, E, 24, Z10),
    WZ + "<10, 10, 1, true>": Case("fused", 2, 18, 0, None, 24, Z10),
    WZ + "<10, 10, 2, false>": Case("fwd", 2, 22, 0, None, 72, Z10),
    WZ + "<10, 10, 2, true>": Case("fused", 2, 10, 8, E, 40, Z10),
    # ---- first layer (32x8x4 / 128x4x4 boxes, ragged on every axis; a partial second channel tile)
    "conv3d_k3_fwd_c1_kernel": Case("fwd+fused", 2, 1, 0, None, 40, (5, 9, 35)),
    "conv3d_k3_fwd_c1w_kernel": Case("fwd+fused", 2, 1, 0, None, 40, (5, 6, 100)),
    # ---- (z,y) Winograd forward: whole 64-channel tiles; a last K chunk of 2 channels; ragged x box (28 of 32; 12 of 16 and
    # 3 of 4 rows)
    "conv3d_k3_fwd_wzy_kernel": Case("fwd+fused", 2, 18, 0, None, 128, (4, 8, 60)),
    "conv3d_k3_fwd_wzy16_kernel": Case("fwd+fused", 2, 10, 0, None, 64, (4, 7, 44)),
    # ---- direct backward-weights, dword staging: ragged boxes; the only kernel whose channel tile may straddle the two tensors
    WGRAD + "<32, 2, 1, 8, 1>": Case("wgrad", 4, 72, 0, None, 136, (3, 9, 54), pipeline=True),
    WGRAD + "<32, 2, 1, 4, 2>": Case("wgrad", 4, 168, 0, None, 40, (3, 17, 54), off=4, pipeline=True),
    WGRAD + "<16, 2, 2, 8, 1>": Case("wgrad", 4, 20, 52, E, 136, (3, 9, 42), pipeline=True),
    WGRAD + "<16, 2, 2, 4, 2>": Case("wgrad", 4, 168, 0, None, 40, (3, 17, 42), pipeline=True),
    WGRAD + "<8, 4, 2, 8, 1>": Case("wgrad", 3, 72, 0, None, 136, (5, 15, 22), pipeline=True),
    WGRAD + "<8, 4, 2, 4, 2>": Case("wgrad", 5, 40, 128, E, 40, (5, 15, 22), pipeline=True),
    # ---- direct backward-weights, 16-byte staging: D = 1, full boxes along x, ragged along y
    VEC + "<32, 2, 1, 8, 1>": Case("wgrad", 3, 72, 0, None, 136, (1, 51, 64), pipeline=True),
    VEC + "<32, 2, 1, 4, 2>": Case("wgrad", 4, 168, 0, None, 40, (1, 51, 64), pipeline=True),
    VEC + "<16, 2, 2, 8, 1>": Case("wgrad", 3, 16, 56, E, 136, (1, 101, 16), pipeline=True),
    VEC + "<16, 2, 2, 4, 2>": Case("wgrad", 4, 168, 0, None, 40, (1, 101, 16), pipeline=True),
    VEC + "<8, 4, 2, 8, 1>": Case("wgrad", 3, 72, 0, None, 136, (1, 202, 8), pipeline=True),
    VEC + "<8, 4, 2, 4, 2>": Case("wgrad", 4, 32, 136, E, 40, (1, 202, 8), pipeline=True),
    # ---- z-only Winograd backward-weights: odd D, ragged along y; the 128 x 16 tile only behind a 16 ++ k boundary
    WGWZ + "<16, 2, 8, 1, false>": Case("wgrad", 3, 16, 56, E, 136, (3, 9, 64), pipeline=True),
    WGWZ + "<16, 2, 8, 1, true>": Case("wgrad", 3, 16, 56, E, 136, (3, 9, 64), lazy=True, pipeline=True),
    WGWZ + "<16, 2, 4, 2, false>": Case("wgrad", 3, 72, 0, None, 136, (3, 9, 64), pipeline=True),
    WGWZ + "<16, 2, 4, 2, true>": Case("wgrad", 3, 32, 40, E, 136, (3, 9, 64), lazy=True, pipeline=True),
    WGWZ + "<8, 4, 8, 1, false>": Case("wgrad", 4, 16, 56, E, 136, (3, 18, 24), pipeline=True),
    WGWZ + "<8, 4, 8, 1, true>": Case("wgrad", 4, 48, 24, E, 136, (3, 18, 24), lazy=True, pipeline=True),
    WGWZ + "<8, 4, 4, 2, false>": Case("wgrad", 4, 32, 40, E, 136, (3, 18, 24), off=4, pipeline=True),
    WGWZ + "<8, 4, 4, 2, true>": Case("wgrad", 4, 72, 0, None, 136, (3, 18, 24), lazy=True, pipeline=True),
    WGWZ + "<4, 8, 8, 1, false>": Case("wgrad", 4, 16, 56, E, 136, (3, 36, 12), pipeline=True),
    WGWZ + "<4, 8, 8, 1, true>": Case("wgrad", 4, 16, 56, E, 136, (3, 36, 12), lazy=True, pipeline=True),
    WGWZ + "<4, 8, 4, 2, false>": Case("wgrad", 4, 72, 0, None, 136, (3, 36, 12), pipeline=True),
    WGWZ + "<4, 8, 4, 2, true>": Case("wgrad", 4, 32, 40, E, 136, (3, 36, 12), lazy=True, pipeline=True),
    # ---- first layer backward-weights (32x4x2 boxes, one block per box below 1024 boxes: nothing to pipeline)
    "conv3d_k3_wgrad_c1_kernel": Case("wgrad", 2, 1, 0, None, 40, (5, 9, 35)),
    # ---- (z,y) Winograd backward-weights: 16 ci x 64 co tiles, ragged third box along x.  180 boxes over 6 tiles: a block
    # walks two boxes, but the workspace of this family is sized for a finer per-source split, so it cannot prove that
    "conv3d_k3_wgrad_wzy_kernel<false>": Case("wgrad", 4, 40, 0, None, 72, (6, 10, 40), off=4),
    "conv3d_k3_wgrad_wzy_kernel<true>": Case("wgrad", 4, 16, 24, E, 72, (6, 10, 40), lazy=True),
}

# Rows the plan cannot choose in-process, with the line of the plan that blocks them.  (The plan reaches every row.)
EXEMPT = {}

# (bx, by, bz) of a row's boxes and the output channels of a block (forward) / the (co, ci) block tile (backward-weights), for
# naming where a wrong element lies.  Read off the row's name; the rows without template arguments are listed.
_FIXED = {
    "conv3d_k3_fwd_c1_kernel": ((32, 8, 4), 32), "conv3d_k3_fwd_c1w_kernel": ((128, 4, 4), 32),
    "conv3d_k3_fwd_wzy_kernel": ((32, 4, 2), 64), "conv3d_k3_fwd_wzy16_kernel": ((16, 4, 4), 64),
    "conv3d_k3_wgrad_c1_kernel": ((32, 4, 2), (32, 1)),
    "conv3d_k3_wgrad_wzy_kernel<false>": ((16, 2, 2), (64, 16)), "conv3d_k3_wgrad_wzy_kernel<true>": ((16, 2, 2), (64, 16)),
}


def geometry(row):
    """((bx, by, bz), tile) of a row: tile = output channels per block (forward rows) or (co, ci) per block (backward-weights)."""
    if row in _FIXED:
        return _FIXED[row]
    base, targs = row.rstrip(">").split("<")
    t = [int(v) for v in targs.split(", ") if v not in ("true", "false")]
    if base == FWD:
        return (t[0], t[1], t[2]), 32 * t[3]
    if base == WZ:
        return (t[0], t[1], 2), 32 * t[2]
    if base in (WGRAD, VEC):
        return (t[0], t[1], t[2]), (16 * t[3], 16 * t[4])
    assert base == WGWZ, row
    return (t[0], t[1], 2), (16 * t[2], 16 * t[3])


def ragged_axes(row):
    """The axes ("x", "y", "z") along which the row's rule lets the last box be ragged."""
    base = row.split("<")[0]
    if base == VEC:                                      # full boxes along x; D == 1
        return "y" if geometry(row)[0][2] == 1 else "yz"
    if base == WGWZ:                                     # full boxes along x
        return "yz"
    if base == "conv3d_k3_wgrad_wzy_kernel":             # even H and D
        return "x"
    if base == "conv3d_k3_fwd_wzy_kernel":               # 32x4x2 boxes only where they pad at most 1.2x
        return "x"
    if base == "conv3d_k3_fwd_wzy16_kernel":             # 16x4x4 boxes up to 1.3x of the z-only kernel's padding
        return "xy"
    return "xy" if geometry(row)[0][2] == 1 else "xyz"


def boxes(row, case):
    """Boxes of the case's volume, over all samples."""
    (bx, by, bz), _ = geometry(row)
    d, h, w = case.dhw
    return case.N * -(-w // bx) * -(-h // by) * -(-d // bz)
