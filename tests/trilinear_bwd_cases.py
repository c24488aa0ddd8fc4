"""Case table of tests/test_gpu_trilinear_bwd.py, a plain-Python restatement of the host-side route rules of the
align_corners=True trilinear backward (csrc/resample.hip: dram_upsample_trilinear_ac_bwd_ws, dram_upsample_trilinear_ac_bwd)
and the float64 reference the kernels are compared with.  Host code only.

The routes (functional.TRI_BWD_ROUTES):
  "z+yx4"     trilinear_bwd_z_kernel into the workspace, then trilinear_bwd_yx4_kernel, `group` planes per round
  "z+gather"  trilinear_bwd_z_kernel into the workspace, then trilinear_bwd_kernel with an identity z axis
  "gather"    trilinear_bwd_kernel alone
  "general"   trilinear_bwd_general_kernel
The restatement (route) is written from the conditions of the host code, not by calling the library;
tests/test_trilinear_bwd_cpu.py ties it to the library through dram_upsample_trilinear_ac_bwd_choice, so that the GPU test
cannot pass while missing the branch a row was written for.

The workspace of a row is given in planes of D*Ho*Wo floats plus spare bytes.  The two-stage routes need at least TRI_CPT = 8
planes of it whatever N*C is (group = planes that fit, rounded down to a multiple of 8), so the rows with 2 or 3 planes of
data get 8, and a single round over the 18 planes of Y2 takes 24."""
import functools
from collections import namedtuple

import numpy as np
import torch

TRI_CPT = 8                     # planes per block (blockIdx.y), and the granule of a workspace round
MAXT = 6                        # taps per input index and axis that the tap kernels hold
YX4_MIN_SCALE = np.float32(0.4546)
YX4_WINDOW = 16                 # outputs [base, base + 15] one thread of the yx4 kernel reads per row
ROUTES = ("z+yx4", "z+gather", "gather", "general")
TWO_STAGE = ("z+yx4", "z+gather")
TOL = 1e-5                      # the project's figure for this operator (test_gpu_parity.py, test_gpu_onload.py)


# ------------------------------------------------------------------------------------------------ route rules
def scale32(n_in, n_out):
    """make_axis: ATen's fp32 align_corners scale."""
    return np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0.0)


def max_taps_host(n_in, n_out):
    """Host-side bound on the outputs that touch one input index (fp64 scale)."""
    if n_out <= 1 or n_in <= 1:
        return n_out
    s = float(n_in - 1) / float(n_out - 1)
    return int(2.0 / s) + 2


def group_list(planes, group):
    """Planes of every workspace round: the `for (p0 = 0; p0 < planes; p0 += group)` loop."""
    return [min(group, planes - p0) for p0 in range(0, planes, group)] if group else []


def route(dy_mis, dx_mis, ws_mis, ws_bytes, in_shape, size):
    """(route, group, planes per round) of a call; *_mis: that pointer is off a 16-byte boundary; ws_bytes 0: no workspace."""
    N, C, D, H, W = in_shape
    Do, Ho, Wo = size
    taps_ok = all(max_taps_host(i, o) <= MAXT for i, o in ((D, Do), (H, Ho), (W, Wo)))
    one_stage = "gather" if taps_ok else "general"
    group = ws_bytes // (D * Ho * Wo * 4)
    group -= group % TRI_CPT
    if group < TRI_CPT or ws_mis or dy_mis or Do <= D or Wo % 4 != 0 or not taps_ok or D * Ho * Wo >= 0x7fffffff:
        return one_stage, 0, []
    sx = scale32(W, Wo)
    yx4 = YX4_MIN_SCALE <= sx <= np.float32(1.0) and W % 4 == 0 and not dx_mis
    return ("z+yx4" if yx4 else "z+gather"), group, group_list(N * C, group)


# ------------------------------------------------------------------------------------------------ fp32 x taps of the yx4 kernel
def src_index32(n_in, n_out, o):
    """src_index in fp32: (i0, i1, l0, l1) of output o."""
    src = scale32(n_in, n_out) * np.float32(o)
    i0 = min(int(src), n_in - 1)
    i1 = i0 + (1 if i0 < n_in - 1 else 0)
    l1 = np.float32(src - np.float32(i0))
    return i0, i1, np.float32(1.0) - l1, l1


def touch_weight32(n_in, n_out, o, i):
    i0, i1, l0, l1 = src_index32(n_in, n_out, o)
    w = np.float32(0.0)
    if i0 == i:
        w = w + l0
    if i1 == i:
        w = w + l1
    return np.float32(w)


def yx4_base(n_in, n_out, xi0):
    """First output of the 16-output window of the thread that owns inputs xi0..xi0+3."""
    if xi0 < 1:
        return 0
    base = int(np.ceil(np.float32(xi0 - 1) / scale32(n_in, n_out))) - 2
    return 0 if base < 0 else base & ~3


def yx4_live_offsets(n_in, n_out):
    """{xi0: sorted offsets o - base of every output o with a non-zero weight on one of the inputs xi0..xi0+3}."""
    live = {}
    for xi0 in range(0, n_in, 4):
        base = yx4_base(n_in, n_out, xi0)
        live[xi0] = sorted({o - base for o in range(n_out) for j in range(4) if touch_weight32(n_in, n_out, o, xi0 + j) != 0})
    return live


# ------------------------------------------------------------------------------------------------ reference
def axis_matrix(n_in, n_out):
    """A [n_out x n_in] in fp64 with ATen's align_corners rule: src = scale * o, i0 = floor(src), i1 = i0 + (i0 < in - 1),
    weights 1 - l1 and l1 (both on i0 where i1 == i0)."""
    A = torch.zeros(n_out, n_in, dtype=torch.float64)
    scale = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
    for o in range(n_out):
        src = scale * o
        i0 = min(int(np.floor(src)), n_in - 1)
        i1 = i0 + (1 if i0 < n_in - 1 else 0)
        l1 = src - i0
        A[o, i0] += 1.0 - l1
        A[o, i1] += l1
    return A


def reference_dx(dy, in_shape):
    """dx[p, z, y, x] = sum over outputs (a, b, c) of A_z[a, z] A_y[b, y] A_x[c, x] dy[p, a, b, c], all in fp64."""
    N, C, D, H, W = in_shape
    Do, Ho, Wo = dy.shape[-3:]
    dx = torch.einsum("az,by,cx,pabc->pzyx", axis_matrix(D, Do), axis_matrix(H, Ho), axis_matrix(W, Wo),
                      dy.double().reshape(N * C, Do, Ho, Wo))
    return dx.reshape(N, C, D, H, W)


def rel_err(got, ref):
    """(max-abs error over max |ref|, relative L2) of got against the fp64 ref."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return ((got - ref).abs().max() / ref.abs().max()).item(), ((got - ref).norm() / ref.norm()).item()


# ------------------------------------------------------------------------------------------------ cases
# shape = (N, C, D, H, W), size = (Do, Ho, Wo); dy / dx / ws: bytes that pointer is off a 16-byte boundary (0 or 4);
# ws_planes, ws_spare: the workspace is ws_planes * D*Ho*Wo*4 + ws_spare bytes; route, groups: what the call must take
Case = namedtuple("Case", "name shape size dy dx ws ws_planes ws_spare route groups data why")


def _c(name, shape, size, route, groups, why, dy=0, dx=0, ws=0, ws_planes=8, ws_spare=0, data=None):
    return Case(name, shape, size, dy, dx, ws, ws_planes, ws_spare, route, groups, data or name, why)


Y1, Y2 = ((1, 3, 4, 4, 8), (8, 8, 16)), ((2, 9, 4, 4, 8), (8, 8, 16))
CASES = [
    _c("Y1", *Y1, "z+yx4", [3], "fewer planes than TRI_CPT"),
    _c("Y2", *Y2, "z+yx4", [18], "18 planes in one round: blockIdx.y 0..2, tail of 2", ws_planes=24),
    _c("Y3", (1, 2, 4, 4, 28), (8, 8, 60), "z+yx4", [2], "x scale 27/59 = 0.4576: output base + 15 is live at xi0 = 16"),
    _c("Y4", (1, 2, 4, 6, 8), (8, 7, 8), "z+yx4", [2], "x scale exactly 1; y 6 -> 7"),
    _c("Y5", (1, 2, 8, 8, 24), (16, 16, 48), "z+yx4", [2], "384 threads per plane: two x blocks, the second ragged"),
    _c("G1", (1, 2, 4, 4, 4), (8, 8, 8), "z+gather", [2], "x scale 3/7 below the yx4 window"),
    _c("G2", (1, 2, 5, 6, 7), (9, 13, 8), "z+gather", [2], "W % 4 != 0"),
    _c("G3", *Y1, "z+gather", [3], "dx alignment alone switches the second stage", dx=4, data="Y1"),
    _c("G4", (1, 2, 1, 4, 4), (6, 8, 8), "z+gather", [2], "D = 1: six z taps with scale 0, exactly MAXT"),
    _c("S1", *Y1, "gather", [], "dy off alignment", dy=4, data="Y1"),
    _c("S2", *Y1, "gather", [], "workspace off alignment", ws=4, data="Y1"),
    _c("S3", *Y1, "gather", [], "workspace of 7 planes: group < TRI_CPT", ws_planes=7, data="Y1"),
    _c("S4", (1, 3, 5, 6, 5), (9, 13, 10), "gather", [], "Wo % 4 != 0, so the ws_bytes entry returns 0"),
    _c("S5", (1, 2, 4, 4, 8), (4, 8, 16), "gather", [], "Do == D"),
    _c("S6", (1, 2, 8, 7, 9), (4, 5, 3), "gather", [], "downsample on every axis"),
    _c("X1", (1, 2, 3, 4, 4), (6, 8, 8), "general", [], "z 3 -> 6: scale 0.4, seven taps"),
    _c("X2", (1, 2, 1, 4, 4), (7, 8, 8), "general", [], "D = 1, seven outputs (neighbour of G4)"),
    _c("X3", (1, 3, 3, 12, 12), (6, 24, 24), "general", [], "two x blocks, three planes on blockIdx.y"),
    _c("P1", *Y2, "z+yx4", [8, 8, 2], "three rounds, the last one short", ws_planes=8, ws_spare=20, data="Y2"),
    _c("P2", *Y2, "z+yx4", [16, 2], "four bytes short of 17 planes: 16 fit", ws_planes=17, ws_spare=-4, data="Y2"),
    _c("P4", *Y2, "z+yx4", [8, 8, 2], "15 planes fit: the round is 8 (down to a multiple of TRI_CPT)", ws_planes=15, data="Y2"),
    _c("P3", (1, 11, 4, 4, 4), (8, 8, 8), "z+gather", [8, 3], "two rounds through the gather second stage", ws_planes=8),
    _c("P3full", (1, 11, 4, 4, 4), (8, 8, 8), "z+gather", [11], "P3 in one round", ws_planes=16, data="P3"),
]
BY_NAME = {c.name: c for c in CASES}
IDS = [c.name for c in CASES]


def per_plane_bytes(case):
    return case.shape[2] * case.size[1] * case.size[2] * 4


def ws_bytes(case):
    return case.ws_planes * per_plane_bytes(case) + case.ws_spare


def restated(case):
    return route(case.dy != 0, case.dx != 0, case.ws != 0, ws_bytes(case), case.shape, case.size)


@functools.lru_cache(maxsize=None)
def case_data(data_name):
    """(dy ~ N(0, 1) in fp32, fp64 reference dx) of the cases that share `data_name`; computed once, not to be modified."""
    case = BY_NAME[data_name]
    seed = 7000 + IDS.index(data_name)
    dy = torch.randn(*case.shape[:2], *case.size, generator=torch.Generator().manual_seed(seed))
    return dy, reference_dx(dy, case.shape)
