"""CPU checks behind tests/test_gpu_trilinear_bwd.py: the restated route rules of the align_corners=True trilinear backward
(tests/trilinear_bwd_cases.py) agree with the library's own choice (dram_upsample_trilinear_ac_bwd_choice, host arithmetic
only), the case table reaches every route, flag and fallback it was written for, the 16-output window of the yx4 kernel holds
every live weight (and is used to its last output by the case written for that), and the float64 reference is the adjoint of
ATen's forward."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dram_amd import _lib

import trilinear_bwd_cases as T

CASES = pytest.mark.parametrize("case", T.CASES, ids=T.IDS)


def library_choice(dy_mis, dx_mis, ws_mis, ws_bytes, shape, size):
    group = ctypes.c_int64(-1)
    rc = _lib.lib.dram_upsample_trilinear_ac_bwd_choice(int(dy_mis), int(dx_mis), int(ws_mis), ws_bytes, *shape, *size,
                                                        ctypes.byref(group))
    assert rc >= 0, _lib.lib.dram_last_error()
    return T.ROUTES[rc], group.value


# ------------------------------------------------------------------------------------------------ routes
@CASES
def test_restated_route_is_the_table_and_the_library(case):
    route, group, groups = T.restated(case)
    assert (route, groups) == (case.route, case.groups), (route, group, groups)
    assert library_choice(case.dy, case.dx, case.ws, T.ws_bytes(case), case.shape, case.size) == (route, group)
    assert sum(groups) == (case.shape[0] * case.shape[1] if route in T.TWO_STAGE else 0)
    assert group % T.TRI_CPT == 0 and all(0 < g <= group for g in groups)
    assert case.dy in (0, 4) and case.dx in (0, 4) and case.ws in (0, 4) and T.ws_bytes(case) % 4 == 0
    # small: at most 2 x 16 x 16 x 48 gradient voxels (Y5, the smallest with two x blocks in the yx4 kernel)
    assert int(np.prod(case.shape[:2])) * int(np.prod(case.size)) <= 24576, "the case has grown"


def test_restated_route_is_the_library_over_a_sweep():
    """Every pair of axis lengths around the tap bound and the yx4 window, every flag, workspaces around the 8-plane granule."""
    n = 0
    seen = set()
    for W, Wo in [(4, 8), (4, 12), (8, 8), (8, 16), (8, 20), (12, 24), (12, 28), (28, 60), (7, 8), (8, 10), (3, 8), (1, 8), (8, 4)]:
        for D, Do in [(1, 6), (1, 7), (3, 6), (4, 8), (4, 4), (5, 3), (2, 5), (2, 6), (1, 1), (3, 7)]:
            shape, size = (2, 5, D, 3, W), (Do, 5, Wo)
            per_plane = D * 5 * Wo * 4
            for ws_bytes in (0, 7 * per_plane, 8 * per_plane - 4, 8 * per_plane, 9 * per_plane + 4, 16 * per_plane):
                for flags in range(8):
                    mis = (flags & 1, flags >> 1 & 1, flags >> 2 & 1)
                    r = T.route(*mis, ws_bytes, shape, size)
                    assert library_choice(*mis, ws_bytes, shape, size) == r[:2], (shape, size, ws_bytes, mis, r)
                    seen.add(r[0])
                    n += 1
    assert n == 13 * 10 * 6 * 8 and seen == set(T.ROUTES)


def test_choice_rejects_bad_sizes():
    group = ctypes.c_int64(0)
    assert _lib.lib.dram_upsample_trilinear_ac_bwd_choice(0, 0, 0, 0, 1, 1, 0, 4, 4, 8, 8, 8, ctypes.byref(group)) < 0
    assert b"bad sizes" in _lib.lib.dram_last_error()
    assert _lib.lib.dram_upsample_trilinear_ac_bwd_choice(0, 0, 0, 0, 1, 70000, 4, 4, 4, 8, 8, 8, ctypes.byref(group)) < 0
    assert b"out of range" in _lib.lib.dram_last_error()


def test_tap_bound_edges():
    """The edges of MAXT = 6 that the X and G cases stand on."""
    assert T.max_taps_host(1, 6) == 6 and T.max_taps_host(1, 7) == 7          # an axis of length 1: every output
    assert T.max_taps_host(3, 6) == 7                                          # scale exactly 0.4: int(2 / 0.4) + 2
    assert T.max_taps_host(4, 8) == 6 and T.max_taps_host(28, 60) == 6
    # (1, 1, 3, 4, 128) x2 of test_trilinear_align_corners: D = 3 -> 6 sends its backward to the general kernel
    assert T.route(0, 0, 0, 1 << 30, (1, 1, 3, 4, 128), (6, 8, 256))[0] == "general"


def test_every_route_flag_and_fallback_has_a_case():
    by_route = {r: [c for c in T.CASES if c.route == r] for r in T.ROUTES}
    assert all(by_route.values())
    aligned = dict(dy=0, dx=0, ws=0)
    for flag in ("dy", "dx", "ws"):
        # a case where this flag alone is raised, and where lowering it changes the route
        hits = [c for c in T.CASES if getattr(c, flag) == 4 and all(getattr(c, f) == 0 for f in aligned if f != flag)]
        assert hits, flag
        for c in hits:
            assert T.route(0, 0, 0, T.ws_bytes(c), c.shape, c.size)[0] != c.route, (flag, c.name)
    # the small-workspace fallback: a row that a workspace of 8 planes would send through two stages
    small = [c for c in T.CASES if c.ws_planes < T.TRI_CPT and c.route == "gather"]
    assert small and all(T.route(0, 0, 0, 8 * T.per_plane_bytes(c), c.shape, c.size)[0] in T.TWO_STAGE for c in small)
    # more than one round through either second stage, with a short last round; a round rounded down to the granule
    for r in T.TWO_STAGE:
        assert any(len(c.groups) >= 2 and c.groups[-1] < c.groups[0] for c in by_route[r]), r
    assert any(T.ws_bytes(c) // T.per_plane_bytes(c) > c.groups[0] > 0 and len(c.groups) > 1 for c in by_route["z+yx4"])
    # blockIdx.y > 0 in the yx4 kernel and in the general kernel; both ends of the yx4 scale window
    assert any(max(c.groups) > T.TRI_CPT for c in by_route["z+yx4"])
    assert any(c.shape[0] * c.shape[1] > 1 for c in by_route["general"])
    sx = [T.scale32(c.shape[4], c.size[2]) for c in by_route["z+yx4"]]
    assert max(sx) == 1.0 and min(sx) < 0.46
    assert any(T.scale32(c.shape[4], c.size[2]) < T.YX4_MIN_SCALE and c.shape[4] % 4 == 0 and c.dx == 0 for c in by_route["z+gather"])


# ------------------------------------------------------------------------------------------------ the yx4 window
@pytest.mark.parametrize("case", [c for c in T.CASES if c.route == "z+yx4"], ids=lambda c: c.name)
def test_yx4_window_holds_every_live_weight(case):
    live = T.yx4_live_offsets(case.shape[4], case.size[2])
    assert len(live) == case.shape[4] // 4
    for xi0, offs in live.items():
        assert offs and offs[0] >= 0 and offs[-1] < T.YX4_WINDOW, (xi0, offs)


def test_y3_uses_the_last_output_of_the_window():
    live = T.yx4_live_offsets(28, 60)
    assert T.YX4_WINDOW - 1 in live[16], live
    # no narrower row at this ratio does: the reason the case is 28 wide
    for W, Wo in [(8, 16), (24, 48), (8, 8)]:
        assert all(offs[-1] < T.YX4_WINDOW - 1 for offs in T.yx4_live_offsets(W, Wo).values())


# ------------------------------------------------------------------------------------------------ the reference
def aten_dx(dy, case, dtype):
    x = torch.zeros(case.shape, dtype=dtype, requires_grad=True)
    F.interpolate(x, size=case.size, mode="trilinear", align_corners=True).backward(dy.to(dtype))
    return x.grad


@CASES
def test_reference_is_aten_in_fp64(case):
    dy, ref = T.case_data(case.data)
    mx, l2 = T.rel_err(aten_dx(dy, case, torch.float64), ref)
    assert mx <= 1e-12 and l2 <= 1e-12, (mx, l2)


def test_reference_by_hand():
    # 2 -> 3 along one axis: outputs at 0, 0.5, 1
    assert torch.equal(T.axis_matrix(2, 3), torch.tensor([[1, 0], [0.5, 0.5], [0, 1]], dtype=torch.float64))
    dy = torch.tensor([1.0, 10.0, 100.0]).view(1, 1, 1, 1, 3)
    assert torch.equal(T.reference_dx(dy, (1, 1, 1, 1, 2)).flatten(), torch.tensor([6.0, 105.0], dtype=torch.float64))
    # 3 -> 2 along y: outputs at 0 and 2; the last output has i0 = i1 = 2, the middle input gets nothing
    dy = torch.tensor([3.0, 5.0]).view(1, 1, 1, 2, 1)
    assert torch.equal(T.reference_dx(dy, (1, 1, 1, 3, 1)).flatten(), torch.tensor([3.0, 0.0, 5.0], dtype=torch.float64))
    # z 1 -> 3 (every output on the one input) times x 2 -> 3, two planes
    dy = torch.tensor([[[1.0, 2.0, 4.0]], [[8.0, 16.0, 32.0]], [[64.0, 128.0, 256.0]]]).view(1, 1, 3, 1, 3)
    dy = torch.cat([dy, -2 * dy], 1)
    want = torch.tensor([[73.0 + 73.0, 73.0 + 292.0], [-292.0, -730.0]], dtype=torch.float64)
    assert torch.equal(T.reference_dx(dy, (1, 2, 1, 1, 2)).view(2, 2), want)
    # 3 -> 5: scale 0.5, rows (1, 0, 0), (.5, .5, 0), (0, 1, 0), (0, .5, .5), (0, 0, 1)
    assert torch.equal(T.axis_matrix(3, 5).sum(0), torch.tensor([1.5, 2.0, 1.5], dtype=torch.float64))


@CASES
def test_aten_fp32_backward_is_within_the_gpu_tolerance(case):
    """The reference alone: an fp32 evaluation of the same adjoint (ATen's, CPU) stays within the tolerance asked of the
    kernels, so a kernel that misses it is wrong and the data is not to blame."""
    dy, ref = T.case_data(case.data)
    mx, l2 = T.rel_err(aten_dx(dy, case, torch.float32), ref)
    print(f"trilinear-bwd-accuracy: {case.name} ATen fp32 (CPU): max-rel {mx:.2e} rel-L2 {l2:.2e} vs fp64")
    assert mx <= T.TOL and l2 <= T.TOL, (mx, l2)
