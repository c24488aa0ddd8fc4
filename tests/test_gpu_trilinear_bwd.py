"""The align_corners=True trilinear backward (csrc/resample.hip), route by route and per plane group, through the C ABI.

Every row of tests/trilinear_bwd_cases.py is one dram_upsample_trilinear_ac_bwd_ws call: dy ~ N(0, 1) sits at the row's
byte shift, dx (NaN before the call: an element that is not written fails) and the workspace sit between guard words (a
write outside either fails), and functional.trilinear_bwd_choice, asked with the very tensors of the call, must name the
row's route and plane group -- tests/test_trilinear_bwd_cpu.py pins the table to the restated host rules.  The result is
compared with the float64 dense-matrix adjoint of ATen's forward (trilinear_bwd_cases.reference_dx) at 1e-5, max-abs over
max |ref| and relative L2.  Where the arithmetic per plane is the same, results are compared bit for bit: a workspace that
splits the planes into rounds against one round, a batch against its planes two at a time, the fallbacks against the entry
point without a workspace, and the Python path under a small TRI_BWD_WS_CAP against the uncapped one.

Each case prints a `trilinear-bwd-accuracy:` line before it asserts (run with -s to see the figures)."""
import pytest
import torch

import trilinear_bwd_cases as T
from test_gpu_onload import Placed, p, stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENTRY = "dram_upsample_trilinear_ac_bwd_ws"


def run(case, dy=None, ws_nbytes=None):
    """One call of the case (dy: a device tensor to use instead of a fresh placement of the case's data).  Asserts the
    route, that dx is written everywhere and that nothing outside dx and the workspace is; returns dx on the host."""
    from dram_amd import _lib, functional as HF
    N, C, D, H, W = case.shape
    if dy is None:
        dy = Placed((N, C) + case.size, case.dy, src=T.case_data(case.data)[0]).t
    assert dy.data_ptr() % 16 == case.dy
    dx = Placed(case.shape, case.dx)
    nbytes = T.ws_bytes(case) if ws_nbytes is None else ws_nbytes
    ws = Placed((nbytes // 4,), case.ws)
    route, group = HF.trilinear_bwd_choice(dy, dx.t, ws.t, case.shape)
    want = T.route(case.dy != 0, case.dx != 0, case.ws != 0, nbytes, case.shape, case.size)
    assert (route, group) == want[:2], (case.name, route, group, want)
    if ws_nbytes is None:
        assert (route, T.group_list(N * C, group)) == (case.route, case.groups), (case.name, route, group)
    _lib.call(ENTRY, p(dy), p(dx.t), p(ws.t), nbytes, N, C, D, H, W, *case.size, stream())
    torch.cuda.synchronize()
    assert dx.intact(), f"{case.name}: write outside dx"
    assert ws.intact(), f"{case.name}: write outside the workspace"
    got = dx.t.cpu()
    assert not bool(torch.isnan(got).any()), f"{case.name}: dx not written everywhere"
    return got


@pytest.fixture(scope="module")
def results():
    """dx of every case that more than one test looks at, computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = run(T.BY_NAME[name])
        return cache[name]
    return get


@pytest.mark.parametrize("case", T.CASES, ids=T.IDS)
def test_route_and_accuracy(case, results):
    got = results(case.name)
    mx, l2 = T.rel_err(got, T.case_data(case.data)[1])
    print(f"trilinear-bwd-accuracy: {case.name} {case.shape}->{case.size} [{case.route}, rounds {case.groups}]: "
          f"max-rel {mx:.2e} rel-L2 {l2:.2e} vs fp64")
    assert mx <= T.TOL and l2 <= T.TOL, f"{case.name}: max-rel {mx:.3e}, rel-L2 {l2:.3e} > {T.TOL}"


@pytest.mark.parametrize("split,whole", [("P1", "Y2"), ("P2", "Y2"), ("P4", "Y2"), ("P3", "P3full")])
def test_rounds_give_the_bits_of_one_round(split, whole, results):
    """A plane's arithmetic does not depend on the round it falls into: a wrong dy / dx offset of a round, a wrong plane
    count of the short last round or a workspace read at the wrong plane changes bits even below the tolerance."""
    assert T.BY_NAME[split].data == T.BY_NAME[whole].data and len(T.BY_NAME[whole].groups) == 1 < len(T.BY_NAME[split].groups)
    assert torch.equal(results(split), results(whole))


def test_batch_gives_the_bits_of_its_planes_two_at_a_time(results):
    """Y2 in one round of 18 planes (three blocks along blockIdx.y, the last with two planes) against nine calls on two planes."""
    whole = results("Y2").flatten(0, 1)
    y2 = T.BY_NAME["Y2"]
    dy = Placed(y2.shape[:2] + y2.size, 0, src=T.case_data("Y2")[0]).t.flatten(0, 1)
    pair = y2._replace(name="Y2 pair", shape=(1, 2) + y2.shape[2:], ws_planes=8, groups=[2])
    for k in range(9):
        got = run(pair, dy=dy[2 * k:2 * k + 2].unsqueeze(0)).flatten(0, 1)
        assert torch.equal(got, whole[2 * k:2 * k + 2]), f"planes {2 * k}, {2 * k + 1}"


@pytest.mark.parametrize("name", ["S1", "S2", "S3"])
def test_fallbacks_give_the_bits_of_the_entry_without_workspace(name, results):
    from dram_amd import _lib
    case = T.BY_NAME[name]
    N, C, D, H, W = case.shape
    dy = Placed((N, C) + case.size, case.dy, src=T.case_data(case.data)[0])
    dx = Placed(case.shape, case.dx)
    _lib.call("dram_upsample_trilinear_ac_bwd", p(dy.t), p(dx.t), N, C, D, H, W, *case.size, stream())
    torch.cuda.synchronize()
    assert dx.intact()
    assert torch.equal(results(name), dx.t.cpu())
    # and the one-stage kernel does not care where dy sits
    assert torch.equal(results("S1"), results("S2")) and torch.equal(results("S2"), results("S3"))


def test_python_path_under_a_small_workspace_cap(monkeypatch):
    """functional.trilinear_ac_backward with TRI_BWD_WS_CAP of 8 planes (rounds 8, 8, 2) against the uncapped call (the 18
    planes of _ws_bytes: rounds 16, 2), through autograd."""
    from dram_amd import functional as HF
    y2 = T.BY_NAME["Y2"]
    dy = T.case_data("Y2")[0].to(DEV)

    def grad():
        x = torch.zeros(y2.shape, device=DEV, requires_grad=True)
        HF.upsample_trilinear_ac(x, size=y2.size).backward(dy)
        torch.cuda.synchronize()
        return x.grad.cpu()
    full = grad()
    cap = 8 * T.per_plane_bytes(y2)
    assert T.route(0, 0, 0, cap, y2.shape, y2.size) == ("z+yx4", 8, [8, 8, 2])
    assert T.route(0, 0, 0, 18 * T.per_plane_bytes(y2), y2.shape, y2.size) == ("z+yx4", 16, [16, 2])
    # the allocator's tensors are 16-byte aligned: the library takes these routes for them
    assert HF.trilinear_bwd_choice(dy, torch.empty(y2.shape, device=DEV), HF._ws(cap, DEV), y2.shape) == ("z+yx4", 8)
    monkeypatch.setattr(HF, "TRI_BWD_WS_CAP", cap)
    capped = grad()
    assert torch.equal(capped, full)
    mx, l2 = T.rel_err(capped, T.case_data("Y2")[1])
    print(f"trilinear-bwd-accuracy: Y2 through autograd, workspace cap of 8 planes: max-rel {mx:.2e} rel-L2 {l2:.2e} vs fp64")
    assert mx <= T.TOL and l2 <= T.TOL
