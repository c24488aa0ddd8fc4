"""CPU checks behind tests/test_gpu_k1_kernels.py: the float64 restatement of tests/k1_cases.py is the oracle's conv3d and
its autograd, the exact inputs satisfy the precondition under which the device must agree bit for bit, every case's kernel
label is what the library itself answers (dram_conv3d_k1_fwd_choice / dram_conv3d_k1_bwd_choice: host arithmetic, the rule
the launches go through), and the table reaches every kernel, pass count, channel tail and round it was written for."""
import numpy as np
import pytest
import torch

from dram_amd import _lib
from oracle import dram_oracle as O

import k1_cases as K

CASES = pytest.mark.parametrize("case", K.CASES, ids=K.IDS)


# ------------------------------------------------------------------------------------------------ the restatement
@CASES
@pytest.mark.parametrize("kind", ["exact", "real"])
def test_restatement_is_the_oracle_in_fp64(case, kind):
    inp = K.exact_inputs(case.id) if kind == "exact" else K.real_inputs(case.id)
    ref = K.reference(case, inp)
    t = lambda a: torch.from_numpy(np.array(a, dtype=np.float64))
    x = t(K.activated(inp.x.astype(np.float64), inp.coef)).requires_grad_(True)
    w = t(inp.w).requires_grad_(True)
    b = None if inp.bias is None else t(inp.bias).requires_grad_(True)
    y = O.conv3d(x.view(case.N, case.Cin, case.S, 1, 1), w.view(case.Cout, case.Cin, 1, 1, 1), b, pad=0).view(case.N, case.Cout, case.S)
    close = lambda got, want: float((got.detach() - t(want)).abs().max()) <= 1e-12 * max(1.0, float(np.abs(want).max()))
    assert close(y, ref["y"])
    if case.op == "bwd":
        y.backward(t(inp.dy))
        assert close(x.grad, ref["dx"]) and close(w.grad.view(case.Cout, case.Cin), ref["dw"]) and close(b.grad, ref["db"])
    if kind == "exact":     # integers: the two fp64 evaluations agree exactly, whatever their order
        assert torch.equal(y.detach(), t(ref["y"]))
        if case.op == "bwd":
            assert torch.equal(x.grad, t(ref["dx"])) and torch.equal(w.grad.view(case.Cout, case.Cin), t(ref["dw"]))
            assert torch.equal(b.grad, t(ref["db"]))


def test_restatement_by_hand():
    x = np.array([[[1, 2], [3, 4]]], dtype=np.float32)                    # N 1, Cin 2, S 2
    w = np.array([[1, -1], [2, 0], [0, 3]], dtype=np.float32)             # Cout 3
    bias = np.array([10, 20, 30], dtype=np.float32)
    dy = np.array([[[1, 0], [0, 1], [2, -2]]], dtype=np.float32)
    ref = K.restate(x, w, bias, dy)
    assert ref["y"].tolist() == [[[8, 8], [22, 24], [39, 42]]]
    assert ref["y_abs"].tolist() == [[[14, 16], [22, 24], [39, 42]]]
    assert ref["dx"].tolist() == [[[1, 2], [5, -6]]]                      # w^T dy
    assert ref["dw"].tolist() == [[1, 3], [2, 4], [-2, -2]] and ref["db"].tolist() == [1, 1, 0]
    assert ref["dw_abs"].tolist() == [[1, 3], [2, 4], [6, 14]] and ref["db_abs"].tolist() == [1, 1, 4]
    coef = np.array([[-1, 2], [0, 5]], dtype=np.float32)                  # rows (n, c): 2 - x clamped at 0; the constant 5
    assert K.activated(x, coef).tolist() == [[[1, 0], [5, 5]]]


# ------------------------------------------------------------------------------------------------ exact inputs
@CASES
def test_exact_inputs_keep_every_partial_sum_exact(case):
    inp = K.exact_inputs(case.id)
    for a in inp:
        if a is not None:
            assert a.dtype == np.float32 and bool((a == np.rint(a)).all())
    margin = K.exactness_margin(case, inp)
    assert 0 < margin < K.EXACT_LIMIT, margin
    ref = K.exact_reference(case.id)
    for name in ("y", "dx", "dw", "db"):
        if name in ref:     # the fp32 cast the device result is compared with loses nothing
            assert bool((ref[name].astype(np.float32).astype(np.float64) == ref[name]).all())
            assert float(np.abs(ref[name]).max()) > 0
    if case.lazy:           # a zero row, a negative row, and ReLU clamps something
        assert 0.0 in inp.coef[:, 0] and bool((inp.coef[:, 0] < 0).any())
        raw = K.activated(inp.x, inp.coef, relu=False)
        assert bool((raw < 0).any()) and bool((K.activated(inp.x, inp.coef) >= 0).all())


def test_real_inputs_are_shared_and_read_only():
    a, b = K.real_inputs("f_vec_co17"), K.real_inputs("f_vec_co17")
    assert a is b and not a.x.flags.writeable
    assert K.exact_reference("d_vec_co17") is K.exact_reference("d_vec_co17")


# ------------------------------------------------------------------------------------------------ routes
@CASES
def test_label_is_the_library_choice(case):
    got = K.library_kernels(case)
    assert case.kernel in got, (case.id, got)
    if case.op == "bwd":    # the label names the kernel of its own half of the call
        assert got[0 if case.kernel in K.DGRAD_KERNELS else 1] == case.kernel
    assert all(s in (0, 4) for s in (case.x_shift, case.out_shift, case.dy_shift))
    # small: at most 2 x 20 x 8196 floats in a tensor
    assert case.N * max(case.Cin, case.Cout) * case.S <= 2 * 20 * 8196, "the case has grown"


def test_choice_over_a_sweep():
    """The rule in words (include/dram_hip.h), over every flag: float4 kernels need S % 4 == 0 and both their tensors
    aligned; backward-weights goes multi for Cout > 1, vec for Cout == 1, scalar without 16-byte rows of dy and x.  x_mis does
    not bear on backward-data, dx_mis not on backward-weights."""
    lib = _lib.lib
    for S in (1, 4, 693, 1028, 4099, 8196, 1 << 33):
        rows16 = S % 4 == 0
        for flags in range(8):
            a, b, c = flags & 1, flags >> 1 & 1, flags >> 2 & 1
            assert lib.dram_conv3d_k1_fwd_choice(a, b, S) == int(rows16 and not a and not b)
            for Cin, Cout in ((1, 1), (64, 1), (1, 2), (64, 8), (128, 8), (20, 17)):
                assert lib.dram_conv3d_k1_bwd_choice(a, b, c, Cin, Cout, S, 0) == int(rows16 and not a and not c)
                want = 2 if not (rows16 and not a and not b) else (3 if Cout == 1 else 4)
                assert lib.dram_conv3d_k1_bwd_choice(a, b, c, Cin, Cout, S, 1) == want
    # more channel tiles than gridDim.z holds: the one-output kernel's loop over outputs takes over
    assert lib.dram_conv3d_k1_bwd_choice(0, 0, 0, 8 * 256, 8 * 256, 4, 1) == 3
    assert lib.dram_conv3d_k1_bwd_choice(0, 0, 0, 8 * 255, 8 * 257, 4, 1) == 4


def test_choice_rejects_bad_arguments():
    lib = _lib.lib
    assert lib.dram_conv3d_k1_fwd_choice(0, 0, 0) < 0 and b"conv3d_k1_fwd_choice: bad dimensions" in lib.dram_last_error()
    for args in ((0, 0, 0, 0, 1, 4, 0), (0, 0, 0, 1, 0, 4, 1), (0, 0, 0, 1, 1, 0, 1), (0, 0, 0, 1, 1, -4, 0)):
        assert lib.dram_conv3d_k1_bwd_choice(*args) < 0 and b"conv3d_k1_bwd_choice: bad dimensions" in lib.dram_last_error()
    for which in (-1, 2):
        assert lib.dram_conv3d_k1_bwd_choice(0, 0, 0, 1, 1, 4, which) < 0 and b"which" in lib.dram_last_error()


def test_workspace_size_is_the_2048_voxel_layout():
    for c in K.BWD_CASES:
        assert _lib.lib.dram_conv3d_k1_bwd_ws_bytes(c.N, c.Cin, c.Cout, c.S) == 4 * K.ws_floats(c)
        assert K.partial_floats(c, K.library_kernels(c)[1]) <= K.ws_floats(c)
    assert _lib.lib.dram_conv3d_k1_bwd_ws_bytes(2, 0, 1, 4) == 0


def test_workspace_and_pointer_errors_are_reported_without_a_gpu():
    """A workspace one byte short, or none, is refused before anything is launched -- also when dx is asked for."""
    q, (N, Cin, Cout, S) = 16, (2, 9, 9, 3080)
    need = _lib.lib.dram_conv3d_k1_bwd_ws_bytes(N, Cin, Cout, S)
    for outs in ((q, q, q), (None, q, None), (None, None, q), (q, None, q)):
        assert _lib.lib.dram_conv3d_k1_bwd(q, q, q, *outs, q, need - 1, N, Cin, Cout, S, None) == -2
        assert b"workspace too small" in _lib.lib.dram_last_error()
        assert _lib.lib.dram_conv3d_k1_bwd_lazy(q, q, q, 1, q, *outs, q, need - 1, N, Cin, Cout, S, None) == -2
        with pytest.raises(_lib.DramHipError, match="workspace is null"):
            _lib.call("dram_conv3d_k1_bwd", q, q, q, *outs, None, need, N, Cin, Cout, S, None)
    with pytest.raises(_lib.DramHipError, match="null pointer"):
        _lib.call("dram_conv3d_k1_bwd", None, q, q, q, q, q, q, need, N, Cin, Cout, S, None)
    with pytest.raises(_lib.DramHipError, match="null pointer"):
        _lib.call("dram_conv3d_k1_fwd", q, q, q, None, N, Cin, Cout, S, None)
    with pytest.raises(_lib.DramHipError, match="bad dimensions"):
        _lib.call("dram_conv3d_k1_fwd", q, q, q, q, 65536, Cin, Cout, S, None)


# ------------------------------------------------------------------------------------------------ coverage
def test_every_kernel_pass_tail_and_round_has_a_case():
    by = {k: [c for c in K.CASES if k in K.library_kernels(c) and c.kernel == k] for k in K.KERNELS}
    assert all(by.values()), {k: len(v) for k, v in by.items()}
    FS, FV, DS, DV, WS, WV, WM = K.KERNELS

    # passes of K1_MAXCO outputs: one, two, three; a full last pass and a ragged one; more than one pass on BOTH kernels of the
    # forward and of backward-data (the scalar read-modify-write and the float4 one)
    for fam in ((FS, FV), (DS, DV)):
        cases = by[fam[0]] + by[fam[1]]
        assert {K.passes(c.Cout) for c in cases} >= {1, 2, 3}
        assert any(c.Cout == K.K1_MAXCO for c in cases) and any(c.Cout == 2 * K.K1_MAXCO for c in cases)
        assert all(any(c.Cout > K.K1_MAXCO and c.Cout % K.K1_MAXCO for c in by[k]) for k in fam)
    assert any(c.Cout > 2 * K.K1_MAXCO for c in by[FV]) and any(c.Cout > 2 * K.K1_MAXCO for c in by[DV])
    # scalar for each reason: the row length; only the written tensor off; only the read tensor off
    assert any(c.S % 4 for c in by[FS]) and any(c.S % 4 for c in by[DS])
    assert any(c.S % 4 == 0 and c.out_shift and not c.x_shift for c in by[FS])
    assert any(c.S % 4 == 0 and c.x_shift and not c.out_shift for c in by[FS])
    assert any(c.S % 4 == 0 and c.out_shift and not c.dy_shift and c.Cout > K.K1_MAXCO for c in by[DS])
    # blocks: a ragged last block of the scalar kernel, a float4 block with one live thread, a sample index > 0
    assert any(c.S > 2 * K.THREADS and c.S % K.THREADS for c in by[FS] + by[DS])
    assert any(c.S // 4 % K.THREADS == 1 for c in by[FV]) and any(c.S // 4 % K.THREADS == 1 for c in by[DV])
    assert all(any(c.N > 1 for c in v) for v in by.values())
    assert any(not c.bias for c in by[FS]) and any(not c.bias for c in by[FV])
    assert any(c.lazy for c in by[FS]) and any(c.lazy for c in by[FV])
    assert all(any(c.lazy for c in by[k]) for k in (WS, WV, WM))

    # conv1x1_wgrad_vec_kernel: one output; every Cin % WG_CT situation crossed with every block situation
    assert all(c.Cout == 1 and c.S % 4 == 0 and not (c.x_shift or c.dy_shift) for c in by[WV])
    tiles = lambda c: (K.cdiv(c.Cin, K.WG_CT), c.Cin % K.WG_CT)
    blocks = lambda c: (K.cdiv(c.S, K.WG_VPB), min(c.S, K.WG_VPB) // 4, (c.S % K.WG_VPB) // 4)
    want_tiles = {(1, 7), (1, 0), (2, 1), (3, 8)}         # a tail alone; exactly one tile; two tiles, tail 1; three, tail 8
    want_blocks = {(1, 1, 1),                             # one thread
                   (1, K.THREADS + 1, K.THREADS + 1),     # one block, 257 float4: thread 0 alone has a second one
                   (2, 2 * K.THREADS, 1)}                 # a full block and one with a single live thread
    plain = [c for c in by[WV] if not c.lazy]
    assert {(tiles(c), blocks(c)) for c in plain} == {(t, b) for t in want_tiles for b in want_blocks}
    assert all(c.N == 2 for c in plain)

    # conv1x1_wgrad_multi_kernel: channel tiles crossed with rounds
    ch = lambda c: (K.cdiv(c.Cin, K.WM_CT), c.Cin % K.WM_CT, K.cdiv(c.Cout, K.WM_CO), c.Cout % K.WM_CO)
    want_ch = {(1, 1, 1, 2),      # Cout = 2, the smallest that selects it: six of eight output rows idle
               (1, 0, 1, 0),      # exact tiles
               (2, 1, 2, 1),      # 2 x 2 tiles, tails of one channel: blockIdx.z = 0..3
               (3, 4, 3, 1)}      # 3 x 3 tiles
    full = K.WM_VPB // K.WM_ROUND
    want_rounds = {((0, 1),),                 # one thread
                   ((3, 2),),                 # fewer than four rounds: three full ones and a round of two threads
                   ((full, 0), (0, 1))}       # a full block of eight rounds, a second block with one float4
    plain = [c for c in by[WM] if not c.lazy]
    assert {(ch(c), tuple(K.multi_rounds(c.S))) for c in plain} == {(t, r) for t in want_ch for r in want_rounds}
    assert min(c.Cout for c in by[WM]) == 2 and all(c.N == 2 for c in plain)
    # ... its partials leave part of the workspace untouched in at least one case, and fill it in another
    assert any(K.partial_floats(c, WM) < K.ws_floats(c) for c in by[WM])
    assert any(K.partial_floats(c, WM) == K.ws_floats(c) for c in by[WM])

    # conv1x1_wgrad_kernel with several outputs: for the row length, for dy alone, for x alone
    many = [c for c in by[WS] if c.Cout > 1]
    assert any(c.S % 4 for c in many)
    assert any(c.S % 4 == 0 and c.dy_shift and not c.x_shift for c in many)
    assert any(c.S % 4 == 0 and c.x_shift and not c.dy_shift for c in many)
    assert any(K.cdiv(c.S, K.WG_VPB) > 1 and c.S % K.WG_VPB < K.THREADS for c in many)      # a last block of a few voxels


def test_rounding_counts():
    assert K.k_fwd(64) == 65 and K.k_fwd(1) == 2
    assert [K.k_dgrad(co) for co in (1, 8, 9, 11, 16, 17)] == [2, 9, 10, 10, 10, 11]
    assert all(K.k_dgrad(co) <= co + K.passes(co) for co in range(1, 40))      # never more than a single chain would take
    assert K.bound(17, np.array([2.0]))[0] == 17 * 2.0 ** -23
