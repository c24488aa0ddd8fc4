"""The ledger of tests/conv_row_cases.py, without a device: the table has exactly one case per row of the library's nine 3x3x3
conv kernel tables (dram_conv3d_k3_kernel_rows), and the library's own choice -- the fwd_choice / wgrad_plan a launch goes
through -- sends every case to the row it is filed under.  A new instantiation without a case fails here, and so does a case
whose row is gone or whose shape the plan has started to send elsewhere.

Blocks per tile against boxes: `_split_and_boxes` of test_gpu_wgrad_direct.py is written for N = 2 and reads the box off the
first three template arguments, which is the box only for the two direct families.  `_split_bound` below is the same query
(dram_conv3d_k3_wgrad_ws_bytes over one partial dW) for any N, with the boxes from conv_row_cases.geometry; the two are compared
where both apply.  The workspace is sized for the plan of one tensor and for that of a concat, and a launch whose own plan
needs more slabs than it holds is refused (DRAM_EWS) before anything runs: the figure is an upper bound of the blocks per tile
of any launch that takes place, so a block walks at least boxes / bound of them.
"""
import ctypes
import os
import re

import torch

import conv_row_cases as RC
import test_gpu_wgrad_direct as WD
from conv_row_cases import CASES, EXEMPT


def chunk_channels():
    """KC of csrc/conv_device.h: the input channels of one LDS stage of every forward kernel."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "bodyct-dram_amd", "csrc", "conv_device.h")
    with open(path) as f:
        return int(re.search(r"constexpr int KC = (\d+);", f.read()).group(1))


def _families():
    from dram_amd import functional as HF
    return {RC.FWD: HF.K3_FWD_DIRECT, RC.WZ: HF.K3_FWD_WZ, "conv3d_k3_fwd_c1_kernel": HF.K3_FWD_C1,
            "conv3d_k3_fwd_c1w_kernel": HF.K3_FWD_C1, "conv3d_k3_fwd_wzy_kernel": HF.K3_FWD_WZY,
            "conv3d_k3_fwd_wzy16_kernel": HF.K3_FWD_WZY, RC.WGRAD: HF.K3_WGRAD_DIRECT, RC.VEC: HF.K3_WGRAD_VEC,
            RC.WGWZ + "|false": HF.K3_WGRAD_WZ, RC.WGWZ + "|true": HF.K3_WGRAD_WZ_LAZY, "conv3d_k3_wgrad_c1_kernel": HF.K3_WGRAD_C1,
            "conv3d_k3_wgrad_wzy_kernel": HF.K3_WGRAD_WZY}


def family(row):
    """The launch counter (K3_*) of a row."""
    base = row.split("<")[0]
    if base == RC.WGWZ:
        base += "|true" if row.endswith("true>") else "|false"
    return _families()[base]


def shifted(shape, off):
    """An uninitialised CPU tensor whose base pointer is `off` bytes past a 16-byte boundary."""
    n = 1
    for s in shape:
        n *= s
    store = torch.empty(n + 8)
    lead = (-store.data_ptr() % 16 + off) // 4
    t = store[lead:lead + n].view(*shape)
    assert t.data_ptr() % 16 == off
    return t


def fwd_choice(case, fused):
    """(family, name) of the forward / backward-data launch of a case, from dram_conv3d_k3_fwd_choice_src; the name also as
    functional.conv_fwd_kernel_name gives it for tensors of the case's shapes and alignment."""
    from dram_amd import functional as HF
    from dram_amd import _lib
    big = tuple(a + b for a, b in zip(case.dhw, case.excess)) if case.C2 else (0, 0, 0)
    buf = ctypes.create_string_buffer(96)
    if case.mode == "bwd-data":     # Cout -> C1 + C2 from a plain dy into the split destination
        kind = _lib.lib.dram_conv3d_k3_fwd_choice_src(case.Cout, case.C1 + case.C2, *case.dhw, case.C1, case.C2, *big, 0,
                                                      0, 0, 0, 0, 0, int(case.off != 0), buf, len(buf))
        name = HF.conv_fwd_kernel_name(case.dhw, case.C1 + case.C2, case.Cout, dst_split=(case.C1, case.C2, *big),
                                       src=(shifted((case.N, case.Cout, *case.dhw), case.off), None, 0))
    else:
        ox = (case.excess[2] + 1) // 2 if case.C2 else 0
        kind = _lib.lib.dram_conv3d_k3_fwd_choice_src(case.C1 + case.C2, case.Cout, *case.dhw, case.Cout, 0, 0, 0, 0, int(fused),
                                                      case.C2, *big, ox, int(case.off != 0), buf, len(buf))
        x1 = shifted((case.N, case.C1, *case.dhw), case.off)
        x2 = shifted((case.N, case.C2, *big), 0) if case.C2 else None
        name = HF.conv_fwd_kernel_name(case.dhw, case.Cout, case.C1 + case.C2, fused=fused, src=(x1, x2, ox))
    assert kind >= 0 and name == buf.value.decode(), (name, buf.value)
    return kind, name


def wgrad_choice(case):
    from dram_amd import functional as HF
    from dram_amd import _lib
    buf = ctypes.create_string_buffer(96)
    kind = _lib.lib.dram_conv3d_k3_wgrad_choice(case.N, case.C1, case.C2, case.Cout, *case.dhw, int(case.lazy), buf, len(buf))
    name = HF.conv_wgrad_kernel_name(case.N, case.dhw, case.Cout, case.C1, case.C2, lazy=case.lazy)
    assert kind >= 0 and name == buf.value.decode(), (name, buf.value)
    return kind, name


def choices(case):
    """Every (family, name) the launches of a case take: one, or two for a row driven once plain and once fused."""
    if case.mode == "wgrad":
        return [wgrad_choice(case)]
    return [fwd_choice(case, fused) for fused in {"fwd": (False,), "bwd-data": (False,), "fused": (True,), "fwd+fused": (False, True)}[case.mode]]


def _split_bound(N, ci, co, dhw):
    """Upper bound of the blocks per (ci, co) tile of a backward-weights launch: the partial dW slabs its workspace holds."""
    from dram_amd import _lib
    slab = co * ci * 27 * 4
    ws = _lib.lib.dram_conv3d_k3_wgrad_ws_bytes(N, ci, co, *dhw)
    assert ws > 0 and ws % slab == 0
    return ws // slab


def test_one_case_per_row():
    from dram_amd import functional as HF
    rows = HF.conv_kernel_rows()
    print(f"conv rows: {len(rows)} listed, {len(CASES)} cases, {len(EXEMPT)} exempt")
    assert rows and len(rows) == len(set(rows))
    assert not set(CASES) & set(EXEMPT)
    missing, stale = set(rows) - set(CASES) - set(EXEMPT), (set(CASES) | set(EXEMPT)) - set(rows)
    assert not missing, f"rows without a case: {sorted(missing)}"
    assert not stale, f"cases of rows the library no longer has: {sorted(stale)}"
    assert len(CASES) == len(rows) - len(EXEMPT)
    # at most the combinations that only DRAM_CONV_DIRECT reaches may be exempt: rows of the two direct backward-weights tables
    assert all(r.split("<")[0] in (RC.WGRAD, RC.VEC) for r in EXEMPT), sorted(EXEMPT)


def test_rows_buffer_too_small():
    """The listing reports a buffer that cannot hold it as an error, and writes an empty string."""
    from dram_amd import _lib
    buf = ctypes.create_string_buffer(b"x" * 63, 64)
    assert _lib.lib.dram_conv3d_k3_kernel_rows(buf, len(buf)) < 0
    assert buf.value == b""
    assert _lib.lib.dram_conv3d_k3_kernel_rows(None, 0) < 0


def test_the_library_sends_every_case_to_its_row():
    for row, case in CASES.items():
        assert case.mode in ("fwd", "fused", "bwd-data", "wgrad", "fwd+fused"), row
        assert case.C2 == 0 or case.excess == RC.E, row      # the crop (1, 2, 2) the launches' references use
        for kind, name in choices(case):
            assert (name, kind) == (row, family(row)), (row, case)
        # the mode is the one the row's FUSED / LAZY argument stands for
        if row.endswith("true>"):
            assert case.mode == "fused" or (case.mode == "wgrad" and case.lazy), row
        elif row.endswith("false>"):
            assert case.mode in ("fwd", "bwd-data") or (case.mode == "wgrad" and not case.lazy), row


def test_what_every_case_must_have():
    """More than one box; channel tails; more than one K chunk / channel tile; at least one split destination per forward
    family that has a plain row; a concat among the fused and lazy cases (its second source goes without ReLU)."""
    chunk = chunk_channels()
    for row, case in CASES.items():
        (bx, by, bz), tile = RC.geometry(row)
        d, h, w = case.dhw
        assert RC.boxes(row, case) > case.N, row
        for axis, size, box in (("x", w, bx), ("y", h, by), ("z", d, bz)):   # a ragged last box wherever the rule allows one
            assert (size % box != 0) == (axis in RC.ragged_axes(row)), (row, axis)
        cin = case.Cout if case.mode == "bwd-data" else case.C1 + case.C2    # the launch's K for a forward kernel
        if case.mode == "wgrad" and cin > 1:
            co, ci = tile
            assert case.Cout % co != 0 and cin % ci != 0, row                # tails in both tile directions
            assert -(-case.Cout // co) * -(-cin // ci) >= 4, row             # ... and several tiles
        elif cin > 1:
            assert cin > chunk and cin % chunk != 0, row                     # >= two K chunks, the last one partial
    modes = {(row.split("<")[0], c.mode) for row, c in CASES.items()}
    assert (RC.FWD, "bwd-data") in modes and (RC.WZ, "bwd-data") in modes
    assert any(c.mode == "fused" and c.C2 for c in CASES.values()) and any(c.mode == "wgrad" and c.lazy and c.C2 for c in CASES.values())
    # a concat boundary inside a K chunk, on the direct and on the z-only kernel
    for base in (RC.FWD, RC.WZ):
        assert any(r.split("<")[0] == base and c.mode != "bwd-data" and c.C2 and c.C1 % chunk != 0 for r, c in CASES.items()), base


def test_pipeline_cases_give_a_block_more_than_one_box():
    for row, case in CASES.items():
        if case.mode != "wgrad":
            assert not case.pipeline, row
            continue
        if row.split("<")[0] in (RC.WGRAD, RC.VEC, RC.WGWZ):
            assert case.pipeline, row
        if not case.pipeline:
            continue
        ci = case.C1 + case.C2
        split, nboxes = _split_bound(case.N, ci, case.Cout, case.dhw), RC.boxes(row, case)
        print(f"{row}: at most {split} blocks per tile for {nboxes} boxes")
        assert 1 <= split < nboxes, (row, split, nboxes)
        if case.C2 == 0 and row.split("<")[0] in (RC.WGRAD, RC.VEC):     # where _split_and_boxes applies: the same figures at its N
            assert WD.N == 2
            assert WD._split_and_boxes(ci, case.Cout, case.dhw) == (_split_bound(2, ci, case.Cout, case.dhw),
                                                                     RC.boxes(row, case._replace(N=2))), row


def test_exempt_rows_are_never_chosen():
    """Every exempt row (none, as the plan stands) really is out of reach: no shape of a small grid selects it."""
    from dram_amd import functional as HF
    assert all(isinstance(why, str) and why for why in EXEMPT.values())
    if not EXEMPT:
        return
    seen = set()
    for d in (1, 2, 3, 4, 6):
        for h in (4, 5, 8, 10):
            for w in (6, 8, 12, 16, 20, 22, 32, 40, 64):
                for c1, c2 in ((8, 0), (20, 0), (16, 16), (32, 16), (8, 8), (20, 12)):
                    for co in (24, 40, 64, 72, 136):
                        for lazy in (False, True):
                            seen.add(HF.conv_wgrad_kernel_name(2, (d, h, w), co, c1, c2, lazy=lazy))
    assert not seen & set(EXEMPT), sorted(seen & set(EXEMPT))
