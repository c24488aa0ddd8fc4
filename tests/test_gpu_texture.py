"""csrc/texture.hip on the device against the numpy restatement (tests/texture_restatement.py, itself held against a textbook table
and direct pair counts by tests/test_texture_cpu.py): the tables are integers, so every comparison is exact."""
import numpy as np
import pytest
import torch

import texture_cases as TC

pytestmark = pytest.mark.gpu

GUARD = 64


def _st():
    return torch.cuda.current_stream().cuda_stream


def _placed(a, offset):
    """A device copy of the flat array whose first element lies `offset` elements past a 16-byte boundary; (holder, pointer)."""
    flat = np.ascontiguousarray(a).reshape(-1)
    holder = torch.zeros(flat.size + offset, dtype=torch.from_numpy(flat[:1].copy()).dtype, device="cuda")
    assert holder.data_ptr() % 16 == 0
    holder[offset:] = torch.from_numpy(flat.copy())
    return holder, holder.data_ptr() + offset * flat.itemsize


def gpu_table(scan, labels, kind, mask, n, levels, distance, offset=0, lo=TC.LO, width=TC.WIDTH):
    """dram_label_glcm through the C ABI on a guard-banded, poisoned output (the entry initialises it); every input `offset`
    elements off the 16-byte alignment."""
    from dram_amd._lib import call
    lab = TC.as_kind(labels, kind)
    holders = [_placed(scan, offset), _placed(lab, offset)] + ([] if mask is None else [_placed(mask, offset)])
    size = n * 13 * levels * levels
    out = torch.full((2 * GUARD + size,), -7, dtype=torch.int64, device="cuda")
    call("dram_label_glcm", holders[0][1], holders[1][1], kind, None if mask is None else holders[2][1], n, lo, width, levels, distance,
         out[GUARD:].data_ptr(), *lab.shape, _st())
    host = out.cpu().numpy()
    del holders
    assert np.all(host[:GUARD] == -7) and np.all(host[GUARD + size:] == -7), "a guard band was written"
    return host[GUARD:GUARD + size].reshape(n, 13, levels, levels).copy()


def _assert_equal(got, ref, where):
    assert got.dtype == ref.dtype and got.shape == ref.shape, where
    bad = np.argwhere(got != ref)
    assert bad.size == 0, (where, len(bad), bad[:5].tolist(), [int(got[tuple(b)]) for b in bad[:5]], [int(ref[tuple(b)]) for b in bad[:5]])


@pytest.mark.parametrize("name", TC.names())
def test_label_glcm_matches_the_restatement(name):
    c = TC.case(name)
    plans = set()
    for kind, n, levels, distance, masked in c["runs"]:
        ref = TC.expected(name, n, levels, distance, masked)
        plans.add(TC.plan(kind, n, levels, distance))
        for offset in (0, 1):                                            # vector loads, and every row piece off its alignment
            got = gpu_table(c["scan"], c["labels"], kind, c["mask"] if masked else None, n, levels, distance, offset)
            _assert_equal(got, ref, (name, kind, n, levels, distance, masked, offset))
    assert plans == {0, 1}, plans
    kind, n, levels, distance, masked = c["runs"][-1]
    again = gpu_table(c["scan"], c["labels"], kind, c["mask"] if masked else None, n, levels, distance, 1)
    assert again.tobytes() == got.tobytes()                               # no dependence on the order of the atomics


def test_every_setting_is_exercised():
    runs = [r for name in TC.names() for r in TC.case(name)["runs"]]
    seen = {(TC.plan(kind, n, levels, d), kind) for kind, n, levels, d, _ in runs}
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {r[2] for r in runs} == {2, 16, 32} and {r[3] for r in runs} == {1, 2, 4} and {r[4] for r in runs} == {False, True}
    for d in (1, 2, 4):
        assert {TC.plan(kind, n, levels, dd) for kind, n, levels, dd, _ in runs if dd == d} == {0, 1}, d
    odd = TC.case("odd")
    assert odd["labels"].min() < 0 and (odd["labels"] == 4).any() and (odd["labels"] == 0).any()          # nobody's voxels, each kind
    assert odd["scan"].min() < TC.LO and odd["scan"].max() >= TC.LO + 16 * TC.WIDTH                        # both clamps


def test_full_box_pair_counts():
    c = TC.case("full_box")
    for d in (1, 2, 4):
        got = gpu_table(c["scan"], c["labels"], 0, None, 1, 16, d)
        assert got.sum(axis=(2, 3))[0].tolist() == TC.box_pairs(c["labels"].shape, d), d


def test_checkerboard_pairs_lie_on_the_face_diagonals_only():
    c = TC.case("checkerboard")
    got = gpu_table(c["scan"], c["labels"], 0, None, 2, 16, 1)
    pairs = got.sum(axis=(2, 3))
    box = TC.box_pairs(c["labels"].shape, 1)
    for d in range(13):
        changes = sum(abs(o) for o in TC.TR.OFFSETS[d])
        assert pairs[:, d].sum() == (box[d] if changes == 2 else 0), d


@pytest.mark.parametrize("kind,n", [(0, 1), (1, 1), (0, 8), (1, 8)])
def test_contention_on_one_entry(kind, n):
    """One label at one grey level over 2^21 voxels: every pair of a direction lands on one entry, in either plan."""
    shape = (32, 256, 256)
    scan = np.full(shape, -640, np.int16)                                # level 4
    labels = np.ones(shape, np.uint8)
    got = gpu_table(scan, labels, kind, None, n, 16, 1)
    ref = np.zeros((n, 13, 16, 16), np.int64)
    ref[0, :, 4, 4] = TC.box_pairs(shape, 1)
    _assert_equal(got, ref, (kind, n))
    assert TC.plan(kind, n, 16, 1) == (0 if n == 1 else 1)


def test_window_parameters():
    """lo, width and levels as the call gives them, a width of one and an extreme lo among them."""
    c = TC.case("odd_u8")
    for lo, width, levels in ((-1300, 1, 32), (0, 1000, 2), (-(1 << 31), 1 << 30, 4), ((1 << 31) - 1, 1, 16), (-32768, 2048, 32)):
        ref = TC.TR.glcm(c["scan"], c["labels"], 3, c["mask"], levels, lo, width, 1)
        _assert_equal(gpu_table(c["scan"], c["labels"], 0, c["mask"], 3, levels, 1, 1, lo=lo, width=width), ref, (lo, width, levels))


def test_refusals_launch_nothing():
    from dram_amd._lib import DramHipError, call, lib
    c = TC.case("odd")
    scan = torch.from_numpy(c["scan"].copy()).cuda()
    labels = torch.from_numpy(c["labels"].copy()).cuda()
    out = torch.full((5 * 13 * 256 + 64,), -7, dtype=torch.int64, device="cuda")

    def args(scan=scan.data_ptr(), lab=labels.data_ptr(), kind=1, mask=None, n=5, lo=-1000, width=75, levels=16, distance=1, glcm=out.data_ptr(),
             D=19, H=21, W=37):
        return (scan, lab, kind, mask, n, lo, width, levels, distance, glcm, D, H, W, _st())

    refused = (dict(scan=None), dict(lab=None), dict(glcm=None), dict(n=0), dict(n=-3), dict(kind=2), dict(kind=-1), dict(kind=0, n=256),
               dict(levels=1), dict(levels=33), dict(distance=0), dict(distance=5), dict(width=0), dict(width=-1), dict(D=0), dict(H=0),
               dict(W=-1), dict(D=32769, H=1, W=1), dict(D=1, H=32769, W=1), dict(D=1, H=1, W=32769), dict(D=2048, H=1024, W=1024),
               dict(n=1 << 21, levels=32), dict(lab=labels.data_ptr() + 1), dict(lab=labels.data_ptr() + 2), dict(scan=scan.data_ptr() + 1))
    for kw in refused:
        assert lib.dram_label_glcm(*args(**kw)) == -1, kw
    with pytest.raises(DramHipError, match="misaligned"):
        call("dram_label_glcm", *args(scan=scan.data_ptr() + 1))
    torch.cuda.synchronize()
    assert bool((out == -7).all())
    # uint8 labels at any address, a scan at any even address
    assert lib.dram_label_glcm(*args(kind=0, lab=labels.data_ptr() + 1, scan=scan.data_ptr() + 2, D=1, H=1, W=3, n=1)) == 0
    torch.cuda.synchronize()
    assert bool((out[:13 * 256] >= 0).all()) and bool((out[13 * 256:] == -7).all())
