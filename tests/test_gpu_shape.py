"""csrc/shape.hip on the device against the numpy restatement (tests/shape_restatement.py, itself held against direct counts and
analytic bodies by tests/test_shape_cpu.py): the tables are integers, so every comparison is exact."""
import numpy as np
import pytest
import torch

import shape_cases as SC

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


def gpu_tables(labels, kind, n, offset):
    """dram_label_shape through the C ABI on guard-banded, poisoned outputs (the entry initialises them)."""
    from dram_amd._lib import call
    lab = SC.as_kind(labels, kind)
    holder, p_labels = _placed(lab, offset)
    out = torch.full((3 * GUARD + n * 266,), -7, dtype=torch.int64, device="cuda")
    cfg = out[GUARD:GUARD + n * 256]
    mom = out[2 * GUARD + n * 256:2 * GUARD + n * 266]
    call("dram_label_shape", p_labels, kind, n, cfg.data_ptr(), mom.data_ptr(), *lab.shape, _st())
    host = out.cpu().numpy()
    del holder
    guards = np.concatenate((host[:GUARD], host[GUARD + n * 256:2 * GUARD + n * 256], host[2 * GUARD + n * 266:]))
    assert np.all(guards == -7), "a guard band was written"
    return {"cfg": host[GUARD:GUARD + n * 256].reshape(n, 256).copy(), "mom": host[2 * GUARD + n * 256:2 * GUARD + n * 266].reshape(n, 10).copy()}


def _assert_tables_equal(got, ref, where):
    for key in ("cfg", "mom"):
        assert got[key].dtype == ref[key].dtype and got[key].shape == ref[key].shape, (where, key)
        bad = np.argwhere(got[key] != ref[key])
        assert bad.size == 0, (where, key, bad[:5].tolist(), [int(got[key][tuple(b)]) for b in bad[:5]], [int(ref[key][tuple(b)]) for b in bad[:5]])


@pytest.mark.parametrize("name", SC.names())
def test_label_shape_matches_the_restatement(name):
    c = SC.case(name)
    seen = set()
    for kind, n in SC.variants(name):
        ref = SC.expected(name, n)
        seen.add(SC.plan(kind, n))
        for offset in (0, 1):                                            # 16-byte loads, and rows off the 16-byte alignment
            got = gpu_tables(c["labels"], kind, n, offset)
            _assert_tables_equal(got, ref, (name, kind, n, offset))
        _assert_tables_equal(gpu_tables(c["labels"], kind, n, 0), got, (name, kind, n, "again"))     # no dependence on the order of the atomics
    assert seen == ({0, 1} if c["n"] < SC.first_n_past_lds() else {1}), seen


def test_both_plans_and_label_kinds_are_exercised():
    seen = {(SC.plan(kind, n), kind) for name in SC.names() for kind, n in SC.variants(name)}
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert SC.plan(1, SC.case("random_i32_300")["n"]) == 1 and SC.plan(0, SC.case("random_u8")["n"]) == 0


def test_refusals_launch_nothing():
    from dram_amd._lib import DramHipError, call, lib
    c = SC.case("random_u8")
    labels = torch.from_numpy(SC.as_kind(c["labels"], 1).copy()).cuda()
    out = torch.full((2, 5 * 256), -7, dtype=torch.int64, device="cuda")

    def args(lab=labels.data_ptr(), kind=1, n=5, cfg=out[0].data_ptr(), mom=out[1].data_ptr(), D=7, H=9, W=11):
        return (lab, kind, n, cfg, mom, D, H, W, _st())

    refused = (dict(lab=None), dict(cfg=None), dict(mom=None), dict(n=0), dict(n=-3), dict(kind=2), dict(kind=-1), dict(kind=0, n=256),
               dict(D=0), dict(H=0), dict(W=-1), dict(D=32769, H=1, W=1), dict(D=1, H=32769, W=1), dict(D=1, H=1, W=32769),
               dict(D=2048, H=1024, W=1024), dict(n=1 << 23), dict(lab=labels.data_ptr() + 1), dict(lab=labels.data_ptr() + 2))
    for kw in refused:
        assert lib.dram_label_shape(*args(**kw)) == -1, kw
    with pytest.raises(DramHipError, match="misaligned"):
        call("dram_label_shape", *args(lab=labels.data_ptr() + 2))
    torch.cuda.synchronize()
    assert bool((out == -7).all())
    assert lib.dram_label_shape(*args(kind=0, lab=labels.data_ptr() + 1, D=1, H=1, W=3, n=1)) == 0      # uint8 labels at any address
    torch.cuda.synchronize()
    assert bool((out[0, :256] >= 0).all()) and bool((out[0, 256:] == -7).all()) and bool((out[1, 10:] == -7).all())
