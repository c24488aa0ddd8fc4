"""The eight kernels of csrc/pcm.hip, each through its C entry point on its own, past one block.

Cases, inputs and the float64 reference: tests/pcm_kernel_cases.py (checked on the host by tests/test_pcm_kernels_cpu.py,
which also shows that a wrong offset, a lost block, a skipped feature plane, an ignored c_lo or a mirrored adjoint moves
the reference by more than ten times the tolerance used here).  Every case runs on 585 nodes (blockIdx.x = 0, 1, 2; the last
block holds 73) and B = 2.

Every output -- ds and ds2 included -- is filled with NaN before the call and sits between guard words: an element that is
not written, or a write outside the tensor, fails.  Exact assertions: non-edge weights and gradients are 0.0, nodes without an
in-grid edge have zero rows in attn, ds and dtheta, every other softmax row sums to 1 within E * 2^-23.

Values: per output tensor against the float64 reference, by the yardstick of tests/test_gpu_oneshot_shapes.py.  e32 is the
error of the same restatement evaluated on the CPU in float32 (max-abs over max |ref|, and relative L2); the kernel must stay
within 4 * e32 in both.  The kernels use fmaf and expf and divide by an accumulated norm in their own order -- a few
roundings either way, where a wrong offset, plane, block or gate is an error of 1e-2 to 1.  No number is fixed in advance:
each case prints a `pcm-accuracy:` line per output before it asserts (profiles/pcm_accuracy.txt is that output of one run).
An output whose reference is identically 0 (ds of relu_split0: nothing lies inside the activation) must be exactly 0.  The
1e-6 floor for e32 == 0 (aggregation with weights of 0 and 1 only) applies to no case of this file: every attn here is a
random tensor, so every e32 is positive.

The backward entry points are given the float32 roundings of the float64 attention and of a random dattn, so that they do not
inherit the forward kernels' error."""
import ctypes
import math

import pytest
import torch

import pcm_kernel_cases as K
from test_gpu_onload import DEV, Placed, call, p, stream

pytestmark = pytest.mark.gpu
EINVAL = -1               # DRAM_EINVAL (include/dram_hip.h)
D, H, W = K.GRID


def offsets_arg(offs):
    flat = [int(v) for o in offs for v in o]
    return (ctypes.c_int * len(flat))(*flat)


def dev(t):
    """float32 on the device.  The caller keeps the tensor: a temporary would be freed, and its memory handed to the next
    operand, before the kernel runs."""
    return t.float().to(DEV).contiguous()


def valid_mask(offs_name):
    """[1, E, D, H, W] bool on the host."""
    return K.Stencil(K.OFFSETS[offs_name], K.GRID).valid().bool()


def finish(*outs):
    torch.cuda.synchronize()
    for o in outs:
        assert o.intact(), "a write outside the tensor"
        assert not bool(torch.isnan(o.t).any()), "an element was not written"
    return [o.t.cpu() for o in outs]


def compare(cid, entry, name, got):
    """One `pcm-accuracy:` line, then kernel error <= 4 * e32 in both measures (exactly 0 for an all-zero reference)."""
    ref64, e32 = K.reference(cid)
    ref = ref64[name]
    if e32[name] is None:
        print(f"pcm-accuracy: {cid:24s} {entry:9s} {name:6s} reference identically 0: HIP max |x| {float(got.abs().max()):.1e}")
        assert float(got.abs().max()) == 0.0, (cid, name)
        return
    k_max, k_l2 = K.errs(got, ref)
    e_max, e_l2 = e32[name]
    print(f"pcm-accuracy: {cid:24s} {entry:9s} {name:6s} HIP max {k_max:.2e} L2 {k_l2:.2e}   CPU-fp32 (e32) max {e_max:.2e} L2 {e_l2:.2e}")
    t_max, t_l2 = K.tolerance(e32[name])
    assert math.isfinite(k_max) and math.isfinite(k_l2), (cid, name)
    assert k_max <= t_max, (cid, name, "max", k_max, e_max)
    assert k_l2 <= t_l2, (cid, name, "L2", k_l2, e_l2)


def rows_of(t, nodes):
    """t [B, C, D, H, W], nodes [D, H, W] bool -> the values at those nodes."""
    return t[:, :, nodes]


# ------------------------------------------------------------------------------------------------ softmax family
@pytest.mark.parametrize("cid", [c.id for c in K.SPLIT_CASES])
def test_attention_split_fwd(cid):
    c = K.CASES[cid]
    offs = K.OFFSETS[c.offs]
    E = len(offs)
    theta, phi = (dev(t) for t in K.split_inputs(cid)[:2])
    attn = Placed((K.B, E, D, H, W))
    call("dram_pcm_attention_split_fwd", p(theta), p(phi), offsets_arg(offs), E, c.flags, c.scale, c.F_relu, p(attn.t),
         K.B, c.F, D, H, W)
    got, = finish(attn)
    valid = valid_mask(c.offs).expand_as(got)
    none = K.edgeless_nodes(c.offs)
    assert float(got[~valid].abs().max()) == 0.0                           # a non-edge has weight exactly 0
    assert float(rows_of(got, none).abs().max() if bool(none.any()) else 0.0) == 0.0
    sums = rows_of(got.double().sum(1, keepdim=True), ~none)
    assert float((sums - 1.0).abs().max()) <= E * 2.0 ** -23
    assert float(got.min()) >= 0.0
    compare(cid, "split_fwd", "attn", got)


@pytest.mark.parametrize("cid", [c.id for c in K.SPLIT_CASES])
def test_attention_split_bwd(cid):
    c = K.CASES[cid]
    offs = K.OFFSETS[c.offs]
    E = len(offs)
    ref64, _ = K.reference(cid)
    theta, phi, dattn, attn = (dev(t) for t in K.split_inputs(cid) + (ref64["attn"],))
    split = K.is_split(c)
    ds, dtheta, dphi = Placed((K.B, E, D, H, W)), Placed((K.B, c.F, D, H, W)), Placed((K.B, c.F, D, H, W))
    ds2 = Placed((K.B, E, D, H, W)) if split else None
    call("dram_pcm_attention_split_bwd", p(theta), p(phi), p(attn), p(dattn), offsets_arg(offs), E,
         c.flags, c.scale, c.F_relu, p(ds.t), p(ds2.t) if split else None, p(dtheta.t), p(dphi.t), K.B, c.F, D, H, W)
    outs = finish(*([ds, dtheta, dphi] + ([ds2] if split else [])))
    got = dict(zip(["ds", "dtheta", "dphi"] + (["ds2"] if split else []), outs))
    valid = valid_mask(c.offs).expand_as(got["ds"])
    none = K.edgeless_nodes(c.offs)
    assert float(got["ds"][~valid].abs().max()) == 0.0
    if split:
        assert float(got["ds2"][~valid].abs().max()) == 0.0
    if bool(none.any()):
        assert float(rows_of(got["ds"], none).abs().max()) == 0.0 and float(rows_of(got["dtheta"], none).abs().max()) == 0.0
    for name in got:
        compare(cid, "split_bwd", name, got[name])


# ------------------------------------------------------------------------------------------------ sum-normalised family
@pytest.mark.parametrize("cid", [c.id for c in K.SUM_CASES])
def test_attention_sum_fwd(cid):
    c = K.CASES[cid]
    offs = K.OFFSETS[c.offs]
    E = len(offs)
    theta, phi = (dev(t) for t in K.sum_inputs(cid)[:2])
    attn = Placed((K.B, E, D, H, W))
    call("dram_pcm_attention_sum_fwd", p(theta), p(phi), offsets_arg(offs), E, c.mode, p(attn.t), K.B, c.F, D, H, W)
    got, = finish(attn)
    valid = valid_mask(c.offs).expand_as(got)
    assert float(got[~valid].abs().max()) == 0.0
    ref64, _ = K.reference(cid)
    if c.mode != K.SUM_COSINE:          # the gate is decided alike: exact zeros where the reference has them, nowhere else
        assert torch.equal(got == 0, ref64["attn"] == 0)
    compare(cid, "sum_fwd", "attn", got)


@pytest.mark.parametrize("cid", [c.id for c in K.SUM_CASES])
def test_attention_sum_bwd(cid):
    """pcm_attn_sum_bwd_kernel and pcm_attn_sum_dphi_kernel; heu1 included, which PcmAttentionSumFn.backward never launches:
    the entry point differentiates u with the 0.03 gate held constant."""
    c = K.CASES[cid]
    offs = K.OFFSETS[c.offs]
    E = len(offs)
    ref64, _ = K.reference(cid)
    theta, phi, dattn, attn = (dev(t) for t in K.sum_inputs(cid) + (ref64["attn"],))
    ds, dtheta, dphi = Placed((K.B, E, D, H, W)), Placed((K.B, c.F, D, H, W)), Placed((K.B, c.F, D, H, W))
    call("dram_pcm_attention_sum_bwd", p(theta), p(phi), p(attn), p(dattn), offsets_arg(offs), E,
         c.mode, p(ds.t), p(dtheta.t), p(dphi.t), K.B, c.F, D, H, W)
    got = dict(zip(["ds", "dtheta", "dphi"], finish(ds, dtheta, dphi)))
    valid = valid_mask(c.offs).expand_as(got["ds"])
    assert float(got["ds"][~valid].abs().max()) == 0.0
    for name in got:
        compare(cid, "sum_bwd", name, got[name])


# ------------------------------------------------------------------------------------------------ aggregation
@pytest.mark.parametrize("cid", ["agg_" + c.id for c in K.AGG_CASES])
def test_aggregate_fwd(cid):
    c = K.CASES[cid]
    offs = K.OFFSETS[c.offs]
    attn, v = (dev(t) for t in K.agg_inputs(cid)[:2])
    out = Placed((K.B, c.C, D, H, W))
    call("dram_pcm_aggregate_fwd", p(attn), p(v), offsets_arg(offs), len(offs), p(out.t), K.B, c.C, D, H, W)
    got, = finish(out)
    none = K.edgeless_nodes(c.offs)
    if bool(none.any()):
        assert float(rows_of(got, none).abs().max()) == 0.0
    compare(cid, "agg_fwd", "out", got)


@pytest.mark.parametrize("cid", ["agg_" + c.id for c in K.AGG_CASES])
def test_aggregate_bwd(cid):
    """pcm_aggregate_dattn_kernel and pcm_scatter_adjoint_kernel with gridDim.y = C."""
    c = K.CASES[cid]
    offs = K.OFFSETS[c.offs]
    E = len(offs)
    attn, v, dout = (dev(t) for t in K.agg_inputs(cid))
    dattn, dv = Placed((K.B, E, D, H, W)), Placed((K.B, c.C, D, H, W))
    call("dram_pcm_aggregate_bwd", p(attn), p(v), p(dout), offsets_arg(offs), E, p(dattn.t), p(dv.t), K.B, c.C,
         D, H, W)
    got = dict(zip(["dattn", "dv"], finish(dattn, dv)))
    valid = valid_mask(c.offs).expand_as(got["dattn"])
    assert float(got["dattn"][~valid].abs().max()) == 0.0
    for name in got:
        compare(cid, "agg_bwd", name, got[name])


# ------------------------------------------------------------------------------------------------ refusals
class Buffers:
    """Device operands of every entry point for F (or C) = 5 planes on the common grid and a table of E offsets; inputs
    finite, outputs NaN between guards."""

    def __init__(self, E=18, planes=5):
        g = torch.Generator().manual_seed(90)
        self.E, self.planes = E, planes
        rnd = lambda n: torch.rand((K.B, n, D, H, W), generator=g).to(DEV)
        self.theta, self.phi, self.attn, self.dattn = rnd(planes), rnd(planes), rnd(E), rnd(E)
        self.out = {k: Placed((K.B, n, D, H, W)) for k, n in
                    (("attn", E), ("ds", E), ("ds2", E), ("dtheta", planes), ("dphi", planes), ("agg", planes))}

    def untouched(self):
        torch.cuda.synchronize()
        return all(o.intact() and bool(torch.isnan(o.t).all()) for o in self.out.values())


def raw(name, *args):
    from dram_amd import _lib
    return getattr(_lib.lib, name)(*args, stream())


def split_fwd(b, offs, E, flags, scale, F_relu, planes):
    return raw("dram_pcm_attention_split_fwd", p(b.theta), p(b.phi), offs, E, flags, scale, F_relu, p(b.out["attn"].t), K.B, planes,
               D, H, W)


def split_bwd(b, offs, E, flags, scale, F_relu, planes, ds2=True):
    return raw("dram_pcm_attention_split_bwd", p(b.theta), p(b.phi), p(b.attn), p(b.dattn), offs, E, flags, scale, F_relu,
               p(b.out["ds"].t), p(b.out["ds2"].t) if ds2 else None, p(b.out["dtheta"].t), p(b.out["dphi"].t), K.B, planes, D, H, W)


def sum_fwd(b, offs, E, planes):
    return raw("dram_pcm_attention_sum_fwd", p(b.theta), p(b.phi), offs, E, K.SUM_HEU2, p(b.out["attn"].t), K.B, planes, D, H, W)


def sum_bwd(b, offs, E, planes):
    return raw("dram_pcm_attention_sum_bwd", p(b.theta), p(b.phi), p(b.attn), p(b.dattn), offs, E, K.SUM_HEU2, p(b.out["ds"].t),
               p(b.out["dtheta"].t), p(b.out["dphi"].t), K.B, planes, D, H, W)


def agg_fwd(b, offs, E, planes):
    return raw("dram_pcm_aggregate_fwd", p(b.attn), p(b.theta), offs, E, p(b.out["agg"].t), K.B, planes, D, H, W)


def agg_bwd(b, offs, E, planes):
    return raw("dram_pcm_aggregate_bwd", p(b.attn), p(b.theta), p(b.phi), offs, E, p(b.out["ds"].t), p(b.out["dtheta"].t), K.B,
               planes, D, H, W)


def test_refusals_launch_nothing():
    """Each refusal returns DRAM_EINVAL and leaves the NaN-filled outputs alone; the valid call that follows succeeds."""
    from dram_amd import _lib
    k3 = K.OFFSETS["k3"]
    good = offsets_arg(k3)
    b = Buffers(E=18, planes=5)
    every = lambda offs, E: [split_fwd(b, offs, E, 0, 1, 5, 5), split_bwd(b, offs, E, 0, 1, 5, 5), sum_fwd(b, offs, E, 5),
                             sum_bwd(b, offs, E, 5), agg_fwd(b, offs, E, 5), agg_bwd(b, offs, E, 5)]
    # 129 offsets (the buffers of `big` hold 129 planes, so that even an accepted call would stay inside them)
    big = Buffers(E=129, planes=5)
    many = offsets_arg([k3[i % 18] for i in range(129)])
    big_calls = [split_fwd(big, many, 129, 0, 1, 5, 5), split_bwd(big, many, 129, 0, 1, 5, 5), sum_fwd(big, many, 129, 5),
                 sum_bwd(big, many, 129, 5), agg_fwd(big, many, 129, 5), agg_bwd(big, many, 129, 5)]
    assert big_calls == [EINVAL] * 6 and big.untouched()
    assert b"1..128" in _lib.lib.dram_last_error()
    # an offset component of 128 (does not fit the table's signed char)
    far = offsets_arg([(0, 0, 128)] + k3[1:])
    assert every(far, 18) == [EINVAL] * 6 and b.untouched()
    assert b"offset out of range" in _lib.lib.dram_last_error()
    # F = 65 on both sum entry points (acc[PCM_SUM_MAXF = 64] per thread)
    wide = Buffers(E=18, planes=65)
    assert sum_fwd(wide, good, 18, 65) == EINVAL and sum_bwd(wide, good, 18, 65) == EINVAL and wide.untouched()
    assert sum_fwd(wide, good, 18, 64) == 0 and sum_bwd(wide, good, 18, 64) == 0      # the limit itself is accepted
    # F_relu > F
    assert split_fwd(b, good, 18, K.PCM_RELU, 1, 6, 5) == EINVAL and split_bwd(b, good, 18, K.PCM_RELU, 1, 6, 5) == EINVAL
    # L2 normalisation together with F_relu < F
    assert split_fwd(b, good, 18, K.PCM_L2NORM, 0, 3, 5) == EINVAL and split_bwd(b, good, 18, K.PCM_L2NORM, 0, 3, 5) == EINVAL
    assert split_fwd(b, good, 18, K.PCM_L2NORM | K.PCM_RELU, 0, 3, 5) == EINVAL
    assert split_bwd(b, good, 18, K.PCM_L2NORM | K.PCM_RELU, 0, 3, 5) == EINVAL
    # a split backward without ds2
    assert split_bwd(b, good, 18, K.PCM_RELU, 1, 3, 5, ds2=False) == EINVAL
    assert b"ds2" in _lib.lib.dram_last_error()
    assert b.untouched()
    # the valid calls that follow succeed and write everything
    assert every(good, 18) == [0] * 6
    assert split_bwd(b, good, 18, K.PCM_RELU, 1, 3, 5) == 0
    assert split_bwd(b, good, 18, 0, 1, 3, 5, ds2=False) == 0             # no activation: no split, ds2 may be null
    torch.cuda.synchronize()
    for name, o in b.out.items():
        assert o.intact() and not bool(torch.isnan(o.t).any()), name
