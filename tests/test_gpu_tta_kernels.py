"""The three kernels of csrc/infer_tta.hip, each through its C entry point on its own.

Cases, inputs, the fp64 reference and the derived tolerances: tests/tta_cases.py (checked on the host by tests/test_tta_cpu.py,
which also shows that the forward move in place of the inverse, dropped flips, averaged logits, a division by V - 1 and a
paste without the lobe test each move the reference by more than ten of the tolerances used here).  R = 12 with L = 3 and
R = 10 with L = 8: R^3 is no multiple of a block, the 8 x 8 x 16 boxes are cut on every axis, and 8 chunks x 48 views are 384
chunk-views.  Every output is filled with NaN before the call and sits between guard words.

Each case prints a `tta-accuracy:` line with the largest measured ratio to its bound before it asserts
(profiles/tta_accuracy.txt is that output of one run).

The equivariant cases (every view shows the same probabilities) pin the order of the sums: over the header's binary tree of
the view index 2, 4 and 8 equal values give the single value bit for bit, 3 and 48 stay within 2 ulp, and the kernel's mean
equals the same tree evaluated in fp32 on the host (tta_cases.tree_sum32) bit for bit.  Added left to right, 8 equal values
are no longer exact and 48 are up to 11 ulp off at these inputs."""
import ctypes

import numpy as np
import pytest
import torch

import tta_cases as T
from test_gpu_onload import DEV, Placed, call, p, stream

pytestmark = pytest.mark.gpu
U = T.U


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)          # (a C-ordered copy: the shared inputs are read-only)


def finish(*outs, nan_ok=False):
    torch.cuda.synchronize()
    for o in outs:
        assert o.intact(), "a write outside the tensor"
        assert nan_ok or not bool(torch.isnan(o.t).any()), "an element was not written"
    return [o.t.cpu().numpy() for o in outs]


def report(line):
    print("tta-accuracy: " + line)


def run_combine(dense, views, with_spread=True):
    V, L, R = dense.shape[0], dense.shape[1], dense.shape[-1]
    assert V == len(views)
    d = dev(dense.reshape(V, L, 1, R, R, R))
    mean, spread = Placed((L, R, R, R)), Placed((L, R, R, R)) if with_spread else None
    call("dram_tta_combine", p(d), p(mean.t), p(spread.t) if with_spread else None, L, R, T.views_arg(views), V)
    outs = finish(*([mean, spread] if with_spread else [mean]))
    return outs if with_spread else (outs[0], None)


def device_sigmoid(logits):
    """[L, R, R, R] -> the fp32 sigmoid that dram_lobe_paste computes: chunk l is an R^3 box of a volume in which every voxel
    carries its label, so the align-corners resize is the identity (scale 1, weights 1 and 0) and what is pasted is the
    sigmoid itself."""
    L, R = logits.shape[0], logits.shape[-1]
    lobe = np.repeat(np.arange(1, L + 1, dtype=np.uint8), R * R * R).reshape(L * R, R, R)
    chunks = [v for l in range(L) for v in (l * R, 0, 0, R, R, R, l + 1)]
    d, lobe_d = dev(logits), dev(lobe)
    htp = Placed((L * R, R, R))
    call("dram_lobe_paste", p(d), p(lobe_d), p(htp.t), (ctypes.c_int * len(chunks))(*chunks), L, L * R, R, R, R)
    return finish(htp)[0].reshape(L, R, R, R)


# ------------------------------------------------------------------------------------------------ expand
@pytest.mark.parametrize("R,L", T.SHAPES)
def test_expand_is_permute_flip_bit_for_bit(R, L):
    V = len(T.FULL_VIEWS)
    x = np.random.default_rng(7 + R).standard_normal((L, 1, R, R, R)).astype(np.float32)
    x_d = dev(x)
    xv = Placed((V, L, 1, R, R, R))
    call("dram_tta_expand", p(x_d), p(xv.t), L, R, T.views_arg(T.FULL_VIEWS), V)
    got, = finish(xv)
    one = Placed((L, 1, R, R, R))
    for v, (perm, flip) in enumerate(T.FULL_VIEWS):
        one.t.fill_(float("nan"))
        call("dram_spatial_permute_flip", p(x_d), p(one.t), L, 1, R, R, R, (ctypes.c_int * 3)(*perm), (ctypes.c_int * 3)(*flip))
        ref, = finish(one)
        assert np.array_equal(got[v].view(np.uint32), ref.view(np.uint32)), (v, perm, flip)
        assert np.array_equal(got[v], T.apply_view(x, (perm, flip))), (v, perm, flip)


def test_expand_repeated_views_and_one_view():
    R, L = 12, 2
    x = np.random.default_rng(9).standard_normal((L, 1, R, R, R)).astype(np.float32)
    x_d = dev(x)
    for views in ((T.CYCLE_VIEW,), (T.CYCLE_VIEW, T.IDENTITY, T.CYCLE_VIEW)):
        xv = Placed((len(views), L, 1, R, R, R))
        call("dram_tta_expand", p(x_d), p(xv.t), L, R, T.views_arg(views), len(views))
        got, = finish(xv)
        for v, view in enumerate(views):
            assert np.array_equal(got[v], T.apply_view(x, view))


# ------------------------------------------------------------------------------------------------ combine
@pytest.mark.parametrize("R,L", T.SHAPES)
def test_combine_one_identity_view_is_the_paste_sigmoid(R, L):
    base = T.base_logits(R, L)
    m, s = run_combine(base[None], (T.IDENTITY,))
    assert np.array_equal(m.view(np.uint32), device_sigmoid(base).view(np.uint32))
    assert not s.any()
    m2, _ = run_combine(base[None], (T.IDENTITY,), with_spread=False)
    assert np.array_equal(m, m2)
    ref_m, _, _ = T.combine_ref(base[None], (T.IDENTITY,))
    report(f"combine R={R} L={L} V=1 identity: mean {np.abs(m - ref_m).max() / T.mean_tol(1):.3f} of mean_tol, spread exactly 0")
    assert np.abs(m - ref_m).max() <= T.mean_tol(1)


@pytest.mark.parametrize("R,L", T.SHAPES)
@pytest.mark.parametrize("V", sorted(T.EQUIVARIANT_EXACT))
def test_combine_equivariant_power_of_two_is_exact(V, R, L):
    """dense[v] = view_v(dense[0]): V equal probabilities.  A sum of 2, 4 or 8 equal values and a division by a power of two
    are exact: m is the V = 1 result bit for bit and s == 0."""
    views = T.EQUIVARIANT_EXACT[V]
    assert len(views) == V and any(v[0][2] != 2 for v in views)
    m1, _ = run_combine(T.base_logits(R, L)[None], (T.IDENTITY,))
    m, s = run_combine(T.equivariant_dense(R, L, views), views)
    assert np.array_equal(m.view(np.uint32), m1.view(np.uint32))
    assert not s.any()


@pytest.mark.parametrize("R,L", T.SHAPES)
@pytest.mark.parametrize("V", sorted(T.EQUIVARIANT_ULP))
def test_combine_equivariant_within_2_ulp(V, R, L):
    views = T.EQUIVARIANT_ULP[V]
    m1, _ = run_combine(T.base_logits(R, L)[None], (T.IDENTITY,))
    dense = T.equivariant_dense(R, L, views)
    m, s = run_combine(dense, views)
    ref_m, ref_var, _ = T.combine_ref(dense, views)
    seq = T.tree_sum32([m1] * V) / np.float32(V)            # the definition's own sequence, in fp32 on the host
    ulps = np.abs(m.astype(np.float64) - m1) / np.spacing(m1)
    report(f"combine R={R} L={L} V={V} equivariant: mean off the V=1 result by {ulps.max():.0f} ulp at most (asked: 2), "
           f"{np.abs(m - ref_m).max() / T.mean_tol(V):.3f} of mean_tol, s^2 {np.abs(s.astype(np.float64) ** 2 - ref_var).max() / T.var_tol(V):.2e} "
           f"of var_tol, equal to the host's fp32 sequence: {np.array_equal(m, seq)}")
    assert np.array_equal(m.view(np.uint32), seq.view(np.uint32))
    assert np.abs(m - ref_m).max() <= T.mean_tol(V)
    assert np.abs(s.astype(np.float64) ** 2 - ref_var).max() <= T.var_tol(V)
    assert ulps.max() <= 2


@pytest.mark.parametrize("R,L", T.SHAPES)
@pytest.mark.parametrize("name", sorted(T.RANDOM_CASES))
def test_combine_random_views(name, R, L):
    """Independent logits per view in [-12, 12] with +-40 planted; all 48 views, the 8 flips, only views that move x, only views
    that keep x, a repeated 3-cycle, and 11 views (a group of three left over after two groups of four)."""
    views = T.RANDOM_CASES[name]
    V = len(views)
    dense = T.random_dense(R, L, name)
    assert (np.abs(dense) == 40).sum() >= 8
    ref_m, ref_var, ref_s = T.random_reference(R, L, name)
    m, s = run_combine(dense, views)
    e_m = np.abs(m - ref_m).max() / T.mean_tol(V)
    e_v = np.abs(s.astype(np.float64) ** 2 - ref_var).max() / T.var_tol(V)
    big = ref_s >= T.S_MIN
    e_s = (np.abs(s - ref_s)[big] / T.spread_tol(V, ref_s[big])).max()
    report(f"combine R={R} L={L} {name:10s} V={V:2d}: mean {e_m:.3f} of mean_tol, s^2 {e_v:.3f} of var_tol, s {e_s:.3f} of spread_tol "
           f"on {int(big.sum())} of {big.size} points with s >= 2^-8")
    assert big.sum() > big.size // 2
    assert e_m <= 1 and e_v <= 1 and e_s <= 1
    assert m.min() >= 0 and m.max() <= 1 and s.min() >= 0 and s.max() <= 0.5 + U
    m2, _ = run_combine(dense, views, with_spread=False)            # spread = NULL: the same mean
    assert np.array_equal(m.view(np.uint32), m2.view(np.uint32))


# ------------------------------------------------------------------------------------------------ paste of probabilities
def chunks_arg(chunks):
    flat = [int(v) for c in chunks for v in c]
    return (ctypes.c_int * len(flat))(*flat)


def run_paste_prob(prob, prob2, lobe):
    D, H, W = T.VOLUME
    L = len(T.PASTE_CHUNKS)
    prob_d, prob2_d, lobe_d = dev(prob), None if prob2 is None else dev(prob2), dev(lobe)
    htp, htp2 = Placed(T.VOLUME), None if prob2 is None else Placed(T.VOLUME)
    call("dram_lobe_paste_prob", p(prob_d), p(prob2_d), p(lobe_d), p(htp.t), None if htp2 is None else p(htp2.t),
         chunks_arg(T.PASTE_CHUNKS), L, D, H, W, T.PASTE_R)
    return finish(*([htp] if htp2 is None else [htp, htp2]), nan_ok=True)


def test_paste_prob_two_fields():
    prob, prob2, lobe = T.paste_prob_inputs()
    got = run_paste_prob(prob, prob2, lobe)
    nan0 = np.full(T.VOLUME, np.nan)
    for name, field, out in (("mean", prob, got[0]), ("spread", prob2, got[1])):
        ref, written = T.paste_prob_ref(field, lobe, T.PASTE_CHUNKS, T.PASTE_R, nan0)
        assert written.sum() > 600 and (~written).sum() > 1000
        assert np.array_equal(np.isnan(out), ~written)            # outside the lobe or every chunk: the NaN fill stays
        err = np.abs(out[written] - ref[written]).max()
        report(f"paste_prob {name}: {err / T.RESIZE_TOL:.3f} of RESIZE_TOL on {int(written.sum())} voxels")
        assert err <= T.RESIZE_TOL
    one, = run_paste_prob(prob, None, lobe)                       # one field: the same values
    assert np.array_equal(one.view(np.uint32), got[0].view(np.uint32))


def test_paste_prob_of_the_sigmoid_is_lobe_paste():
    dense, lobe, _ = T.K.paste_inputs()
    D, H, W = T.VOLUME
    got, = run_paste_prob(T.sigmoid32(dense), None, lobe)
    dense_d, lobe_d = dev(dense), dev(lobe)
    htp = Placed(T.VOLUME)
    call("dram_lobe_paste", p(dense_d), p(lobe_d), p(htp.t), chunks_arg(T.PASTE_CHUNKS), len(T.PASTE_CHUNKS), D, H, W, T.PASTE_R)
    ref, = finish(htp, nan_ok=True)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    w = ~np.isnan(ref)
    err = np.abs(got[w].astype(np.float64) - ref[w]).max()
    same = np.array_equal(got[w].view(np.uint32), ref[w].view(np.uint32))
    report(f"paste_prob(host fp32 sigmoid) against lobe_paste: {err / (2 * U):.3f} of 2 U, bit-identical: {same}")
    assert err <= 2 * U


# ------------------------------------------------------------------------------------------------ refusals
R0, L0 = 12, 3
GOOD = [T.IDENTITY, T.CYCLE_VIEW]
BAD_VIEWS = {"V=0": ([], 0), "V=49": (list(T.FULL_VIEWS) + [T.IDENTITY], 49),
             "perm repeats": ([T.IDENTITY, ((0, 1, 1), (0, 0, 0))], 2), "perm out of range": ([((0, 1, 3), (0, 0, 0))], 1),
             "perm negative": ([((0, -1, 2), (0, 0, 0))], 1), "flip 2": ([T.IDENTITY, ((0, 1, 2), (0, 2, 0))], 2),
             "flip -1": ([((0, 1, 2), (-1, 0, 0))], 1)}


def refused(name, *args):
    from dram_amd import _lib
    rc = getattr(_lib.lib, name)(*args, stream())
    msg = _lib.lib.dram_last_error()
    assert rc != 0 and msg, (name, rc, msg)


@pytest.mark.parametrize("entry", ["dram_tta_expand", "dram_tta_combine"])
def test_view_entry_refusals(entry):
    x = dev(np.zeros((len(T.FULL_VIEWS), L0, 1, R0, R0, R0), dtype=np.float32))
    out, out2 = Placed((49, L0, 1, R0, R0, R0)), Placed((L0, R0, R0, R0))

    def attempt(src, dst, L, R, views, V, dst2=out2):
        arg = T.views_arg(views) if views else None
        if entry == "dram_tta_expand":
            refused(entry, p(src), p(dst.t) if dst else None, L, R, arg, V)
        else:
            refused(entry, p(src), p(dst.t) if dst else None, p(dst2.t) if dst2 else None, L, R, arg, V)

    for views, V in BAD_VIEWS.values():
        attempt(x, out, L0, R0, views or GOOD, V)
    for L, R in ((0, R0), (9, R0), (-1, R0), (L0, 1), (L0, 0)):
        attempt(x, out, L, R, GOOD, 2)
    attempt(None, out, L0, R0, GOOD, 2)
    attempt(x, None, L0, R0, GOOD, 2)
    attempt(x, out, L0, R0, None, 2)
    torch.cuda.synchronize()
    for o in (out, out2):
        assert o.intact() and bool(torch.isnan(o.t).all())        # nothing was written between the guards either


def test_paste_prob_refusals():
    prob, prob2, lobe = T.paste_prob_inputs()
    D, H, W = T.VOLUME
    L = len(T.PASTE_CHUNKS)
    prob_d, prob2_d, lobe_d = dev(prob), dev(prob2), dev(lobe)
    htp, htp2 = Placed(T.VOLUME), Placed(T.VOLUME)
    good = chunks_arg(T.PASTE_CHUNKS)
    nine = chunks_arg([T.PASTE_CHUNKS[0]] * 9)
    outside = chunks_arg(((3, 10, 8, 5, 20, 40, 1),))
    for args in ((p(prob_d), p(prob2_d), p(lobe_d), p(htp.t), p(htp2.t), good, 0, D, H, W, T.PASTE_R),
                 (p(prob_d), p(prob2_d), p(lobe_d), p(htp.t), p(htp2.t), nine, 9, D, H, W, T.PASTE_R),
                 (p(prob_d), p(prob2_d), p(lobe_d), p(htp.t), p(htp2.t), good, L, D, H, W, 1),
                 (p(prob_d), p(prob2_d), p(lobe_d), p(htp.t), p(htp2.t), outside, 1, D, H, W, T.PASTE_R),
                 (None, p(prob2_d), p(lobe_d), p(htp.t), p(htp2.t), good, L, D, H, W, T.PASTE_R),
                 (p(prob_d), p(prob2_d), None, p(htp.t), p(htp2.t), good, L, D, H, W, T.PASTE_R),
                 (p(prob_d), p(prob2_d), p(lobe_d), None, p(htp2.t), good, L, D, H, W, T.PASTE_R),
                 (p(prob_d), p(prob2_d), p(lobe_d), p(htp.t), None, good, L, D, H, W, T.PASTE_R),
                 (p(prob_d), None, p(lobe_d), p(htp.t), p(htp2.t), good, L, D, H, W, T.PASTE_R),
                 (p(prob_d), p(prob2_d), p(lobe_d), p(htp.t), p(htp2.t), None, L, D, H, W, T.PASTE_R)):
        refused("dram_lobe_paste_prob", *args)
    torch.cuda.synchronize()
    for o in (htp, htp2):
        assert o.intact() and bool(torch.isnan(o.t).all())
