"""GPU tests of the SegOverlap kernels (dram_seg_overlap_fwd / _bwd of csrc/loss.hip: per-sample Tversky + focal on logits)
through the C ABI, on guard-banded, NaN-poisoned buffers (tests/gpu_buffers.py), against the numpy fp64 restatement of the
header's text (tests/seg_overlap_restatement.py, pinned to torch's autograd by tests/test_seg_overlap_cpu.py).

Shapes: N=2, S=7 (below one 16-byte group: the ragged path alone); N=3, S=SEG_CHUNK+5 (two blocks per sample, a block edge
at every sample edge, a ragged tail, samples 1 and 2 starting off a 16-byte boundary); N=1, S=3*SEG_CHUNK (whole blocks).

Bounds (the SegOverlap item, derives them from the kernel's operation chain; u = 2^-24).  Per call,
the limits the device math library is built to: expf 3 ulp = 6u, log1pf 2 ulp = 4u; every other fp32 operation, the
correctly rounded division included, 1u.
  p, q                      K_P = 12     e = expf(-|z|) 6, 1 + e 1, 1 / . 1 and half of e's 6, times e 6 + 1
  a group of four in fp32   K_SUM = 3    three additions before the fp64 accumulator (sums are fp64 from there on)
  TP, SP                    15 u sum     K_P + K_SUM; ST and M are integers and compare with ==
  -log p_t, -log(1 - p_t)   11           l = log1pf(e): 6 + 4; max(., 0) + l: 1
  alpha_t (1 - p_t)^gamma   8 + 7 gamma + 2 x      x = gamma (-log(1 - p_t)) the exponential's argument, its absolute error
                                         (7 gamma + 2 x) u; expf 6; alpha_t and the product 2
  focal term, in its sum    K_F(x) = 23 + 7 gamma + 2 x     the above, 11, the product 1, K_SUM
  gout[1] d out[1] / dz     K_B(x) = 38 + 7 gamma + 2 x     the inner sum 26 and its product 1, 1 / (N M) rounded and multiplied 2, gout 1
  gout[0] d out[0] / dz     K_A = 28     p q 25, the coefficient's rounding, two products; plus the coefficient's own error
x differs per voxel, so a sum of focal terms is held to u sum_i K_F(x_i) |f_i| (terms with a large x are the ones that
vanish).  The Tversky index and the backward's two coefficients are functions of TP and SP: their bound is the closed
form evaluated at TP (1 +- 15u), SP (1 +- 15u).  One more u for each final fp32 rounding (out, state, the last addition of
dz).  Below fp32's normal range (2^-126) only the magnitude is asked.  Nothing here comes from a measurement; the largest
measured ratio error / bound is printed by every test and recorded in DESIGN.md."""
import itertools

import numpy as np
import pytest
import torch

import seg_overlap_restatement as R
from gpu_buffers import Placed, call, p as ptr

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
TINY = 2.0 ** -126
EPS64 = 2.0 ** -50                # the restatement's own fp64 rounding where it forms 1 - TI, a value of order 1
K_P, K_SUM, K_A = 12, 3, 28
CHUNK = 4096                     # dram_seg_loss_chunk(), asserted below
SHAPES = [(2, 7), (3, CHUNK + 5), (1, 3 * CHUNK)]
AB = [(.5, .5), (.3, .7), (0.0, 1.0)]
GAMMA = [0.0, 1.0, 2.0, 1.5]
ALPHA = [0.0, .25, 1.0]
SMOOTH = 1.0
GOUT = (0.75, -1.5)
KINDS = {torch.uint8: 0, torch.float32: 2}
WORST = {}


def k_f(x, gamma):
    return 23 + 7 * gamma + 2 * x


def k_b(x, gamma):
    return 38 + 7 * gamma + 2 * x


def _note(name, err, tol):
    r = float(np.max(np.asarray(err) / np.asarray(tol)))
    WORST[name] = max(WORST.get(name, 0.0), r)
    return r


def _data(N, S, logits, seed):
    """z, t, voi as numpy ([N, S]; t and voi boolean).  Sample 1 (where there is one) has an empty volume of interest; t is
    set outside the voi too, where it must not count."""
    g = torch.Generator().manual_seed(seed)
    if logits == "normal":
        z = torch.randn(N, S, generator=g)
    else:
        z = torch.where(torch.rand(N, S, generator=g) < 0.5, 100.0, -100.0)
    voi = torch.rand(N, S, generator=g) < 0.6
    t = torch.rand(N, S, generator=g) < 0.3
    voi[:, 0], voi[:, -1], t[:, 0], t[:, -1] = True, True, True, False      # the first and last voxel of a sample count
    if N > 1:
        voi[1] = False
    return z.numpy(), t.numpy(), voi.numpy()


def _place(a, dtype, shift):
    return Placed(a.shape, shift * torch.empty((), dtype=dtype).element_size(), dtype=dtype, src=torch.from_numpy(a).to(dtype))


class Run:
    """One forward and backward through the C ABI on placed buffers; everything read back."""

    def __init__(self, z, t, voi, prm, t_dtype=torch.float32, v_dtype=torch.float32, shift=1, gout=GOUT):
        from dram_amd import _lib
        N, S = z.shape
        a, b, alpha, gamma = prm
        zp, tp = _place(z, torch.float32, shift), _place(t, t_dtype, shift)
        vp = None if voi is None else _place(voi, v_dtype, shift)
        out, state = Placed((2,), 4 * shift), Placed((_lib.lib.dram_seg_overlap_state_floats(N),), 4 * shift)
        nws = _lib.lib.dram_seg_overlap_ws_bytes(N, S)
        assert nws == N * (8 + 5 * -(-S // CHUNK)) * 8
        ws = Placed((nws // 8,), 0, dtype=torch.float64)
        dz = Placed((N, S), 4 * shift)
        gp = Placed((2,), 4 * shift, src=torch.tensor(gout))
        vptr, kv = (None, 0) if vp is None else (ptr(vp.t), KINDS[v_dtype])
        call("dram_seg_overlap_fwd", ptr(zp.t), ptr(tp.t), vptr, KINDS[t_dtype], kv, N, S, a, b, SMOOTH, alpha, gamma,
             ptr(out.t), ptr(state.t), ptr(ws.t), nws)
        call("dram_seg_overlap_bwd", ptr(zp.t), ptr(tp.t), vptr, KINDS[t_dtype], kv, N, S, alpha, gamma, ptr(state.t),
             ptr(gp.t), ptr(dz.t))
        torch.cuda.synchronize()
        self.intact = all(x.intact() for x in (zp, tp, out, state, ws, dz, gp) + (() if vp is None else (vp,)))
        self.inputs_kept = torch.equal(zp.t.cpu(), torch.from_numpy(z)) or bool(np.isnan(z).any())
        self.out, self.state, self.dz = out.t.cpu().numpy(), state.t.cpu().numpy().reshape(N, 5), dz.t.cpu().numpy()
        self.tot = ws.t.cpu().numpy()[:8 * N].reshape(N, 8)

    def bits(self):
        return tuple(x.tobytes() for x in (self.out, self.state, self.dz, self.tot))


def _corners(fn, tot):
    """max |fn(TP', SP') - fn(TP, SP)| over TP' = TP (1 +- 15u), SP' = SP (1 +- 15u): what the error of the two fp32-fed sums
    does to a function of the totals."""
    base, dev = fn(tot), 0.0
    for sa, sb in itertools.product((-1, 1), repeat=2):
        alt = tot.copy()
        alt[:, 0] *= 1 + sa * (K_P + K_SUM) * U
        alt[:, 1] *= 1 + sb * (K_P + K_SUM) * U
        dev = np.maximum(dev, np.abs(fn(alt) - base))
    return dev


def _check(run, z, t, voi, prm, gout=GOUT):
    """Hold one run to the restatement within the bounds of the module docstring; returns the ratios error / bound."""
    a, b, alpha, gamma = prm
    N, S = z.shape
    v = np.ones_like(t) if voi is None else voi
    assert run.intact and run.inputs_kept
    assert np.isfinite(run.out).all() and np.isfinite(run.state).all() and np.isfinite(run.dz).all() and np.isfinite(run.tot).all()
    tot = R.totals(z, t, voi, alpha, gamma)
    _, _, f, x = R.voxel_terms(z.astype(np.float64), t, alpha, gamma)
    fbound = U * np.where(v, k_f(x, gamma) * np.abs(f), 0.0).sum(-1) + S * TINY
    # totals: the two counts are THE integers
    assert (run.tot[:, 2] == tot[:, 2]).all() and (run.tot[:, 3] == tot[:, 3]).all() and (run.tot[:, 7] == 0).all()
    r = {"TP": _note("TP", np.abs(run.tot[:, 0] - tot[:, 0]), (K_P + K_SUM) * U * tot[:, 0] + S * TINY),
         "SP": _note("SP", np.abs(run.tot[:, 1] - tot[:, 1]), (K_P + K_SUM) * U * tot[:, 1] + S * TINY),
         "FS": _note("FS", np.abs(run.tot[:, 4] - tot[:, 4]), fbound)}
    # per-sample terms and coefficients, and out
    loss_n, F_n = R.sample_terms(tot, a, b, SMOOTH)
    dloss = _corners(lambda w: R.sample_terms(w, a, b, SMOOTH)[0], tot) + EPS64
    M = np.maximum(tot[:, 3], 1.0)
    cs, cu = R.tversky_coefficients(tot, a, b, SMOOTH)
    dcs = _corners(lambda w: R.tversky_coefficients(w, a, b, SMOOTH)[0], tot)
    dcu = _corners(lambda w: R.tversky_coefficients(w, a, b, SMOOTH)[1], tot)
    cf = np.where(tot[:, 3] > 0, 1.0 / (N * M), 0.0)
    r["loss_n"] = _note("loss_n", np.abs(run.state[:, 0] - loss_n), dloss + U * np.abs(loss_n) + TINY)
    r["F_n"] = _note("F_n", np.abs(run.state[:, 1] - F_n), fbound / M + U * np.abs(F_n) + TINY)
    r["c_set"] = _note("c_set", np.abs(run.state[:, 2] - cs), dcs + U * np.abs(cs) + TINY)
    r["c_unset"] = _note("c_unset", np.abs(run.state[:, 3] - cu), dcu + U * np.abs(cu) + TINY)
    assert np.abs(run.state[:, 4] - cf).max() <= U * cf.max() + TINY
    assert (np.abs(run.tot[:, 5] - loss_n) <= dloss + TINY).all() and (np.abs(run.tot[:, 6] - F_n) <= fbound / M).all()
    want = R.seg_overlap(z, t, voi, a, b, SMOOTH, alpha, gamma)
    r["out0"] = _note("out0", abs(run.out[0] - want[0]), dloss.sum() + U * abs(want[0]) + TINY)
    r["out1"] = _note("out1", abs(run.out[1] - want[1]), (fbound / M).sum() / N + U * abs(want[1]) + TINY)
    # dz: per element; exactly +0 (not -0) outside the volume of interest
    d0, d1, xg = R.seg_overlap_grad_parts(z, t, voi, a, b, SMOOTH, alpha, gamma)
    A, B = np.abs(gout[0] * d0), np.abs(gout[1] * d1)
    rel_c = np.where(t, (dcs / np.maximum(np.abs(cs), TINY))[:, None], (dcu / np.maximum(np.abs(cu), TINY))[:, None])
    bound = U * ((K_A + 1) * A + (k_b(xg, gamma) + 1) * B) + rel_c * A + TINY
    ref = gout[0] * d0 + gout[1] * d1
    outside = ~v
    assert (run.dz[outside].view(np.uint32) == 0).all()
    r["dz"] = _note("dz", np.abs(run.dz - ref)[v], bound[v]) if v.any() else 0.0
    assert max(r.values()) <= 1.0, (prm, r)
    return r


def test_constants():
    from dram_amd import _lib
    assert _lib.lib.dram_seg_loss_chunk() == CHUNK and _lib.lib.dram_seg_overlap_state_floats(3) == 15


@pytest.mark.parametrize("with_voi", [True, False], ids=["voi", "novoi"])
@pytest.mark.parametrize("logits", ["normal", "pm100"])
@pytest.mark.parametrize("N,S", SHAPES)
def test_matches_the_restatement_for_every_parameter(N, S, logits, with_voi):
    """Every (a, b) x gamma x alpha of the issue's table, base pointers one element off a 16-byte boundary, float32 masks;
    where a voi is given, a NaN logit and an infinite one outside it must not reach any result."""
    z, t, voi = _data(N, S, logits, seed=N * 1000 + S)
    if with_voi:
        out_idx = np.argwhere(~voi)
        z[tuple(out_idx[0])], z[tuple(out_idx[-1])] = np.nan, np.inf
    else:
        voi = None
    worst, second = {}, None
    for (a, b), gamma, alpha in itertools.product(AB, GAMMA, ALPHA):
        prm = (a, b, alpha, gamma)
        run = Run(z, t, voi, prm)
        for k, v in _check(run, z, t, voi, prm).items():
            worst[k] = max(worst.get(k, 0.0), v)
        if second is None:
            second = Run(z, t, voi, prm)
            assert second.bits() == run.bits()                     # a second run: the same bits
    print(f"N={N} S={S} {logits} voi={with_voi}: largest error / bound", {k: round(v, 4) for k, v in worst.items()})
    print("so far over the file:", {k: round(v, 4) for k, v in WORST.items()})


@pytest.mark.parametrize("logits", ["normal", "pm100"])
@pytest.mark.parametrize("N,S", SHAPES)
def test_same_bits_for_every_mask_kind_and_alignment(N, S, logits):
    """uint8 and float32 masks in every pairing, aligned bases and bases one element off; a NULL voi against a voi of ones."""
    z, t, voi = _data(N, S, logits, seed=N * 1000 + S + 1)
    ones = np.ones_like(voi)
    for prm in ((.5, .5, .25, 2.0), (.3, .7, 1.0, 1.5)):
        base = Run(z, t, voi, prm, shift=0)
        _check(base, z, t, voi, prm)
        for td, vd, shift in itertools.product((torch.uint8, torch.float32), (torch.uint8, torch.float32), (0, 1)):
            other = Run(z, t, voi, prm, td, vd, shift)
            assert other.intact and other.bits() == base.bits(), (td, vd, shift)
        null = Run(z, t, None, prm, shift=0)
        _check(null, z, t, None, prm)
        for td, vd, shift in ((torch.uint8, torch.uint8, 1), (torch.float32, torch.float32, 0), (torch.uint8, None, 1)):
            other = Run(z, t, None if vd is None else ones, prm, td, vd or torch.float32, shift)
            assert other.intact and other.bits() == null.bits(), (td, vd, shift)


def test_non_binary_masks_count_as_set_and_gout_scales_by_powers_of_two_exactly():
    N, S = 3, CHUNK + 5
    z, t, voi = _data(N, S, "normal", seed=5)
    prm = (.3, .7, .25, 2.0)
    base = Run(z, t, voi, prm)
    g = torch.Generator().manual_seed(6)
    tf = np.where(t, (torch.rand(N, S, generator=g).numpy() + 0.5) * np.where(torch.rand(N, S, generator=g).numpy() < .5, -1, 1), 0.0)
    vf = np.where(voi, torch.rand(N, S, generator=g).numpy() * 1e-3 + 1e-30, 0.0).astype(np.float32)
    t8, v8 = np.where(t, 200, 0).astype(np.uint8), np.where(voi, 3, 0).astype(np.uint8)
    assert Run(z, tf.astype(np.float32), vf, prm).bits() == base.bits()
    assert Run(z, t8, v8, prm, torch.uint8, torch.uint8).bits() == base.bits()
    # the products with gout come last: a power of two scales every element exactly, and a zero gout[1] leaves gout[0]'s part
    double = Run(z, t, voi, prm, gout=(2 * GOUT[0], 2 * GOUT[1]))
    assert (double.dz == 2 * base.dz).all()
    first, second = Run(z, t, voi, prm, gout=(GOUT[0], 0.0)), Run(z, t, voi, prm, gout=(0.0, GOUT[1]))
    assert (first.dz.astype(np.float32) + second.dz.astype(np.float32) == base.dz).all()
    _check(first, z, t, voi, prm, gout=(GOUT[0], 0.0))
    _check(second, z, t, voi, prm, gout=(0.0, GOUT[1]))


def test_refusals_leave_every_buffer_alone_and_an_empty_batch_launches_nothing():
    from dram_amd import _lib
    N, S = 2, 7
    bufs = [Placed((N, S)), Placed((N, S)), Placed((2,)), Placed((5 * N,)), Placed((2 * 13,), dtype=torch.float64), Placed((N, S))]
    zp, tp, out, state, ws, dz = bufs
    snap = [b.store.clone() for b in bufs]
    lib, st = _lib.lib, torch.cuda.current_stream().cuda_stream
    order = ("z", "t", "voi", "kt", "kv", "N", "S", "a", "b", "s", "alpha", "gamma", "out", "state", "ws", "nws", "st")

    def fwd(**kw):
        arg = dict(z=ptr(zp.t), t=ptr(tp.t), voi=None, kt=2, kv=2, N=N, S=S, a=.5, b=.5, s=1.0, alpha=.5, gamma=2.0,
                   out=ptr(out.t), state=ptr(state.t), ws=ptr(ws.t), nws=2 * 13 * 8, st=st)
        arg.update(kw)
        return lib.dram_seg_overlap_fwd(*[arg[k] for k in order])
    assert fwd(nws=2 * 13 * 8 - 8) == -2 and fwd(s=0.0) == -1 and fwd(kt=1) == -1 and fwd(alpha=1.5) == -1 and fwd(N=-1) == -1
    assert fwd(N=0) == 0 and fwd(S=0) == 0
    assert lib.dram_seg_overlap_bwd(ptr(zp.t), ptr(tp.t), None, 2, 2, N, S, .5, -1.0, ptr(state.t), ptr(out.t), ptr(dz.t), st) == -1
    assert lib.dram_seg_overlap_bwd(ptr(zp.t), ptr(tp.t), None, 2, 2, 0, S, .5, 2.0, ptr(state.t), ptr(out.t), ptr(dz.t), st) == 0
    torch.cuda.synchronize()
    for b, s in zip(bufs, snap):
        assert torch.equal(b.store.view(torch.uint8), s.view(torch.uint8))
