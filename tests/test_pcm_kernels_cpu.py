"""Host-side checks of tests/pcm_kernel_cases.py, the reference tests/test_gpu_pcm_kernels.py holds csrc/pcm.hip to:
  * the float64 restatement, composed as aggregate(attention(theta, phi), g), equals oracle.dram_oracle.pcm_forward to 1e-12
    in value and gradients for every merge type the oracle knows;
  * the inputs of every case satisfy the conditions that make float32 and float64 take the same discrete decisions;
  * sensitivity: a reference with one offset negated, block 1 (nodes 256..511) dropped, one feature plane skipped, c_lo
    ignored or the adjoint gathering at j + o_e differs from the true one by at least ten times the GPU test's tolerance."""
import pytest
import torch

import pcm_kernel_cases as K
from oracle import dram_oracle as O

ALL = list(K.CASES)
SPLIT = [c.id for c in K.SPLIT_CASES]
SUM = [c.id for c in K.SUM_CASES]


# ------------------------------------------------------------------------------------------------ against the oracle
def _restated_pcm(p, cam, f, offs, merge, p_enc_dim):
    """PCM.forward through the restatement, dispatched as dram_amd.functional.pcm_attention dispatches to the entry points."""
    th, ph, g = O._lin(p, "theta", f), O._lin(p, "phi", f), O._lin(p, "G", cam)
    modes = {"sm": (0, 0), "scaled_dot_product": (0, 1), "scaled_dot_product_relu": (1, 1), "smrelu": (1, 0), "smscaled": (0, 2),
             "l2sm": (2, 0), "l2smrelu": (3, 0)}
    if merge in O.PCM_GEO_MERGES:
        geo = O.pcm_geo_feature(p_enc_dim, f.shape[2:], f.dtype).unsqueeze(0).expand(f.shape[0], -1, -1, -1, -1)
        gth, gph = O._lin(p, "geo_theta", geo), O._lin(p, "geo_phi", geo)
        if merge == "att_is_all":
            a = K.attention_split(th + gth, ph + gph, offs, 0, 1, th.shape[1])
        else:
            relu = K.PCM_RELU if merge == "scaled_dot_product_geo_relu" else 0
            a = K.attention_split(torch.cat([th, gth], 1), torch.cat([ph, gph], 1), offs, relu, 1, th.shape[1])
    elif merge in O.PCM_SUM_MERGES:
        a = K.attention_sum(th, ph, offs, {"cosine": 0, "heu1": 1, "heu2": 2}[merge])
    elif merge == O.PCM_L2_MERGE:       # softmax_e(-5 (theta - phi_e)^2): the 'sm' form on (10 theta, -5) . (phi, phi^2)
        a = K.attention_split(torch.cat([10.0 * th, torch.full_like(th, -5.0)], 1), torch.cat([ph, ph * ph], 1), offs, 0, 0, 2)
    else:
        a = K.attention_split(th, ph, offs, *modes[merge], th.shape[1])
    return O._lin(p, "r", K.aggregate(a, g, offs))


@pytest.mark.parametrize("merge", O.PCM_DOT_MERGES + O.PCM_GEO_MERGES + O.PCM_SUM_MERGES + (O.PCM_L2_MERGE,))
def test_restatement_equals_oracle(merge):
    g = torch.Generator().manual_seed(70)
    grid, Bn, C, G, Gd, P = (4, 5, 6), 2, 6, 2, 3, 12
    Fd = 1 if merge == O.PCM_L2_MERGE else 4
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    p = {"theta.weight": rnd(Fd, C), "theta.bias": rnd(Fd), "phi.weight": rnd(Fd, C), "phi.bias": rnd(Fd),
         "G.weight": rnd(Gd, G), "G.bias": rnd(Gd), "r.weight": rnd(G, Gd), "r.bias": rnd(G)}
    if merge in O.PCM_GEO_MERGES:
        p.update({"geo_theta.weight": rnd(Fd, P), "geo_theta.bias": rnd(Fd), "geo_phi.weight": rnd(Fd, P), "geo_phi.bias": rnd(Fd)})
    f = rnd(Bn, C, *grid)
    if merge in O.PCM_SUM_MERGES:           # positive features and maps: sums of similarities away from 0
        f = f.abs()
        for k in ("theta.weight", "theta.bias", "phi.weight", "phi.bias"):
            p[k] = p[k].abs() * (0.12 if merge == "heu1" else 1.0)
    if merge == "smscaled":
        f = f * 0.03
    cam, gout = rnd(Bn, G, *grid), rnd(Bn, G, *grid)
    offs = [tuple(int(v) for v in o) for o in O.pcm_offsets(3, 2, False)]
    res = []
    for fn in ("oracle", "restated"):
        f_, cam_ = f.clone().requires_grad_(True), cam.clone().requires_grad_(True)
        if fn == "oracle":
            out = O.pcm_forward(p, cam_, f_, 3, 2, False, merge, 1, False, p_enc_dim=P if merge in O.PCM_GEO_MERGES else 0)
        else:
            out = _restated_pcm(p, cam_, f_, offs, merge, P)
        (out * gout).sum().backward()
        res.append((out.detach(), cam_.grad, f_.grad))
    (o_r, c_r, f_r), (o_k, c_k, f_k) = res
    rel = lambda a, b: ((a - b).abs().max() / b.abs().max()).item()
    assert rel(o_k, o_r) <= 1e-12 and rel(c_k, c_r) <= 1e-12
    if merge == "heu1":
        # the oracle (as the reference) forms heu1's similarities under no_grad: no gradient at all reaches theta / phi.  The
        # entry point, and with it the restatement, differentiates u with the 0.03 gate held constant
        assert f_r is None and f_k is not None and float(f_k.abs().max()) > 0.0
        th = O._lin(p, "theta", f)
        assert 0.02 < (K.attention_sum_raw(th, O._lin(p, "phi", f), offs, K.SUM_HEU1) == 0).double().mean().item() < 0.98
    else:
        assert rel(f_k, f_r) <= 1e-12


# ------------------------------------------------------------------------------------------------ input conditions
def test_skew_offsets():
    offs = K.OFFSETS["skew"]
    assert len(offs) == 128 == len(set(offs)) and (0, 0, 0) not in offs
    mirrored = sum(1 for o in offs if tuple(-v for v in o) in set(offs))
    assert 0 < mirrored <= 16                                       # mostly without the mirror image
    assert max(abs(v) for o in offs for v in o) == 6 and all(-127 <= v <= 127 for o in offs for v in o)
    valid = K.Stencil(offs, K.GRID).valid()
    never = [o for e, o in enumerate(offs) if float(valid[0, e].sum()) == 0.0]
    assert {o for o in offs if abs(o[0]) >= 5} <= set(never) and len(never) >= 16     # some offsets never land inside the grid
    none = K.edgeless_nodes("skew")
    assert 0 < int(none.sum()) < K.S // 4 and int((~none).sum()) > 0      # both kinds of node
    assert torch.equal(none.nonzero(), torch.tensor([[4, y, x] for y in (7, 8) for x in (11, 12)]))
    for name in ("k3", "k5"):
        assert not bool(K.edgeless_nodes(name).any())
    assert len(K.OFFSETS["k3"]) == 18 and len(K.OFFSETS["k5"]) == 125 and (0, 0, 0) in K.OFFSETS["k5"]


def test_grid_reaches_three_blocks():
    assert K.S == 585 and K.S // 256 == 2 and K.S % 256 == 73 and K.B == 2 and len(set(K.GRID)) == 3
    b, z, y, x = K.ZERO_NODE
    assert 256 <= (z * K.GRID[1] + y) * K.GRID[2] + x < 512


@pytest.mark.parametrize("cid", SPLIT)
def test_split_inputs_are_exact(cid):
    c = K.CASES[cid]
    theta, phi, dattn = K.split_inputs(cid)
    offs = K.OFFSETS[c.offs]
    for t in (theta, phi, dattn):
        assert torch.equal(t.float().double(), t)
    nz = theta != 0
    if c.flags & K.PCM_L2NORM:          # the zero-theta node, and only it
        b, z, y, x = K.ZERO_NODE
        assert int((~nz).sum()) == c.F and not bool(nz[b, :, z, y, x].any())
    else:
        assert bool(nz.all())
    assert bool((phi != 0).all())
    lim = 0.25 if c.scale == K.SCALE_100 else 2.0
    assert float(theta.abs().max()) <= lim and float(phi.abs().max()) <= lim
    # the float32 dots equal the float64 dots bit for bit: the ReLU gate (exact zeros included) cannot differ
    k64, k32 = {}, {}
    K.attention_split(theta, phi, offs, c.flags, c.scale, c.F_relu, k64)
    K.attention_split(theta.float(), phi.float(), offs, c.flags, c.scale, c.F_relu, k32)
    for name in ("dot_act", "dot_raw"):
        assert k32[name].dtype == torch.float32 and torch.equal(k32[name].detach().double(), k64[name].detach())
    if c.flags & K.PCM_RELU and c.F_relu > 0:
        valid = K.Stencil(offs, K.GRID).valid().bool().expand_as(k64["dot_act"])
        d = k64["dot_act"].detach()[valid]
        assert 0.1 < (d > 0).double().mean().item() < 0.9       # the gate is open and shut; exact zeros occur or not:
        print(f"{cid}: {int((d == 0).sum())} of {d.numel()} activated dots are exactly 0")
    if c.flags & K.PCM_L2NORM:
        b, z, y, x = K.ZERO_NODE
        assert float(k64["dot_act"].detach()[b, :, z, y, x].abs().max()) == 0.0
        assert float(dattn[b, :, z, y, x].abs().max()) < 1e-10 and float(dattn.abs().max()) > 1.0


@pytest.mark.parametrize("cid", SUM)
def test_sum_inputs_are_decided(cid):
    c = K.CASES[cid]
    theta, phi, dattn = K.sum_inputs(cid)
    offs = K.OFFSETS[c.offs]
    no_tie, low = K.sum_input_conditions(c, theta, phi)
    assert no_tie and low >= K.MIN_ROW_SUM
    k, m, valid = K.heu_integers(theta, phi, offs)
    k32, m32, _ = K.heu_integers(theta.float(), phi.float(), offs)
    assert torch.equal(k32.double(), k) and torch.equal(m32.double(), m)        # dot and L1 distance exact in float32
    assert torch.equal(k, k.round()) and torch.equal(m, m.round())
    if c.mode == K.SUM_COSINE:
        assert float(theta.min()) >= 0.125 and float(phi.min()) >= 0.125       # norms >= 0.125 >> 1e-8
        assert float(K.attention_sum_raw(theta, phi, offs, c.mode)[valid].min()) > 0.0
    else:
        u64 = (k / 64.0) / (1.0 + m / 8.0)
        u32 = (k32 / 64.0) / (1.0 + m32 / 8.0)
        thr64, thr32 = (0.03, torch.tensor(0.03, dtype=torch.float32)) if c.mode == K.SUM_HEU1 else (0.0, 0.0)
        assert torch.equal((u32 < thr32)[valid], (u64 < thr64)[valid])          # the gate, float32 against float64
        if c.mode == K.SUM_HEU1:
            assert torch.equal((u32 < thr32)[valid], ((u32.double()) < 0.03)[valid])     # (0.03f against the double 0.03)
            assert float((u64 - 0.03).abs()[valid].min()) >= 1.0 / (100.0 * (64.0 + 8.0 * float(m.max())))
        shut = (u64 < thr64)[valid].double().mean().item()
        assert 0.1 < shut < 0.9


@pytest.mark.parametrize("cid", ["agg_" + c.id for c in K.AGG_CASES])
def test_aggregate_inputs(cid):
    c = K.CASES[cid]
    attn, v, dout = K.agg_inputs(cid)
    valid = K.Stencil(K.OFFSETS[c.offs], K.GRID).valid().bool().expand_as(attn)
    assert float(attn.min()) >= 0.0 and float(attn[~valid].abs().max() if bool((~valid).any()) else 0.0) == 0.0
    assert float(attn[valid].max()) > 0.9


# ------------------------------------------------------------------------------------------------ sensitivity
def _moved(cid, corrupted, names=None):
    """Every named output of `corrupted` is >= 10 x the GPU tolerance (4 x e32 of the same case) from the reference."""
    ref64, e32 = K.reference(cid)
    checked = 0
    for name in (names or ref64):
        if e32[name] is None:
            continue
        tol = K.tolerance(e32[name])
        got = K.errs(corrupted[name], ref64[name])
        assert got[0] >= 10.0 * tol[0] and got[1] >= 10.0 * tol[1], (cid, name, got, tol)
        assert tol[0] < 1e-4 and tol[1] < 1e-4, (cid, name, tol)       # the tolerance itself is a rounding-level number
        checked += 1
    assert checked > 0
    return checked


def _flip_index(offs):
    """The first small, nonzero offset of the table."""
    return next(e for e, o in enumerate(offs) if any(o) and max(abs(v) for v in o) <= 2)


@pytest.mark.parametrize("cid", ALL)
def test_one_offset_negated(cid):
    offs = list(K.OFFSETS[K.CASES[cid].offs])
    e = _flip_index(offs)
    offs[e] = tuple(-v for v in offs[e])
    _moved(cid, K.evaluate(cid, offsets=offs))


@pytest.mark.parametrize("cid", ALL)
def test_block_one_dropped(cid):
    ref64, _ = K.reference(cid)
    out = {}
    for name, t in ref64.items():
        t = t.clone().flatten(2)
        t[:, :, 256:512] = 0.0
        out[name] = t.view_as(ref64[name])
    _moved(cid, out)


@pytest.mark.parametrize("cid", ALL)
def test_one_plane_skipped(cid):
    c = K.CASES[cid]
    planes = c.C if isinstance(c, K.AggCase) else c.F
    _moved(cid, K.evaluate(cid, skip_plane=planes - 1))


@pytest.mark.parametrize("cid", SPLIT)
def test_adjoint_launches(cid):
    """dphi as dram_pcm_attention_split_bwd composes it from pcm_scatter_adjoint_kernel launches equals autograd's; with
    c_lo ignored in the second launch (relu_split3: channels 0, 1 overwritten from ds2, channels 3, 4 never written) or with
    the gather at j + o_e it does not."""
    c = K.CASES[cid]
    ref64, _ = K.reference(cid)
    theta = K.split_inputs(cid)[0]
    offs = K.OFFSETS[c.offs]
    F1 = c.F_relu if K.is_split(c) else c.F
    parts = []
    if F1 > 0:
        parts.append(K.scatter_adjoint(ref64["ds"], theta[:, :F1], offs))
    if F1 < c.F:
        parts.append(K.scatter_adjoint(ref64["ds2"], theta[:, F1:], offs))
    dphi = torch.cat(parts, 1)
    assert K.errs(dphi, ref64["dphi"])[0] <= 1e-12
    if 0 < F1 < c.F:
        bad = dphi.clone()
        bad[:, :c.F - F1] = K.scatter_adjoint(ref64["ds2"], theta[:, :c.F - F1], offs)
        bad[:, F1:] = 0.0
        _moved(cid, {"dphi": bad}, ["dphi"])
    mirrored = [tuple(-v for v in o) for o in offs]
    w = ref64["ds2"] if F1 == 0 else ref64["ds"]
    _moved(cid, {"dphi": torch.cat([K.scatter_adjoint(w, theta[:, :max(F1, 1)], mirrored), dphi[:, max(F1, 1):]], 1)}, ["dphi"])


def test_c_lo_case_exists():
    assert [c.id for c in K.SPLIT_CASES if 0 < c.F_relu < c.F and K.is_split(c)] == ["relu_split3"]
    assert [c.id for c in K.SPLIT_CASES if c.F_relu == 0 and K.is_split(c)] == ["relu_split0"]
    assert {(c.flags, c.scale) for c in K.SPLIT_CASES if c.offs == "k3" and c.F_relu == c.F} == {
        (0, 0), (0, 1), (1, 1), (1, 0), (0, 2), (2, 0), (3, 0)}
