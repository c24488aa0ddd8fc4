"""The per-op norm entry points of csrc/norm.hip past one lap and one block of their small kernels.

dram_norm_fwd_train, dram_bn_fwd_eval, dram_norm_bwd, dram_bn_stats, dram_bn_bwd_sums and dram_bn_bwd_apply_sums through the C
ABI on the cases of tests/norm_stat_cases.py: 300 and 350 work items per statistic (the `it += 256` laps of norm_finalize_kernel
and bn_stats_finalize_kernel, their it / nchunks, it % nchunks decode and the chunk_len weighting of a ragged last chunk), 300
members (the second lap of the rowcoef loop), 130 and 300 channels and 99 and 270 statistics (further blocks of the 64-thread
finalizers), 260 to 900 rows (further blocks of row_sum_chunks_kernel and bn_eval_coef_kernel).  The comment next to each case in
that file says what it reaches; tests/test_norm_stats_cpu.py shows that with these inputs a lost, doubled or mis-weighted work
item is at least ten tolerances away.

Against the float64 reference of that file: check() of tests/test_gpu_parity.py at its TOL = 1e-4 for everything but the mean,
which is held to mean_bound (derived there from row_moments_kernel's 26 fp32 roundings).  Every output and the workspace is
filled with NaN before the call, every output sits between guard words, no output may keep a NaN.

Each test prints a `norm-stats:` line with its measured errors before it asserts (run with -s to see the figures)."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import norm_stat_cases as K
from norm_stat_cases import BATCH, BATCH_IDS, CASE, CASES, EPS, MOMENTUM
from test_gpu_onload import DEV, Placed, call, ordered, p
from test_gpu_parity import TOL, check, rel_err

pytestmark = pytest.mark.gpu
IDS = [c.id for c in CASES]


def report(line):
    print("norm-stats: " + line)


@lru_cache(maxsize=None)
def on_device(case_id):
    return {k: v.to(DEV) for k, v in K.inputs(case_id).items()}


def workspace(c):
    """The norm workspace between guard bytes, every byte 0xFF (a NaN in each float and each double)."""
    from dram_amd import _lib
    return Placed((int(_lib.lib.dram_norm_ws_bytes(c.N, c.C, c.S)),), dtype=torch.uint8)


def written(tag, **outs):
    """Guard words intact and no NaN left in any of the Placed outputs."""
    torch.cuda.synchronize()
    for name, o in outs.items():
        assert o.intact(), f"{tag}: a write outside {name}"
        assert not bool(torch.isnan(o.t).any()), f"{tag}: {name} has elements that were not written"


class Figures:
    """Collects max-abs / max|ref| per output, prints them in one line, then asserts check() on each."""

    def __init__(self, tag):
        self.tag, self.items, self.line = tag, [], []

    def tol(self, name, got, ref):
        ref = ref.view_as(got) if isinstance(ref, torch.Tensor) else ref
        self.items.append((name, got, ref))
        self.line.append(f"{name} {rel_err(got, ref)[0]:.2e}")

    def mean(self, name, got, case_id):
        f = K.forward_ref(case_id)
        err = (got.detach().double().cpu() - f["save_mean"]).abs()
        bound = K.mean_bound(f["sum_abs_over_count"], f["save_mean"])
        self.worst_mean = (err / bound).max().item()
        self.line.append(f"{name} {err.max().item():.2e} abs = {self.worst_mean:.3f} of its bound")
        self.items.append((name, None, None))

    def done(self):
        report(f"{self.tag}: " + ", ".join(self.line))
        for name, got, ref in self.items:
            if got is None:
                assert self.worst_mean <= 1.0, f"{self.tag}: {name} is {self.worst_mean:.3f} of mean_bound"
            else:
                check(got, ref, f"{self.tag} {name}")


class Fwd:
    """One forward call and what it leaves: y, save_mean, save_rstd, rowcoef (Placed), running statistics where given."""

    def __init__(self, case_id, relu, mode="train", running=True):
        c, D = CASE[case_id], on_device(case_id)
        L = K.layout(case_id)
        self.c, self.relu = c, relu
        nstat = c.C if mode == "eval" else L.nstat
        self.y, self.mean, self.rstd = Placed((c.N, c.C, c.S)), Placed((nstat,)), Placed((nstat,))
        self.coef = Placed((L.rows, 2))
        self.rm = self.rv = None
        outs = dict(y=self.y, save_mean=self.mean, save_rstd=self.rstd, rowcoef=self.coef)
        if mode == "eval":
            call("dram_bn_fwd_eval", p(D["x"]), p(D["gamma"]), p(D["beta"]), p(D["running_mean"]), p(D["running_var"]),
                 p(self.y.t), p(self.mean.t), p(self.rstd.t), p(self.coef.t), EPS, relu, c.N, c.C, c.S)
        else:
            self.ws = workspace(c)
            if running and c.kind == BATCH:
                self.rm, self.rv = Placed((c.C,), src=D["running_mean"]), Placed((c.C,), src=D["running_var"])
                outs.update(running_mean=self.rm, running_var=self.rv)
            call("dram_norm_fwd_train", p(D["x"]), p(D["gamma"]), p(D["beta"]), p(self.y.t), p(self.mean.t), p(self.rstd.t),
                 p(self.coef.t), p(self.rm and self.rm.t), p(self.rv and self.rv.t), MOMENTUM, EPS, c.kind, c.G, relu,
                 c.N, c.C, c.S, p(self.ws.t), self.ws.t.numel())
            outs.update(ws=self.ws)
        written(f"{case_id} {mode} forward relu={relu}", **outs)


@lru_cache(maxsize=None)
def fwd_train(case_id, relu):
    return Fwd(case_id, relu)


@lru_cache(maxsize=None)
def fwd_eval(case_id, relu):
    return Fwd(case_id, relu, mode="eval")


def backward(case_id, f, batch_stats=1, params=True):
    """dram_norm_bwd on the outputs of forward `f`, on a fresh 0xFF workspace -> (dx, dgamma, dbeta) Placed (None without)."""
    c, D = f.c, on_device(case_id)
    dx = Placed((c.N, c.C, c.S))
    dgamma, dbeta = (Placed((c.C,)), Placed((c.C,))) if params else (None, None)
    ws = workspace(c)
    call("dram_norm_bwd", p(D["dy"]), p(D["x"]), p(D["gamma"]), p(f.mean.t), p(f.rstd.t), p(f.coef.t), p(dx.t),
         p(dgamma and dgamma.t), p(dbeta and dbeta.t), c.kind, c.G, f.relu, batch_stats, c.N, c.C, c.S, p(ws.t), ws.t.numel())
    outs = dict(dx=dx, ws=ws)
    if params:
        outs.update(dgamma=dgamma, dbeta=dbeta)
    written(f"{case_id} backward relu={f.relu} batch_stats={batch_stats}", **outs)
    return dx, dgamma, dbeta


@lru_cache(maxsize=None)
def bwd_train(case_id, relu):
    return backward(case_id, fwd_train(case_id, relu))


# ------------------------------------------------------------------ dram_norm_fwd_train
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("case_id", IDS)
def test_fwd_train(case_id, relu):
    """row_moments -> norm_finalize_kernel -> row_affine_act: statistics, per-row {a, b}, running statistics and y."""
    f, ref = fwd_train(case_id, relu), K.forward_ref(case_id)
    fig = Figures(f"fwd_train {case_id} relu={relu}")
    fig.mean("save_mean", f.mean.t, case_id)
    fig.tol("save_rstd", f.rstd.t, ref["save_rstd"])
    fig.tol("rowcoef", f.coef.t, ref["rowcoef"])
    if f.rm is not None:
        fig.tol("running_mean", f.rm.t, ref["running_mean"])
        fig.tol("running_var", f.rv.t, ref["running_var"])
    fig.tol("y", f.y.t, K.y_of(ref["pre"], relu))
    fig.done()


def test_fwd_train_without_running_statistics():
    """running_mean = running_var = NULL (what the backward tests of the suite pass): the same statistics and y bit for bit."""
    case_id = "bn_c130"
    a, b = fwd_train(case_id, 1), Fwd(case_id, 1, running=False)
    assert b.rm is None
    for name in ("y", "mean", "rstd", "coef"):
        assert torch.equal(getattr(a, name).t, getattr(b, name).t), name
    report(f"fwd_train {case_id} without running statistics: y, save_mean, save_rstd, rowcoef equal bit for bit")


# ------------------------------------------------------------------ dram_norm_bwd
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("case_id", IDS)
def test_bwd(case_id, relu):
    """row_bwd_reduce -> row_sum_chunks -> bn_bwd_finalize / gn_bwd_finalize_rows (+ gn_bwd_finalize_params) -> row_bwd_apply
    on that forward's outputs.  With dgamma = dbeta = NULL the group path skips gn_bwd_finalize_params_kernel and the batch
    path its two stores: dx must not change by a bit."""
    dx, dgamma, dbeta = bwd_train(case_id, relu)
    ref = K.backward_ref(case_id, relu)
    fig = Figures(f"bwd {case_id} relu={relu}")
    fig.tol("dx", dx.t, ref["dx"])
    fig.tol("dgamma", dgamma.t, ref["dgamma"])
    fig.tol("dbeta", dbeta.t, ref["dbeta"])
    dx_only, _, _ = backward(case_id, fwd_train(case_id, relu), params=False)
    same = torch.equal(dx_only.t, dx.t)
    fig.line.append("dx without dgamma/dbeta " + ("equal" if same else "DIFFERS"))
    fig.done()
    assert same


# ------------------------------------------------------------------ eval-mode BatchNorm
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("case_id", BATCH_IDS)
def test_bn_eval_forward_and_backward(case_id, relu):
    """bn_eval_coef_kernel (up to 900 rows: 4 blocks) -> row_affine_act, then dram_norm_bwd with batch_stats = 0:
    bn_bwd_finalize_kernel with k2 = k3 = 0, i.e. dx = gamma * rstd * dy'."""
    f, ref, I = fwd_eval(case_id, relu), K.eval_ref(case_id, relu), K.inputs(case_id)
    fig = Figures(f"bn_eval {case_id} relu={relu}")
    assert torch.equal(f.mean.t.cpu(), I["running_mean"])
    fig.tol("save_rstd", f.rstd.t, ref["save_rstd"])
    fig.tol("rowcoef", f.coef.t, ref["rowcoef"])
    fig.tol("y", f.y.t, K.y_of(ref["pre"], relu))
    dx, dgamma, dbeta = backward(case_id, f, batch_stats=0)
    fig.tol("dx", dx.t, ref["dx"])
    fig.tol("dgamma", dgamma.t, ref["dgamma"])
    fig.tol("dbeta", dbeta.t, ref["dbeta"])
    fig.done()


# ------------------------------------------------------------------ dram_bn_stats
@pytest.mark.parametrize("case_id", BATCH_IDS)
def test_bn_stats(case_id):
    """row_moments -> bn_stats_finalize_kernel: per channel {mean, M2} in fp64.  It runs norm_finalize_kernel's fp64 loops on the
    same partials, so its mean, cast to float32, is save_mean of dram_norm_fwd_train bit for bit, and save_rstd is
    float32(1/sqrt(M2/(N*S) + eps)) of its M2 to the rounding of that kernel's own fp64 division and sqrt (1 ulp)."""
    c, D, ref, f = CASE[case_id], on_device(case_id), K.forward_ref(case_id), fwd_train(case_id, 0)
    mm, ws = Placed((c.C, 2), dtype=torch.float64), workspace(c)
    call("dram_bn_stats", p(D["x"]), p(mm.t), c.N, c.C, c.S, p(ws.t), ws.t.numel())
    written(f"bn_stats {case_id}", mean_m2=mm, ws=ws)
    mean, m2 = mm.t[:, 0].cpu(), mm.t[:, 1].cpu()
    fig = Figures(f"bn_stats {case_id}")
    fig.mean("mean", mean, case_id)
    fig.tol("M2", m2, ref["m2"])
    same_mean = torch.equal(mean.float(), f.mean.t.cpu())
    host_rstd = torch.from_numpy((1.0 / np.sqrt(m2.numpy() / (float(c.N) * float(c.S)) + EPS)).astype(np.float32))
    ulps = int((ordered(f.rstd.t.cpu()) - ordered(host_rstd)).abs().max())
    fig.line.append(f"float32(mean) {'==' if same_mean else '!='} save_mean, save_rstd {ulps} ulp from float32(rstd(M2))")
    fig.done()
    assert same_mean
    assert ulps <= 1


# ------------------------------------------------------------------ the split backward
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("case_id", BATCH_IDS)
def test_split_backward_equals_the_whole_backward(case_id, relu):
    """dram_bn_bwd_sums + dram_bn_bwd_apply_sums with count = N*S on a workspace refilled with 0xFF: dx of dram_norm_bwd bit for
    bit, and the fp64 sums cast to float32 are dbeta and dgamma exactly (the assertion of tests/test_gpu_syncbn.py, here with
    260 and 900 rows -- further blocks of row_sum_chunks_kernel -- and 130 channels -- further blocks of bn_bwd_sums_kernel and
    bn_pqr_from_sums_kernel)."""
    c, D, f = CASE[case_id], on_device(case_id), fwd_train(case_id, relu)
    dx, dgamma, dbeta = bwd_train(case_id, relu)
    dx2, sums, ws = Placed((c.N, c.C, c.S)), Placed((c.C, 2), dtype=torch.float64), workspace(c)
    call("dram_bn_bwd_sums", p(D["dy"]), p(D["x"]), p(f.mean.t), p(f.rstd.t), p(f.coef.t), p(sums.t), relu, c.N, c.C, c.S,
         p(ws.t), ws.t.numel())
    call("dram_bn_bwd_apply_sums", p(D["dy"]), p(D["x"]), p(D["gamma"]), p(f.mean.t), p(f.rstd.t), p(f.coef.t), p(sums.t),
         float(c.N) * float(c.S), p(dx2.t), relu, c.N, c.C, c.S, p(ws.t), ws.t.numel())
    written(f"split backward {case_id} relu={relu}", dx=dx2, sums=sums, ws=ws)
    ref = K.backward_ref(case_id, relu)
    fig = Figures(f"split_bwd {case_id} relu={relu}")
    fig.tol("sum dy'", sums.t[:, 0], ref["dbeta"])
    fig.tol("sum dy'*xhat", sums.t[:, 1], ref["dgamma"])
    got_dbeta, got_dgamma = sums.t[:, 0].float(), sums.t[:, 1].float()
    fig.line.append(f"dx max|diff| {(dx2.t - dx.t).abs().max().item():.1e}, dbeta {(got_dbeta - dbeta.t).abs().max().item():.1e}, "
                    f"dgamma {(got_dgamma - dgamma.t).abs().max().item():.1e}")
    fig.done()
    assert torch.equal(dx2.t, dx.t)
    assert torch.equal(got_dbeta, dbeta.t) and torch.equal(got_dgamma, dgamma.t)
