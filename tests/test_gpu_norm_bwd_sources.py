"""dram_norm_bwd_head / dram_norm_bwd_pool_add: the norm backward that takes its incoming gradient from where it comes from.

The fused engine used to write the 1x1x1 head's input gradient (dram_conv3d_k1_bwd_lazy, dx) and to add the max-pool's routed
gradient onto the skip gradient (dram_maxpool3d_2_bwd_acc) before the producing stage's dram_norm_bwd read the result twice.
The two entry points form that gradient while they load.  Here each is compared with the composition it replaces, on the same
inputs: dx, dgamma and dbeta must be equal bit for bit (torch.equal) -- the head policy runs conv1x1_dgrad_kernel's fmaf chain,
the pool policy the accumulate kernel's one fp32 add.  One case per policy and norm is also held to a float64 torch-CPU
norm + ReLU backward with the TOL / check of tests/test_gpu_onload.py.

Shapes (CHUNK = 4096 floats per (row, chunk) block of the row kernels, csrc/norm.hip): the comment next to each says which
kernels the host-side rule sends it to, and why.  Every tensor a policy reads or writes sits between guard words (Placed)."""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_onload import DEV, Placed, call, g, p
from test_gpu_parity import check

pytestmark = pytest.mark.gpu
EPS = 1e-5
BATCH, GROUP = 0, 1

# (name, kind, groups or None for "all channels", batch_stats)
NORMS = [("bn_train", BATCH, 1, 1), ("bn_eval", BATCH, 1, 0), ("gn_one", GROUP, 1, 1), ("gn_all", GROUP, None, 1)]


def report(line):
    print("norm-bwd-source: " + line)


def ws_for(N, C, S):
    from dram_amd import _lib
    return torch.empty(max(int(_lib.lib.dram_norm_ws_bytes(N, C, S)), 16), dtype=torch.uint8, device=DEV)


class Forward:
    """x [N, C, S] and what a forward of norm (+ReLU) leaves for backward: mean, rstd, per-row {a, b}.  gamma has both
    signs, so the ReLU mask keeps either side of the mean."""

    def __init__(self, N, C, S, norm, seed):
        _, self.kind, G, self.batch_stats = norm
        self.N, self.C, self.S = N, C, S
        self.G = C if G is None else G
        self.x_cpu = torch.randn(N, C, S, generator=g(seed)) * 1.7 + 0.6
        self.gamma_cpu = torch.linspace(-1.3, 0.9, C) + 0.05
        self.beta_cpu = torch.linspace(0.4, -0.3, C)
        self.rm_cpu = torch.linspace(0.3, 0.8, C)
        self.rv_cpu = torch.linspace(2.0, 3.5, C)
        self.x, self.gamma, self.beta = self.x_cpu.to(DEV), self.gamma_cpu.to(DEV), self.beta_cpu.to(DEV)
        self.rm, self.rv = self.rm_cpu.to(DEV), self.rv_cpu.to(DEV)
        nstat = C if self.kind == BATCH else N * self.G
        self.mean = torch.empty(nstat, device=DEV)
        self.rstd = torch.empty(nstat, device=DEV)
        self.coef = torch.empty(2 * N * C, device=DEV)
        self.ws = ws_for(N, C, S)
        y = torch.empty_like(self.x)
        if self.batch_stats:
            call("dram_norm_fwd_train", p(self.x), p(self.gamma), p(self.beta), p(y), p(self.mean), p(self.rstd), p(self.coef),
                 None, None, 0.1, EPS, self.kind, self.G, 0, N, C, S, p(self.ws), self.ws.numel())
        else:
            call("dram_bn_fwd_eval", p(self.x), p(self.gamma), p(self.beta), p(self.rm), p(self.rv), p(y),
                 p(self.mean), p(self.rstd), p(self.coef), EPS, 0, N, C, S)
        torch.cuda.synchronize()

    def tail(self, relu):
        """The arguments every backward entry point ends with, after dx / dgamma / dbeta (S only where the entry takes it)."""
        return (self.kind, self.G, relu, self.batch_stats, self.N, self.C)

    def bwd(self, entry, head_args, dx, relu, with_S=True):
        """entry(*head_args, x, gamma, mean, rstd, rowcoef, dx, dgamma, dbeta, kind, G, relu, batch_stats, N, C[, S], ws...)
        -> (dgamma, dbeta), both NaN-filled before the call."""
        dgamma = torch.full((self.C,), float("nan"), device=DEV)
        dbeta = torch.full((self.C,), float("nan"), device=DEV)
        size = (self.S,) if with_S else ()
        call(entry, *head_args, p(self.x), p(self.gamma), p(self.mean), p(self.rstd), p(self.coef), p(dx), p(dgamma), p(dbeta),
             *self.tail(relu), *size, p(self.ws), self.ws.numel())
        torch.cuda.synchronize()
        return dgamma, dbeta

    def reference64(self, d64, relu):
        """(dx, dgamma, dbeta) of norm (+ReLU) in float64 on the CPU for the incoming gradient d64 [N, C, S]."""
        xr = self.x_cpu.double().requires_grad_(True)
        gm, bt = self.gamma_cpu.double().requires_grad_(True), self.beta_cpu.double().requires_grad_(True)
        if self.kind == GROUP:
            y = F.group_norm(xr, self.G, gm, bt, EPS)
        elif self.batch_stats:
            y = F.batch_norm(xr, None, None, gm, bt, True, 0.1, EPS)
        else:
            y = F.batch_norm(xr, self.rm_cpu.double(), self.rv_cpu.double(), gm, bt, False, 0.1, EPS)
        (F.relu(y) if relu else y).backward(d64)
        return xr.grad, gm.grad, bt.grad


def same(tag, got, ref):
    for name, a, b in zip(("dx", "dgamma", "dbeta"), got, ref):
        assert not bool(torch.isnan(a).any()), f"{tag}: {name} has elements that were not written"
        assert torch.equal(a, b), f"{tag}: {name} differs from the composition of the unchanged entry points"


def against64(tag, fwd, got, d64, relu):
    ref = fwd.reference64(d64, relu)
    for name, a, b in zip(("dx", "dgamma", "dbeta"), got, ref):
        check(a, b.view_as(a), f"{tag} {name} vs float64")


# ------------------------------------------------------------------ pool-add
POOL_ADD_CASES = [
    # shape, bytes dy is off 16-byte alignment, the kernels.  The row kernels are the 16-byte ones under dram_norm_bwd's own rule
    # (S % 4 == 0, dy / x / dx 16-byte aligned), so that the sums run in the order they have on the materialised gradient; the
    # policy takes the pooled cells of a float4 together ("vector": W % 4 == 0, gp 8-byte, idx 2-byte aligned) or per element
    ((1, 2, 18, 16, 20), 0, "vector"),      # S = 5760: two chunks per row; 4096 = 12*320 + 256 falls inside an x row, tail of 1664
    ((1, 3, 7, 9, 12), 0, "vector"),        # S = 756: one chunk; the last plane and the last row have no pooled cell
    ((1, 2, 3, 5, 7), 0, "scalar"),         # S = 105: scalar row kernels and per-element cells, everything cropped
    ((2, 2, 6, 10, 11), 0, "scalar"),       # W = 11: pooled cells per element (in the 16-byte row kernels: S = 660), cropped column
    ((2, 3, 6, 10, 12), 4, "scalar"),       # W = 12, but dy is 4 bytes off: scalar row kernels
]


def routed64(gp, idx, shape):
    """The max-pool backward in float64: gp lands on the voxel of its window that idx names, everything else is 0."""
    N, C, D, H, W = shape
    out = torch.zeros(shape, dtype=torch.float64)
    De, He, We = 2 * (D // 2), 2 * (H // 2), 2 * (W // 2)
    for k in range(8):
        dz, dy, dx = k >> 2, (k >> 1) & 1, k & 1
        out[:, :, dz:De:2, dy:He:2, dx:We:2] = gp.double() * (idx == k)
    return out


def pool_add_case(shape, shift, norm, relu, seed):
    N, C, D, H, W = shape
    S = D * H * W
    oshape = (N, C, D // 2, H // 2, W // 2)
    fwd = Forward(N, C, S, norm, seed)
    dy0 = torch.randn(*shape, generator=g(seed + 1))
    gp0 = torch.randn(*oshape, generator=g(seed + 2))
    idx0 = torch.randint(0, 8, oshape, generator=g(seed + 3), dtype=torch.uint8)
    gp, idx = Placed(oshape, src=gp0), Placed(oshape, dtype=torch.uint8, src=idx0)
    # the composition it replaces: accumulate, then the plain backward in place
    old = Placed(shape, shift, src=dy0)
    call("dram_maxpool3d_2_bwd_acc", p(gp.t), p(idx.t), p(old.t), N, C, D, H, W)
    old_dg, old_db = fwd.bwd("dram_norm_bwd", (p(old.t),), old.t, relu)
    # the new entry point, in place over dy as the engine runs it
    new = Placed(shape, shift, src=dy0)
    new_dg, new_db = fwd.bwd("dram_norm_bwd_pool_add", (p(new.t), p(gp.t), p(idx.t), D, H, W), new.t, relu, with_S=False)
    assert old.intact() and new.intact() and gp.intact() and idx.intact()
    assert torch.equal(gp.t.cpu(), gp0) and torch.equal(idx.t.cpu(), idx0)
    got = (new.t, new_dg, new_db)
    same(f"pool_add {shape} shift={shift} {norm[0]} relu={relu}", got, (old.t, old_dg, old_db))
    return fwd, got, dy0.double() + routed64(gp0, idx0, shape)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("norm", NORMS, ids=[n[0] for n in NORMS])
@pytest.mark.parametrize("shape,shift,kernels", POOL_ADD_CASES)
def test_pool_add_equals_accumulate_then_norm_bwd(shape, shift, kernels, norm, relu):
    pool_add_case(shape, shift, norm, relu, seed=900)
    report(f"pool_add {shape} dy shift={shift} {norm[0]} relu={relu} [{kernels} kernels]: dx, dgamma, dbeta equal to "
           f"dram_maxpool3d_2_bwd_acc + dram_norm_bwd")


@pytest.mark.parametrize("norm", NORMS[:3], ids=[n[0] for n in NORMS[:3]])
def test_pool_add_against_float64(norm):
    shape = POOL_ADD_CASES[0][0]
    fwd, got, d64 = pool_add_case(shape, 0, norm, 1, seed=910)
    against64(f"pool_add {shape} {norm[0]}", fwd, got, d64.view(shape[0], shape[1], -1), 1)


# ------------------------------------------------------------------ head
HEAD_CASES = [
    # N, C, Cout, S, the kernels (vector: S % 4 == 0 and g / x / dx 16-byte aligned)
    (2, 5, 1, 2 * 4096 + 12, "vector"),     # three chunks per row, the last of 12 elements; the flagship's single output
    (2, 5, 3, 2 * 4096 + 12, "vector"),     # the fmaf chain over three outputs
    (2, 5, 8, 4096 + 4, "vector"),          # the most outputs the policy takes (one pass of the 1x1x1 kernels)
    (2, 5, 1, 4099, "scalar"),              # S % 4 != 0: scalar kernels, a second chunk of 3 elements
    (2, 5, 3, 4099, "scalar"),
]


def head_case(N, C, Cout, S, norm, relu, seed):
    fwd = Forward(N, C, S, norm, seed)
    g0 = torch.randn(N, Cout, S, generator=g(seed + 1))
    w0 = torch.randn(Cout, C, generator=g(seed + 2))
    gt, w = Placed((N, Cout, S), src=g0), Placed((Cout, C), src=w0)
    # the composition it replaces: the 1x1x1 conv's dx written out, then the plain backward in place
    old = Placed((N, C, S))
    call("dram_conv3d_k1_bwd_lazy", p(gt.t), p(fwd.x), None, 0, p(w.t), p(old.t), None, None, None, 0, N, C, Cout, S)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(old.t).any())
    old_dg, old_db = fwd.bwd("dram_norm_bwd", (p(old.t),), old.t, relu)
    new = Placed((N, C, S))
    new_dg, new_db = fwd.bwd("dram_norm_bwd_head", (p(gt.t), p(w.t), Cout), new.t, relu)
    assert old.intact() and new.intact() and gt.intact() and w.intact()
    assert torch.equal(gt.t.cpu(), g0) and torch.equal(w.t.cpu(), w0)
    got = (new.t, new_dg, new_db)
    same(f"head N={N} C={C} Cout={Cout} S={S} {norm[0]} relu={relu}", got, (old.t, old_dg, old_db))
    return fwd, got, torch.einsum("oc,nos->ncs", w0.double(), g0.double())


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("norm", NORMS, ids=[n[0] for n in NORMS])
@pytest.mark.parametrize("N,C,Cout,S,kernels", HEAD_CASES)
def test_head_equals_dgrad_then_norm_bwd(N, C, Cout, S, kernels, norm, relu):
    head_case(N, C, Cout, S, norm, relu, seed=950)
    report(f"head N={N} C={C} Cout={Cout} S={S} {norm[0]} relu={relu} [{kernels} kernels]: dx, dgamma, dbeta equal to "
           f"dram_conv3d_k1_bwd_lazy (dx) + dram_norm_bwd")


@pytest.mark.parametrize("norm", NORMS[:3], ids=[n[0] for n in NORMS[:3]])
def test_head_against_float64(norm):
    N, C, Cout, S, _ = HEAD_CASES[1]
    fwd, got, d64 = head_case(N, C, Cout, S, norm, 1, seed=960)
    against64(f"head Cout={Cout} S={S} {norm[0]}", fwd, got, d64, 1)


def test_head_refuses_more_outputs_than_one_pass():
    """Cout above the 1x1x1 kernels' group: an error, and nothing written -- the caller keeps the materialising path."""
    from dram_amd import _lib
    assert _lib.lib.dram_norm_bwd_head_ok(8) == 1 and _lib.lib.dram_norm_bwd_head_ok(9) == 0
    assert _lib.lib.dram_norm_bwd_head_ok(0) == 0
    N, C, Cout, S = 1, 3, 9, 64
    fwd = Forward(N, C, S, NORMS[0], seed=970)
    gt = Placed((N, Cout, S), src=torch.randn(N, Cout, S, generator=g(971)))
    w = Placed((Cout, C), src=torch.randn(Cout, C, generator=g(972)))
    dx = Placed((N, C, S))
    with pytest.raises(_lib.DramHipError, match="Cout=9"):
        fwd.bwd("dram_norm_bwd_head", (p(gt.t), p(w.t), Cout), dx.t, 1)
    torch.cuda.synchronize()
    assert dx.intact() and bool(torch.isnan(dx.t).all())
