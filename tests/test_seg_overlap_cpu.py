"""CPU checks of the SegOverlap loss (per-sample Tversky + focal on logits; include/dram_hip.h): the ABI surface and every
refusal of the entry points (nothing is launched), the fp64 restatement's closed-form gradient against torch's autograd of
the same formula, the decomposition over micro-batches that makes the loss fit DataParallelTrainer, and the plumbing of
Batch.supervised as far as it needs no kernel."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import seg_overlap_restatement as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ("dram_seg_overlap_ws_bytes", "dram_seg_overlap_state_floats", "dram_seg_overlap_fwd", "dram_seg_overlap_bwd")


def _case(seed, shape=(3, 1, 5, 6, 7), scale=1.0, voi_share=0.6, t_share=0.3):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(shape, generator=g, dtype=torch.float64) * scale
    voi = torch.rand(shape, generator=g) < voi_share
    t = torch.rand(shape, generator=g) < t_share          # set outside the voi too: it must not count there
    return z, t, voi


def test_abi_surface_and_size_queries_without_a_gpu():
    from dram_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dram_hip.h")).read(), flags=re.S)
    decl = {}
    for m in re.finditer(r"\b(?:int|size_t|const char\*)\s+(dram_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        args = m.group(2).strip()
        decl[m.group(1)] = 0 if args in ("", "void") else len(args.split(","))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in zip(NAMES, (2, 1, 17, 13)):
        assert decl[name] == nargs and len(_lib.SIGNATURES[name][1]) == nargs and hasattr(lib, name), name
    assert _lib.SIGNATURES[NAMES[0]][0] is ctypes.c_size_t and _lib.SIGNATURES[NAMES[1]][0] is ctypes.c_int
    assert _lib.lib.dram_abi_version() == 2
    chunk = _lib.lib.dram_seg_loss_chunk()
    ws, st = _lib.lib.dram_seg_overlap_ws_bytes, _lib.lib.dram_seg_overlap_state_floats
    # 8 fp64 totals per sample, then one tuple of 5 fp64 partials per block, a block never spanning two samples
    assert ws(0, 10) == 0 and ws(3, 0) == 0 and ws(-1, 10) == 0
    assert ws(2, 7) == 2 * (8 + 5) * 8
    assert ws(3, chunk) == 3 * (8 + 5) * 8 and ws(3, chunk + 5) == 3 * (8 + 2 * 5) * 8 and ws(1, 3 * chunk) == (8 + 3 * 5) * 8
    assert st(0) == 0 and st(-2) == 0 and st(1) == 5 and st(16) == 80


def _fwd(**kw):
    q = 64      # a non-null dummy: every call below must be refused before anything is launched
    a = dict(z=q, t=q, voi=q, kt=2, kv=0, N=2, S=10, a=.5, b=.5, s=1.0, alpha=.5, gamma=2.0, out=q, state=q, ws=q,
             ws_bytes=1 << 20)
    a.update(kw)
    return ("dram_seg_overlap_fwd", a["z"], a["t"], a["voi"], a["kt"], a["kv"], a["N"], a["S"], a["a"], a["b"], a["s"],
            a["alpha"], a["gamma"], a["out"], a["state"], a["ws"], a["ws_bytes"], None)


def _bwd(**kw):
    q = 64
    a = dict(z=q, t=q, voi=q, kt=2, kv=0, N=2, S=10, alpha=.5, gamma=2.0, state=q, gout=q, dz=q)
    a.update(kw)
    return ("dram_seg_overlap_bwd", a["z"], a["t"], a["voi"], a["kt"], a["kv"], a["N"], a["S"], a["alpha"], a["gamma"],
            a["state"], a["gout"], a["dz"], None)


INF, NAN = float("inf"), float("nan")
FWD_REFUSED = [dict(N=-1), dict(S=-1), dict(kt=1), dict(kt=3), dict(kv=1), dict(a=-0.1), dict(a=INF), dict(a=NAN),
               dict(b=-1e-9), dict(b=INF), dict(b=NAN), dict(gamma=-0.5), dict(gamma=INF), dict(gamma=NAN), dict(s=0.0),
               dict(s=-1.0), dict(s=NAN), dict(alpha=-0.01), dict(alpha=1.01), dict(alpha=NAN), dict(z=None), dict(t=None),
               dict(out=None), dict(state=None), dict(ws=None)]
BWD_REFUSED = [dict(N=-1), dict(S=-1), dict(kt=1), dict(kv=5), dict(gamma=-0.5), dict(gamma=NAN), dict(alpha=2.0),
               dict(alpha=NAN), dict(z=None), dict(t=None), dict(state=None), dict(gout=None), dict(dz=None)]


@pytest.mark.parametrize("kw", FWD_REFUSED, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_forward_refusals_through_call(kw):
    from dram_amd import _lib
    with pytest.raises(_lib.DramHipError, match=r"dram_seg_overlap_fwd failed \(-1\)"):
        _lib.call(*_fwd(**kw))


@pytest.mark.parametrize("kw", BWD_REFUSED, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_backward_refusals_through_call(kw):
    from dram_amd import _lib
    with pytest.raises(_lib.DramHipError, match=r"dram_seg_overlap_bwd failed \(-1\)"):
        _lib.call(*_bwd(**kw))


def test_short_workspace_and_empty_batches_through_call():
    from dram_amd import _lib
    need = _lib.lib.dram_seg_overlap_ws_bytes(2, 10)
    with pytest.raises(_lib.DramHipError, match=r"failed \(-2\).*workspace too small"):
        _lib.call(*_fwd(ws_bytes=need - 8))
    with pytest.raises(_lib.DramHipError, match=r"failed \(-1\).*aligned"):
        _lib.call(*_fwd(ws=68))
    # a bad parameter is refused even where there is nothing to do; otherwise N S == 0 launches nothing and needs no pointer
    with pytest.raises(_lib.DramHipError, match=r"failed \(-1\)"):
        _lib.call(*_fwd(N=0, s=0.0))
    for kw in (dict(N=0), dict(S=0)):
        none = dict(z=None, t=None, voi=None, out=None, state=None, ws=None, ws_bytes=0)
        _lib.call(*_fwd(**kw, **none))
        _lib.call(*_bwd(**kw, z=None, t=None, voi=None, state=None, gout=None, dz=None))
    # a NULL voi is no error (every voxel counts) and its kind is then not looked at: the refusal below is the workspace's
    with pytest.raises(_lib.DramHipError, match=r"failed \(-2\)"):
        _lib.call(*_fwd(voi=None, kv=7, ws_bytes=8))


PARAMS = [(.5, .5, 1.0, .5, 2.0), (.3, .7, 1e-3, .25, 1.5), (0.0, 1.0, 2.0, 0.0, 0.0), (.7, .6, .5, 1.0, 1.0)]


@pytest.mark.parametrize("a,b,s,alpha,gamma", PARAMS)
@pytest.mark.parametrize("with_voi", [True, False])
def test_restatement_value_and_gradient_equal_torch_autograd_fp64(a, b, s, alpha, gamma, with_voi):
    z, t, voi = _case(1, scale=2.0)
    z.view(-1)[:4] = torch.tensor([100.0, -100.0, 40.0, -40.0], dtype=torch.float64)
    t.view(-1)[:4] = torch.tensor([True, True, False, False])
    voi.view(-1)[:4] = True
    voi[1] = False                                        # one sample with an empty volume of interest
    v = voi if with_voi else None
    for gout in ((1.0, 0.0), (0.0, 1.0), (0.7, -1.3)):
        zz = z.clone().requires_grad_(True)
        out = R.torch_seg_overlap(zz, t, v, a, b, s, alpha, gamma)
        (out * torch.tensor(gout, dtype=torch.float64)).sum().backward()
        got = R.seg_overlap(z.numpy(), t.numpy(), None if v is None else v.numpy(), a, b, s, alpha, gamma)
        assert np.abs(got - out.detach().numpy()).max() <= 1e-12 * max(1.0, np.abs(got).max())
        grad = R.seg_overlap_grad(z.numpy(), t.numpy(), None if v is None else v.numpy(), a, b, s, alpha, gamma, gout)
        ref = zz.grad.numpy()
        assert np.isfinite(grad).all() and np.isfinite(ref).all()
        assert np.abs(grad - ref).max() <= 1e-12 * np.abs(ref).max()
        if with_voi:
            assert (grad[~voi.numpy()] == 0).all() and (grad[1] == 0).all()


def test_special_cases_of_the_definition():
    z, t, voi = _case(2)
    zn, tn, vn = z.numpy(), t.numpy(), voi.numpy()
    # gamma = 0 with alpha = 0.5 is half the plain BCE, per sample inside the voi, then averaged over samples
    bce = torch.nn.functional.binary_cross_entropy_with_logits(z, t.double(), reduction="none")
    want = np.mean([(bce[n][voi[n]]).mean().item() for n in range(z.shape[0])]) / 2
    assert abs(R.seg_overlap(zn, tn, vn, alpha=.5, gamma=0.0)[1] - want) <= 1e-12 * want
    # a = b = 0.5 is soft Dice
    p = torch.sigmoid(z)
    dice = [1 - (2 * (p[n] * t[n] * voi[n]).sum() + 2.0) / ((p[n] * voi[n]).sum() + (t[n] & voi[n]).sum() + 2.0) for n in range(3)]
    assert abs(R.seg_overlap(zn, tn, vn, .5, .5, 1.0)[0] - float(sum(dice))) <= 1e-12
    # an empty volume of interest contributes nothing and produces no NaN; a perfect saturated prediction has TI = 1
    vn0 = vn.copy()
    vn0[0] = False
    out = R.seg_overlap(zn, tn, vn0)
    rest = R.seg_overlap(zn[1:], tn[1:], vn[1:])
    assert np.isfinite(out).all() and abs(out[0] - rest[0]) <= 1e-12 and abs(out[1] - rest[1] * 2 / 3) <= 1e-12
    sat = np.where(tn, 100.0, -100.0)
    out = R.seg_overlap(sat, tn, vn)
    assert abs(out[0]) <= 1e-12 and 0 <= out[1] <= 1e-40
    assert np.isfinite(R.seg_overlap_grad(-sat, tn, vn)).all() and np.isfinite(R.seg_overlap(-sat, tn, vn)).all()


@pytest.mark.parametrize("split", [(2, 4), (1, 2, 3), (6,)])
def test_share_weighted_micro_batch_terms_add_up_to_the_whole_batch(split):
    """The trainer's rule: the first term of every micro-batch adds up, every later term enters with len(micro) / n_global.
    For this loss both hold with no deviation, for the value and for the gradient."""
    z, t, voi = _case(3, shape=(6, 1, 4, 5, 6), scale=1.5)
    voi[4] = False
    zn, tn, vn = z.numpy(), t.numpy(), voi.numpy()
    prm = (.3, .7, 1.0, .25, 2.0)
    whole, gwhole = R.seg_overlap(zn, tn, vn, *prm), R.seg_overlap_grad(zn, tn, vn, *prm, gout=(2.0, 0.5))
    n, parts, grads = zn.shape[0], np.zeros(2), []
    bounds = [0] + [int(k) for k in np.cumsum(split)]
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        share = (hi - lo) / n
        out = R.seg_overlap(zn[lo:hi], tn[lo:hi], vn[lo:hi], *prm)
        parts += np.array([out[0], out[1] * share])
        grads.append(R.seg_overlap_grad(zn[lo:hi], tn[lo:hi], vn[lo:hi], *prm, gout=(2.0, 0.5 * share)))
    assert bounds[-1] == n
    assert np.abs(parts - whole).max() <= 1e-13 * np.abs(whole).max()
    assert np.abs(np.concatenate(grads) - gwhole).max() <= 1e-13 * np.abs(gwhole).max()


def test_supervised_batch_plumbing_without_a_kernel():
    from dram_amd.train_step import (Batch, DeviceIntRegAffLoss, DeviceIntRegAffRefineLoss, DeviceIntRegLoss,
                                     DeviceIntRegRefineLoss, DeviceSegOverlapLoss)
    images = torch.rand(4, 1, 3, 4, 5)
    lobes = (torch.rand(4, 1, 3, 4, 5) < 0.7).float()
    labels = (torch.rand(4, 1, 3, 4, 5) < 0.3).to(torch.uint8)
    b = Batch.supervised(images, lobes, labels)
    assert len(b) == 4 and b.lesions is labels and b.lobes is lobes and b.images is images
    assert b.ctss is None and b.targets is None and b.weight is None and b.keep is None
    m = b.micro(1, 3)
    assert len(m) == 2 and torch.equal(m.lesions, labels[1:3]) and torch.equal(m.images, images[1:3]) and m.targets is None
    flipped = b.augmented(lambda s: {k: (v.flip(-1) if k.startswith("#") else v) for k, v in s.items()})
    assert torch.equal(flipped.lesions, labels.flip(-1)) and torch.equal(flipped.lobes, lobes.flip(-1))
    assert flipped.targets is None and len(flipped.micro(0, 1)) == 1
    dense = torch.zeros(4, 1, 3, 4, 5)
    for loss in (DeviceIntRegRefineLoss(), DeviceIntRegLoss()):
        with pytest.raises(ValueError, match="Batch.supervised"):
            loss(dense, b)
        with pytest.raises(ValueError, match="Batch.supervised"):
            loss(dense, m)
    for loss in (DeviceIntRegAffRefineLoss(0.1), DeviceIntRegAffLoss(0.1)):
        with pytest.raises(ValueError, match="Batch.supervised"):
            loss(lambda *a: pytest.fail("the model must not run"), b, transform=lambda s: s)
    with pytest.raises(ValueError, match="no CT severity scores"):
        b.ctss_device()
    fn = DeviceSegOverlapLoss(a=.3, b=.7, smooth=2.0, alpha=.25, gamma=1.5)
    assert (fn.a, fn.b, fn.smooth, fn.alpha, fn.gamma) == (.3, .7, 2.0, .25, 1.5) and not getattr(fn, "calls_model", False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn(dense, b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn(dense, b, refined=dense.clone())


def test_public_classes_and_host_side_checks():
    import dram_amd
    from dram_amd import functional as HF
    from dram_amd import losses
    for name in ("TverskyLoss", "SoftDiceLoss", "FocalLoss"):
        assert getattr(dram_amd, name) is getattr(losses, name) and name in dram_amd.__all__
    d = losses.SoftDiceLoss(2.0)
    assert isinstance(d, losses.TverskyLoss) and (d.a, d.b, d.smooth) == (.5, .5, 2.0)
    assert (losses.TverskyLoss(.3, .7).a, losses.TverskyLoss(.3, .7).b, losses.TverskyLoss().smooth) == (.3, .7, 1.0)
    assert (losses.FocalLoss().alpha, losses.FocalLoss().gamma) == (.5, 2.0)
    x = torch.zeros(2, 1, 3, 3, 3)
    for fn in (losses.TverskyLoss(), d, losses.FocalLoss(), HF.seg_overlap, HF.seg_overlap_totals):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x, x, x)
    assert "SegOverlapFn" in vars(HF)
