"""DataParallelTrainer with the losses that run the model themselves (DeviceIntRegAffRefineLoss, DeviceIntRegAffLoss:
`calls_model`, three terms, one transform per step) against the step written by hand: loss(model, batch, transform=T),
the weighted sum, backward(), opt.step().  The model is the closed-form three-output stand-in of the affine fixtures
(tests/intreg_restatement.py) with its three scalars as the parameter, and -- where the two forward tapes of one backward
through the fused engine are the point -- the slim DC3D with its dense output as the third.  Volumes are 16^3 and every
test fixes the transform."""
import math
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from intreg_restatement import aff_standin
from test_gpu_dp import _model, _setup_paths

pytestmark = pytest.mark.gpu
SIZE, LR = 16, 1e-2
FACTORS = [2.0, 1.0, 0.5, 0.5]             # LOSS_FACTORS of st_dram_ref*.py: the trainer takes the first three
LOSSES = ["DeviceIntRegAffRefineLoss", "DeviceIntRegAffLoss"]


class StandIn(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.theta = torch.nn.Parameter(torch.tensor([0.8, -0.3, 0.5]))

    def forward(self, imgs, lbs):
        return aff_standin(self.theta)(imgs, lbs)


class ThreeOut(torch.nn.Module):
    """DC3D (dense, refined) with the dense map once more as the 1-channel third output."""

    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, imgs, lbs):
        dense, refined = self.net(imgs, lbs)
        return dense, refined, dense


def _make_model(kind):
    return (StandIn() if kind == "standin" else ThreeOut(_model("ln"))).cuda().train()


def _transform(kind):
    """A fixed T in the form get_affine_transform returns.  "all3" changes the size (trilinear / nearest resampling)."""
    from dram_amd.transforms import Flip3DOneShot, Rescale3DOneShot, Rotate903DOneShot
    chosen = {"all3": [Rescale3DOneShot(None, scale_factor=(12, 16, 20)), Flip3DOneShot(flip_axis=(3,)),
                       Rotate903DOneShot(rotate_axis=(2, 3), rotate_times=3)],
              "fliprot": [Flip3DOneShot(flip_axis=(2, 4)), Rotate903DOneShot(rotate_axis=(3, 4), rotate_times=1)]}[kind]

    def apply(sample):
        for t in chosen:
            sample = t(sample)
        return sample
    apply.p = chosen
    return apply


def _loss(name, T):
    """The loss with its draw fixed to T (what the trainer asks for once per step)."""
    from dram_amd import train_step as TS
    kw = dict(rescale_jitter=[12, 16, 20], band_width=5e-2)
    loss = TS.DeviceIntRegAffRefineLoss(smoothing=0.05, **kw) if name == "DeviceIntRegAffRefineLoss" else TS.DeviceIntRegAffLoss(**kw)
    loss.draw = lambda: T
    return loss


def _batch(n, seed):
    from dram_amd.train_step import synthetic_batch
    return synthetic_batch(n, SIZE, seed, torch.device("cuda", 0))


def _weighted(terms):
    return FACTORS[0] * terms[0] + FACTORS[1] * terms[1] + FACTORS[2] * terms[2]


def _params(m):
    return {k: v.detach().clone() for k, v in m.named_parameters()}


@pytest.mark.parametrize("name", LOSSES)
def test_trainer_runs_a_loss_that_calls_the_model(name):
    from dram_amd.train_step import DataParallelTrainer
    m = _make_model("standin")
    before = _params(m)
    tr = DataParallelTrainer(m, torch.optim.Adam(m.parameters(), lr=LR), loss_fn=_loss(name, _transform("all3")),
                             loss_factors=[2.0, 1.0, 0.5])
    out = tr.step(_batch(3, 500))
    assert isinstance(out, tuple) and len(out) == 3
    for t in out:
        assert t.is_cuda and t.dim() == 0 and not t.requires_grad and math.isfinite(float(t))
    assert tr.overlapped_buckets == 0
    for k, v in m.named_parameters():
        assert bool((v.detach() != before[k]).all()), k          # every element of every trainable parameter moved
    tr.probe(_batch(3, 500), micro_batch=2)                      # the probe takes the same calling convention
    assert all(p.grad is None for p in m.parameters())
    with pytest.raises(ValueError, match="3 terms"):
        DataParallelTrainer(m, torch.optim.Adam(m.parameters(), lr=LR), loss_fn=_loss(name, _transform("all3")),
                            loss_factors=[2.0, 1.0]).step(_batch(3, 500))


@pytest.mark.parametrize("model,tkind", [("standin", "all3"), ("dc3d", "fliprot")])
@pytest.mark.parametrize("name", LOSSES)
def test_trainer_step_equals_the_step_by_hand(name, model, tkind):
    """One micro-batch, one rank: the same kernels in the same order, so the same bits."""
    from dram_amd.train_step import DataParallelTrainer
    T = _transform(tkind)
    ma, mb = _make_model(model), _make_model(model)
    before = _params(ma)
    batch = _batch(3, 501)
    tr = DataParallelTrainer(ma, torch.optim.SGD(ma.parameters(), lr=LR), loss_fn=_loss(name, T), loss_factors=FACTORS)
    got = tr.step(batch)
    loss, opt = _loss(name, None), torch.optim.SGD(mb.parameters(), lr=LR)
    opt.zero_grad(set_to_none=True)
    terms = loss(mb, batch, transform=T)
    _weighted(terms).backward()
    opt.step()
    torch.cuda.synchronize()
    assert len(got) == len(terms) == 3
    for g, t in zip(got, terms):
        assert float(g) == float(t.detach())
    moved = 0
    for (k, a), (_, b) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.equal(a.detach(), b.detach()), k
        moved += bool((a.detach() != before[k]).any())
    assert moved >= 0.9 * len(before)


@pytest.mark.parametrize("name", LOSSES)
def test_micro_batches_add_up(name):
    """N = 4 as two micro-batches under one T: the first term is the whole batch's (a sum over samples), the weighted loss
    and the gradient are those of the two halves by hand, each later term with its share 1/2 (tolerances of test_gpu_dp.py)."""
    from dram_amd.train_step import DataParallelTrainer
    T = _transform("all3")
    ma, mb = _make_model("standin"), _make_model("standin")
    batch = _batch(4, 502)
    tr = DataParallelTrainer(ma, torch.optim.SGD(ma.parameters(), lr=LR), loss_fn=_loss(name, T), loss_factors=FACTORS)
    got = tr.step(batch, micro_batch=2)
    loss = _loss(name, None)
    with torch.no_grad():
        whole = loss(mb, batch, transform=T)
    first = float(whole[0])
    print(f"{name}: first term, trainer {float(got[0]):.8g}, whole batch {first:.8g}")
    assert abs(float(got[0]) - first) <= 1e-6 * max(1.0, abs(first))
    want = 0.0
    for lo in (0, 2):
        terms = loss(mb, batch.micro(lo, lo + 2), transform=T)
        part = FACTORS[0] * terms[0] + (FACTORS[1] * terms[1] + FACTORS[2] * terms[2]) * 0.5
        part.backward()
        want += float(part)
    have = float(_weighted(got))
    print(f"{name}: weighted loss, trainer {have:.8g}, halves by hand {want:.8g}")
    assert abs(have - want) <= 1e-5 * max(1.0, abs(want))
    ga, gb = ma.theta.grad.double(), mb.theta.grad.double()
    print(f"{name}: gradient, trainer {ga.tolist()}, halves by hand {gb.tolist()}")
    assert float((ga - gb).abs().max()) <= 1e-5 * float(gb.abs().max())
    assert float(gb.abs().min()) > 0.0


@pytest.mark.parametrize("which", ["dram_amd.optim.Adam", "torch.optim.Adam"])
def test_clipping_with_a_three_term_loss(which):
    """max_grad_norm small enough to clip: last_grad_norm is the norm of the gradient computed by hand, the update that of
    clip_grad_norm_ in front of the optimiser's step (what tests/test_gpu_clip_trainer.py holds the two-term step to)."""
    from dram_amd import optim as DO
    from dram_amd.train_step import DataParallelTrainer
    max_norm, name, T = 1e-3, LOSSES[0], _transform("all3")
    make = (lambda ps: DO.Adam(ps, lr=1e-3)) if which.startswith("dram_amd") else (lambda ps: torch.optim.Adam(ps, lr=1e-3))
    ma, mb = _make_model("standin"), _make_model("standin")
    before = _params(ma)
    batch = _batch(3, 503)
    tr = DataParallelTrainer(ma, make(ma.parameters()), loss_fn=_loss(name, T), loss_factors=FACTORS, max_grad_norm=max_norm)
    tr.step(batch)
    opt = make(mb.parameters())
    opt.zero_grad(set_to_none=True)
    _weighted(_loss(name, None)(mb, batch, transform=T)).backward()
    want64 = float(mb.theta.grad.double().norm())
    norm = DO.clip_grad_norm_(list(mb.parameters()), max_norm, 2.0)
    opt.step()
    torch.cuda.synchronize()
    got = tr.last_grad_norm
    print(f"{which}: gradient norm {float(got):.8g}, by hand in fp64 {want64:.8g}, max_norm {max_norm}")
    assert want64 > max_norm, "the case is meant to clip"
    assert got.shape == () and got.is_cuda
    assert abs(float(got) - want64) <= 1e-5 * want64
    assert float(got) == float(norm)
    assert torch.equal(ma.theta.detach(), mb.theta.detach())
    assert bool((ma.theta.detach() != before["theta"]).all())


@pytest.mark.parametrize("name", LOSSES)
def test_loss_call_reads_nothing_back(name, monkeypatch):
    """With T drawn before and the batch's scores on the device, loss(model, batch, transform=T) must not read from the
    device: Tensor.cpu / .item / .tolist raise inside the region, and so does every synchronising torch call where this
    build honours torch.cuda.set_sync_debug_mode("error")."""
    T = _transform("all3")
    m, loss, batch = _make_model("standin"), _loss(name, None), _batch(3, 504)
    batch.ctss_device()
    loss(m, batch, transform=T)                 # first use: modules loaded, allocator warm
    torch.cuda.synchronize()
    honoured = False
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device="cuda").item()
        except RuntimeError:
            honoured = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    print(f"torch.cuda.set_sync_debug_mode('error') honoured: {honoured}")

    def refuse(*a, **k):
        raise AssertionError("host read inside the loss")
    for attr in ("cpu", "item", "tolist", "numpy"):
        monkeypatch.setattr(torch.Tensor, attr, refuse)
    if honoured:
        torch.cuda.set_sync_debug_mode("error")
    try:
        terms = loss(m, batch, transform=T)
    finally:
        torch.cuda.set_sync_debug_mode("default")
        monkeypatch.undo()
    assert len(terms) == 3 and all(math.isfinite(float(t)) for t in terms)


def _worker(rank, world, port, backend, name, out):
    _setup_paths()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    try:
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", 0))
            probe = torch.ones(4, device="cuda")
            dist.all_reduce(probe)
            torch.cuda.synchronize()
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    except Exception as e:                        # two ranks on one device: RCCL refuses
        out[rank] = f"refused: {type(e).__name__}: {str(e)[:200]}"
        return
    from dram_amd.train_step import DataParallelTrainer
    m = _make_model("dc3d")
    tr = DataParallelTrainer(m, torch.optim.SGD(m.parameters(), lr=LR), loss_fn=_loss(name, _transform("fliprot")),
                             loss_factors=FACTORS, bucket_mb=0.05)
    assert tr.world == world and len(tr.buckets) > 3
    terms = tr.step(_batch(2, 510 + rank))
    torch.cuda.synchronize()
    out[rank] = {"params": {k: v.detach().cpu() for k, v in m.named_parameters()}, "terms": [float(t) for t in terms],
                 "overlapped": tr.overlapped_buckets}
    dist.destroy_process_group()


@pytest.mark.parametrize("backend", ["gloo", "nccl"])
def test_two_ranks_equal_one_rank_with_micro_batches(backend):
    """As tests/test_gpu_dp.py: two ranks with one shard each (the same T) against one rank running the shards as
    micro-batches, through two forward tapes per backward and the bucketed all-reduce after the last backward."""
    _setup_paths()
    from dram_amd.train_step import Batch, DataParallelTrainer
    world, name = 2, LOSSES[0]
    ctx = mp.get_context("spawn")
    out = ctx.Manager().dict()
    port = 30600 + (os.getpid() % 200) + (0 if backend == "gloo" else 250)
    procs = [ctx.Process(target=_worker, args=(r, world, port, backend, name, out)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
    hung = [p for p in procs if p.is_alive()]
    for p in hung:
        p.kill()
    res = dict(out)
    refused = [v for v in res.values() if isinstance(v, str)]
    if backend == "nccl" and (refused or hung or any(p.exitcode != 0 for p in procs)):
        pytest.skip("RCCL does not run two ranks on one device here "
                    f"({refused[0] if refused else 'init failed'}); the multi-GPU path is the driver's SCALE run")
    assert not hung and all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert set(res) == {0, 1}
    assert res[0]["overlapped"] == res[1]["overlapped"] == 0      # the gradient sink stays off for these losses

    m = _make_model("dc3d")
    sd0 = _params(m)
    tr = DataParallelTrainer(m, torch.optim.SGD(m.parameters(), lr=LR), loss_fn=_loss(name, _transform("fliprot")),
                             loss_factors=FACTORS)
    b0, b1 = _batch(2, 510), _batch(2, 511)
    cat = lambda a, b: torch.cat([a, b], 0)
    both = Batch(cat(b0.images, b1.images), cat(b0.lobes, b1.lobes), cat(b0.lesions, b1.lesions), b0.ctss + b1.ctss,
                 {k: 1.0 / 6 for k in range(6)})
    terms = tr.step(both, micro_batch=2)
    ref = {k: v.detach().cpu() for k, v in m.named_parameters()}
    for i, t in enumerate(terms):
        assert abs(res[0]["terms"][i] + res[1]["terms"][i] - float(t)) <= 1e-5 * max(1.0, abs(float(t))), i
    moved = 0
    for k, e in ref.items():
        step = (e - sd0[k].cpu()).abs().max().item()
        moved += step > 0.0
        for r in range(world):
            err = (res[r]["params"][k] - e).abs().max().item()
            assert err <= 1e-4 * step + 1e-9, (backend, r, k, err, step)
        assert torch.equal(res[0]["params"][k], res[1]["params"][k]), k
    assert moved >= 0.9 * len(ref)
