"""DataParallelTrainer(max_grad_norm=...): the clipped step against a twin that calls dram_amd.optim.clip_grad_norm_ in front
of the optimiser's own step(), the unclipped default against a trainer built without the argument, and two ranks against one
rank's micro-batches with clipping active.  models.DC3D(**SLIM), 2 chunks of 16^3 per step."""
import math
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_gpu_dp import _model, _setup_paths

pytestmark = pytest.mark.gpu
N, SIZE, LR, MAX_NORM = 2, 16, 1e-2, 0.5


def _batch(seed):
    from dram_amd.train_step import synthetic_batch
    return synthetic_batch(N, SIZE, seed, torch.device("cuda", 0))


class ClipThenStep:
    """What the trainer sees of an optimiser (zero_grad, step), with clip_grad_norm_ in front of the real step()."""

    def __init__(self, opt, params, max_norm, norm_type):
        self.opt, self.params, self.max_norm, self.norm_type = opt, list(params), max_norm, norm_type
        self.norm = None

    def zero_grad(self, set_to_none=True):
        self.opt.zero_grad(set_to_none=set_to_none)

    def step(self):
        from dram_amd import optim as DO
        self.norm = DO.clip_grad_norm_(self.params, self.max_norm, self.norm_type)
        self.opt.step()


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def _same(ma, mb, what):
    for (k, a), (_, b) in zip(ma.named_parameters(), mb.named_parameters()):
        assert np.array_equal(_bits(a), _bits(b)), (what, k)


@pytest.mark.parametrize("which", ["dram_amd.optim.Adam", "dram_amd.optim.SGD", "torch.optim.SGD"])
@pytest.mark.parametrize("norm_type", [2.0, math.inf])
def test_clipped_trainer_is_clip_then_step(which, norm_type):
    """Two steps, bit for bit, for an optimiser that takes the clipping into its step() (set_grad_clip) and for a plain torch
    one, which gets clip_grad_norm_ between the all-reduce and its step(); last_grad_norm is the stand-alone function's
    return value."""
    _setup_paths()
    from dram_amd import optim as DO
    from dram_amd.train_step import DataParallelTrainer
    make = {"dram_amd.optim.Adam": lambda ps: DO.Adam(ps, lr=1e-3), "dram_amd.optim.SGD": lambda ps: DO.SGD(ps, lr=LR, momentum=0.9),
            "torch.optim.SGD": lambda ps: torch.optim.SGD(ps, lr=LR, momentum=0.9)}[which]
    max_norm = MAX_NORM if norm_type == 2.0 else 0.05
    ma, mb = _model("ln").cuda().train(), _model("ln").cuda().train()
    sd0 = {k: v.detach().clone() for k, v in ma.named_parameters()}
    _same(ma, mb, "initial weights")
    ta = DataParallelTrainer(ma, make(ma.parameters()), max_grad_norm=max_norm, grad_norm_type=norm_type)
    wrapped = ClipThenStep(make(mb.parameters()), mb.parameters(), max_norm, norm_type)
    tb = DataParallelTrainer(mb, wrapped)
    assert ta.last_grad_norm is None and tb.last_grad_norm is None
    assert (ta.opt._clip is not None) if which.startswith("dram_amd") else not hasattr(ta.opt, "set_grad_clip")
    for k in range(2):
        batch = _batch(400 + k)
        ra, rb = ta.step(batch), tb.step(batch)
        torch.cuda.synchronize()
        assert float(ra[0]) == float(rb[0]) and float(ra[1]) == float(rb[1])
        norm = ta.last_grad_norm
        assert norm.shape == () and norm.is_cuda and norm.dtype == torch.float32
        assert np.array_equal(_bits(norm), _bits(wrapped.norm)), (k, float(norm), float(wrapped.norm))
        print(f"{which} norm_type={norm_type} step {k + 1}: gradient norm {float(norm):.6g}, max_norm {max_norm}")
        assert float(norm) > max_norm, "the case is meant to clip"
        assert tb.last_grad_norm is None
        _same(ma, mb, f"{which} step {k + 1}")
    assert sum(int((v.detach() != sd0[k]).any()) for k, v in ma.named_parameters()) >= 0.9 * len(sd0)


def test_default_is_the_unclipped_step():
    """max_grad_norm=None (the default) against a trainer built without the argument: the same launches, the same bits; and
    it differs from the clipped step, so the comparison can fail."""
    _setup_paths()
    from dram_amd import optim as DO
    from dram_amd.train_step import DataParallelTrainer
    models = [_model("ln").cuda().train() for _ in range(3)]
    trainers = [DataParallelTrainer(models[0], DO.Adam(models[0].parameters(), lr=1e-3)),
                DataParallelTrainer(models[1], DO.Adam(models[1].parameters(), lr=1e-3), max_grad_norm=None, grad_norm_type=2.0),
                DataParallelTrainer(models[2], DO.SGD(models[2].parameters(), lr=LR), max_grad_norm=MAX_NORM)]
    for k in range(2):
        batch = _batch(410 + k)
        for t in trainers:
            t.step(batch)
    torch.cuda.synchronize()
    _same(models[0], models[1], "max_grad_norm=None")
    assert trainers[0].last_grad_norm is None and trainers[1].last_grad_norm is None
    assert trainers[1].opt._clip is None and trainers[2].opt._clip == (MAX_NORM, 2)
    with pytest.raises(NotImplementedError, match="2.0 and inf"):
        DataParallelTrainer(models[0], torch.optim.SGD(models[0].parameters(), lr=LR), max_grad_norm=1.0, grad_norm_type=1)


def _worker(rank, world, port, out):
    _setup_paths()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from dram_amd import optim as DO
    from dram_amd.train_step import DataParallelTrainer
    m = _model("ln").cuda().train()
    tr = DataParallelTrainer(m, DO.SGD(m.parameters(), lr=LR), bucket_mb=0.05, max_grad_norm=MAX_NORM)
    assert tr.world == world and len(tr.buckets) > 3
    tr.step(_batch(420 + rank))
    torch.cuda.synchronize()
    out[rank] = {"params": {k: v.detach().cpu() for k, v in m.named_parameters()}, "norm": float(tr.last_grad_norm)}
    dist.destroy_process_group()


def test_two_ranks_clip_the_global_norm():
    """Two ranks over gloo with one shard each against one rank running both shards as micro-batches, clipping active: the
    norm is the summed gradient's, so the coefficient and the step are the same up to the order of the two-term gradient
    sum (the tolerance of test_two_rank_step_equals_one_rank_micro_batched_step)."""
    _setup_paths()
    from dram_amd import optim as DO
    from dram_amd.train_step import Batch, DataParallelTrainer
    world = 2
    ctx = mp.get_context("spawn")
    out = ctx.Manager().dict()
    port = 30300 + (os.getpid() % 200)
    procs = [ctx.Process(target=_worker, args=(r, world, port, out)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
    hung = [p for p in procs if p.is_alive()]
    for p in hung:
        p.kill()
    res = dict(out)
    assert not hung and all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert set(res) == {0, 1}

    m = _model("ln").cuda().train()
    sd0 = {k: v.detach().clone() for k, v in m.named_parameters()}
    tr = DataParallelTrainer(m, DO.SGD(m.parameters(), lr=LR), max_grad_norm=MAX_NORM)
    b0, b1 = _batch(420), _batch(421)
    cat = lambda a, b: torch.cat([a, b], 0)
    both = Batch(cat(b0.images, b1.images), cat(b0.lobes, b1.lobes), cat(b0.lesions, b1.lesions), b0.ctss + b1.ctss,
                 {k: 1.0 / 6 for k in range(6)})
    tr.step(both, micro_batch=N)
    ref = {k: v.detach().cpu() for k, v in m.named_parameters()}
    norm = float(tr.last_grad_norm)
    print(f"gradient norm of the global batch: one rank {norm:.7g}, two ranks {res[0]['norm']:.7g} / {res[1]['norm']:.7g}")
    assert norm > MAX_NORM, "the case is meant to clip"
    moved = 0
    for r in range(world):
        assert abs(res[r]["norm"] - norm) <= 1e-5 * norm       # as that test holds the summed losses
    assert res[0]["norm"] == res[1]["norm"]
    for k, e in ref.items():
        step = (e - sd0[k].cpu()).abs().max().item()
        moved += step > 0.0
        for r in range(world):
            err = (res[r]["params"][k] - e).abs().max().item()
            assert err <= 1e-4 * step + 1e-9, (r, k, err, step)
        assert torch.equal(res[0]["params"][k], res[1]["params"][k]), k
    assert moved >= 0.9 * len(ref)
