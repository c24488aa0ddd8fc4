"""What the fused engine's backward (dram_amd/engine.py) promises besides its numbers: the order in which finished
parameter gradients reach `model.grad_sink` (with several ranks the bucket and "sbn" all-reduces are issued in that order on
every rank), what becomes of a gradient the sink takes, and that the tape's tensors are released as the walk passes them."""
import pytest
import torch

from dram_amd.configs import SLIM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _model(norm="bn", seed=21):
    import models
    torch.manual_seed(seed)
    model = models.DC3D(**SLIM, norm_method=norm)
    model.init(models.HeNorm(mode="fan_in"))
    return model.to(DEV).train()


def _input(N, shape, seed=22):
    return torch.rand((N, 1) + shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _step(model, x, sink=None):
    """One forward + backward of out.sum() through the engine; returns {name: p.grad (or None)}."""
    for p in model.parameters():
        p.grad = None
    model.grad_sink = sink
    try:
        out, _ = model(x)
        assert type(out.grad_fn).__name__ == "DC3DFusedFnBackward"
        out.sum().backward()
    finally:
        model.grad_sink = None
    return {k: (None if p.grad is None else p.grad.clone()) for k, p in model.named_parameters()}


def _order_from_the_module_tree(model):
    """Head weight, head bias; then per stage, from the last up-block's last stage back to the first down-block's first
    stage: norm weight, norm bias, conv weight (norms without affine parameters have none to deliver)."""
    want = [model.top_layer.weight, model.top_layer.bias]
    for block in reversed(list(model.ds_modules) + [model.bg] + list(model.us_modules)):
        for seq in reversed(block.conv_blocks):
            want += [seq[1].weight, seq[1].bias, seq[0].weight]
    return [p for p in want if p is not None]


@pytest.mark.parametrize("norm,N,shape,sliced", [
    ("bn", 2, (16, 16, 16), False),     # the smallest volume with all three pool levels (2^3 bottleneck)
    ("lnna", 2, (8, 8, 8), False),      # no affine parameters: head and conv weights only; 1^3 bottleneck
    ("bn", 3, (16, 24, 16), True),      # upsampled-input stages in slices of one sample, everything lazy
])
def test_sink_receives_gradients_in_tape_order(norm, N, shape, sliced, monkeypatch):
    from dram_amd import engine
    if sliced:
        monkeypatch.setattr(engine, "MEMORY_MODE", "manual")
        monkeypatch.setattr(engine, "MATERIALISE_BELOW", 0.0)
        monkeypatch.setattr(engine, "KEEP_UPSAMPLED_BELOW", 0.0)
        monkeypatch.setattr(engine, "SLICE_UPSAMPLED_ABOVE", 1e-12)
    model = _model(norm)
    name = {id(p): k for k, p in model.named_parameters()}
    seen = []

    def sink(p, g):
        assert g.shape == p.shape
        seen.append(p)
        return False

    grads = _step(model, _input(N, shape), sink)
    assert engine.LAST_PLAN.sliced_stages == (3 if sliced else 0)
    want = _order_from_the_module_tree(model)
    assert len(want) == (2 + 3 * 14 if norm == "bn" else 2 + 14)
    assert [name[id(p)] for p in seen] == [name[id(p)] for p in want]
    assert all(g is not None for g in grads.values())       # declined by the sink: every gradient comes back through autograd


def test_sink_takes_gradients():
    """A gradient the sink takes is the engine's gradient, bit for bit, and is not delivered a second time."""
    model = _model()
    x = _input(2, (16, 16, 16))
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    plain = _step(model, x)
    model.load_state_dict(sd0)
    norm_params = {id(p) for m in model.modules() if isinstance(m, torch.nn.BatchNorm3d) for p in m.parameters()}
    assert len(norm_params) == 2 * 14
    name = {id(p): k for k, p in model.named_parameters()}
    taken = {}

    def sink(p, g):
        if id(p) not in norm_params:
            return False
        assert name[id(p)] not in taken
        taken[name[id(p)]] = g
        return True

    got = _step(model, x, sink)
    assert set(taken) == {name[i] for i in norm_params}
    for k, g in got.items():
        if k in taken:
            assert g is None, k
            assert torch.equal(taken[k], plain[k]), k
        else:
            assert torch.equal(g, plain[k]), k


def test_backward_releases_the_tape():
    """The walk empties every stage entry behind it (raw output, coefficients, statistics, the output Lazy) and drops kept
    upsampled tensors; the autograd node lets go of the tape itself."""
    from dram_amd import engine
    model = _model()
    x = _input(2, (16, 16, 16))
    record = []
    with torch.no_grad():
        out, _ = engine.forward(model, x, record)
        stages = [e for e in record if isinstance(e, engine._Stage)]
        ups = [s.inp for s in stages if isinstance(s.inp, engine.Upsampled)]
        assert len(stages) == 14 and len(ups) == 3
        assert all(s.y is not None and s.out.raw is not None for s in stages)
        assert all(u.kept is not None for u in ups)         # small tensors: forward kept them for backward-weights
        grads, dx = engine.backward(model, record, torch.ones_like(out), True)
    assert dx.shape == x.shape and len(grads) == len(list(model.parameters()))
    for s in stages:
        assert s.y is None and s.coef is None and s.mean is None and s.rstd is None
        assert s.out.raw is None and s.out.coef is None
    assert all(u.kept is None for u in ups)
    out, _ = model(x)
    assert isinstance(out.grad_fn.record, list)
    out.sum().backward()
    assert out.grad_fn.record is None
