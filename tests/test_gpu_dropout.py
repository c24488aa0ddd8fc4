"""Device dropout (dram_dropout, functional.DropoutFn, modules.HipDropout) on the GPU.  The mask is pinned to its own
definition (include/dram_hip.h), restated in numpy by tests/philox_restatement.py: every comparison with it is bit for
bit.  ATen's mask depends on its launch geometry and cannot serve as a reference."""
import numpy as np
import pytest
import torch

from philox_restatement import dropout_mask, dropout_scale, threshold24

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = -12345.0
STREAMS = [(1234, 0), (2 ** 40 + 7, 2 ** 33 + 4)]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _expected(x, p, seed, offset):
    mask = dropout_mask(x.size, p, seed, offset)
    return np.where(mask, x * dropout_scale(p), np.float32(0.0)).astype(np.float32), mask


def _launch(xbuf, ybuf, lo, n, p, seed, offset):
    """dram_dropout on the n elements from element `lo` of two flat device buffers; returns the whole y buffer."""
    from dram_amd import _lib
    x, y = xbuf[lo:lo + n], ybuf[lo:lo + n]
    _lib.call("dram_dropout", x.data_ptr(), y.data_ptr(), n, threshold24(p), float(dropout_scale(p)), seed, offset,
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return ybuf.cpu().numpy()


@pytest.mark.parametrize("seed,offset", STREAMS)
def test_mask_and_values_are_exact(seed, offset):
    """y == where(mask, x * scale, +0) bit for bit for sizes around the group of four and the block of 1024 elements (the
    16-byte kernel plus the tail group, more than one block), for p = 0.1, 0.5 and 1, with seed and offset words above
    2^32; the elements before and after the tensor are not written.  Group indices above 2^32 (the high counter word of
    the element index) would need a 16 GB tensor and are not tested."""
    rng = np.random.default_rng(3)
    for n in (1, 3, 4, 5, 1023, 1024, 1025, 3074):
        xh = rng.standard_normal(n + 8).astype(np.float32)
        xh[xh == 0] = 1.0
        xbuf = torch.from_numpy(xh).to(DEV)
        assert xbuf.data_ptr() % 16 == 0
        for p in (0.1, 0.5, 1.0):
            ybuf = torch.full((n + 8,), GUARD, dtype=torch.float32, device=DEV)
            got = _launch(xbuf, ybuf, 4, n, p, seed, offset)          # element 4: 16-byte aligned on both sides
            want, mask = _expected(xh[4:4 + n], p, seed, offset)
            assert np.array_equal(_bits(got[4:4 + n]), _bits(want)), (n, p)
            assert (got[:4] == GUARD).all() and (got[4 + n:] == GUARD).all(), (n, p)
            if p == 1.0:
                assert not mask.any() and (_bits(got[4:4 + n]) == 0).all()


@pytest.mark.parametrize("seed,offset", STREAMS)
def test_unaligned_tensors_get_the_same_mask(seed, offset):
    """A source and a destination that are only 4-byte aligned (buf[1:1027] of 1028 elements) take the scalar kernel: same
    mask, same values, guard elements on both sides untouched.  Also one side aligned and the other not."""
    rng = np.random.default_rng(4)
    xh = rng.standard_normal(1028).astype(np.float32)
    xh[xh == 0] = 1.0
    xbuf = torch.from_numpy(xh).to(DEV)
    want, mask = _expected(xh[1:1027], 0.5, seed, offset)
    assert mask.any() and not mask.all()
    ybuf = torch.full((1028,), GUARD, dtype=torch.float32, device=DEV)
    got = _launch(xbuf, ybuf, 1, 1026, 0.5, seed, offset)
    assert np.array_equal(_bits(got[1:1027]), _bits(want))
    assert got[0] == GUARD and got[1027] == GUARD
    # aligned source, unaligned destination
    from dram_amd import _lib
    xal = torch.from_numpy(xh[1:1027].copy()).to(DEV)
    ybuf = torch.full((1028,), GUARD, dtype=torch.float32, device=DEV)
    _lib.call("dram_dropout", xal.data_ptr(), ybuf[1:].data_ptr(), 1026, threshold24(0.5), 2.0, seed, offset,
              torch.cuda.current_stream().cuda_stream)
    got = ybuf.cpu().numpy()
    assert np.array_equal(_bits(got[1:1027]), _bits(want))
    assert got[0] == GUARD and got[1027] == GUARD


def test_dropped_elements_are_plus_zero():
    """A dropped NaN, infinity or negative value becomes +0 (a select, not a product with the mask); kept ones scale."""
    xh = np.tile(np.array([np.nan, np.inf, -np.inf, -1.0], dtype=np.float32), 256)
    xbuf, ybuf = torch.from_numpy(xh).to(DEV), torch.empty(1024, dtype=torch.float32, device=DEV)
    got = _launch(xbuf, ybuf, 0, 1024, 0.5, 1234, 8)
    mask = dropout_mask(1024, 0.5, 1234, 8)
    assert (_bits(got)[~mask] == 0).all()
    kept = got[mask]
    src = xh[mask]
    assert np.array_equal(np.isnan(kept), np.isnan(src))
    assert np.array_equal(kept[~np.isnan(src)], src[~np.isnan(src)] * np.float32(2.0))


def test_backward_recomputes_the_mask():
    from dram_amd import functional as HF
    p = 0.3
    g = torch.Generator().manual_seed(0)
    x = torch.rand((2, 3, 5, 6, 7), generator=g) + 0.5
    x = (x * (torch.randint(0, 2, x.shape, generator=g) * 2 - 1)).to(DEV).requires_grad_(True)     # no zeros
    dy = torch.randn(x.shape, generator=g).to(DEV)
    gen = torch.cuda.default_generators[0]
    torch.manual_seed(11)
    seed, offset = gen.initial_seed(), gen.get_offset()
    y = HF.dropout(x, p)
    assert y.grad_fn.saved_tensors == ()
    assert type(y.grad_fn).__name__ == "DropoutFnBackward"
    y.backward(dy)
    want, mask = _expected(x.detach().cpu().numpy().reshape(-1), p, seed, offset)
    assert np.array_equal(_bits(y.detach().cpu().numpy().reshape(-1)), _bits(want))
    yh, dyh = y.detach().cpu().numpy(), dy.cpu().numpy()
    assert np.array_equal(yh.reshape(-1) != 0, mask) and mask.any() and not mask.all()
    dx = np.where(yh != 0, dyh * dropout_scale(p), np.float32(0.0)).astype(np.float32)
    assert np.array_equal(_bits(x.grad.cpu().numpy()), _bits(dx))


def test_mask_follows_the_device_generator():
    from dram_amd import functional as HF
    x = torch.ones(4099, device=DEV)
    gen = torch.cuda.default_generators[0]
    torch.manual_seed(77)
    o0 = gen.get_offset()
    a = HF.dropout(x, 0.5)
    o1 = gen.get_offset()
    b = HF.dropout(x, 0.5)
    o2 = gen.get_offset()
    assert (o1, o2) == (o0 + 4, o0 + 8)
    assert not torch.equal(a, b)
    torch.manual_seed(77)
    assert gen.get_offset() == o0 and gen.initial_seed() == 77
    assert torch.equal(HF.dropout(x, 0.5), a)
    assert np.array_equal(a.cpu().numpy() != 0, dropout_mask(4099, 0.5, 77, o0))
    state = torch.cuda.get_rng_state(0)
    c = HF.dropout(x, 0.5)
    torch.cuda.set_rng_state(state, 0)
    assert torch.equal(HF.dropout(x, 0.5), c)
    assert torch.equal(c, b)            # the second call after the same seed


def test_checkpointed_block_replays_its_masks():
    """torch.utils.checkpoint restores the generator state before it runs the block's forward again, so the recomputed
    masks are the first run's: output, input gradient and parameter gradients equal those of the plain call from the same
    state bit for bit (conv, GroupNorm + ReLU and dropout kernels are all run-to-run deterministic: no atomics)."""
    import parts
    torch.manual_seed(5)
    block = parts.ConvBlock5d([3, 4], [4, 6], 0, (3, 3), False, (1, 1), dropout=0.25, norm_method="ln").to(DEV).train()
    g = torch.Generator().manual_seed(1)
    xh, gout = torch.randn((2, 3, 6, 8, 12), generator=g), torch.randn((2, 6, 6, 8, 12), generator=g).to(DEV)
    state = torch.cuda.get_rng_state(0)
    res = []
    for wrapped in (True, False):
        torch.cuda.set_rng_state(state, 0)
        block.zero_grad(set_to_none=True)
        x = xh.to(DEV).requires_grad_(True)
        out = parts.checkpoint_wrapper(block, 1, x) if wrapped else block(x)
        out.backward(gout)
        res.append((out.detach().clone(), x.grad.clone(), {k: p.grad.clone() for k, p in block.named_parameters()}))
    (o1, gx1, gp1), (o2, gx2, gp2) = res
    assert (o1 == 0).float().mean().item() > 0.25             # ReLU zeros plus a quarter of the rest: dropout ran
    assert torch.equal(o1, o2)
    assert torch.equal(gx1, gx2)
    for k in gp1:
        assert torch.equal(gp1[k], gp2[k]), k


def test_dropout_model_stays_on_the_library(monkeypatch):
    import models
    from dram_amd.configs import SLIM
    from dram_amd import engine

    def refuse(*a, **k):
        raise AssertionError("ATen dropout was called")
    monkeypatch.setattr(torch.nn.functional, "dropout", refuse)
    monkeypatch.setattr(torch, "dropout", refuse)
    torch.manual_seed(3)
    model = models.DC3D(**dict(SLIM, dropout=0.1)).to(DEV).train()
    assert not engine.supports(model)
    x = torch.randn((2, 1, 16, 16, 16), generator=torch.Generator().manual_seed(2)).to(DEV)
    out, _ = model(x)
    assert type(out.grad_fn).__name__ != "DC3DFusedFnBackward"
    out.square().mean().backward()
    for k, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    again, _ = model(x)
    assert not torch.equal(again, out)                         # training mode: another mask
    model.eval()
    with torch.no_grad():
        e1, _ = model(x)
        e2, _ = model(x)
    assert torch.equal(e1, e2) and torch.isfinite(e1).all()
