"""dram_crop_concat_fwd / dram_crop_concat_bwd (csrc/resample.hip: crop_concat_fwd_kernel, crop_concat_bwd1_kernel,
crop_concat_bwd2_kernel) through the C ABI with a NON-ZERO crop offset, against oracle.crop_concat_5d and its autograd.

The attention model, the only caller of the backward, crops by 0 on every axis, so the zero fill of dt2 outside the window
never ran on the device.  These are pure copies: torch.equal.  Outputs are NaN before the call and sit between guard words.
Shapes: t1 spatial (3, 5, 37) = 555 voxels (three blocks, the last with 43), t2 up to (4, 8, 42) = 1344 voxels (six blocks,
the last with 64); the three extents and the three offsets all differ, so swapped strides or offsets cannot cancel."""
import pytest
import torch

from dram_amd import _lib
from dram_amd import functional as HF
from oracle import dram_oracle as O

from gpu_buffers import DEV, Placed, g, p, stream

pytestmark = pytest.mark.gpu
N = 2
SMALL = (3, 5, 37)
# t2 spatial, offsets (None: the ceil rule of HF.crop_offsets, what the model passes)
GEOMETRY = {
    "z": ((5, 5, 37), None),                 # ceil(2 / 2) = 1 on z alone
    "y": ((3, 8, 37), None),                 # ceil(3 / 2) = 2 on y alone
    "x": ((3, 5, 40), None),                 # ceil(3 / 2) = 2 on x alone
    "zyx_odd": ((4, 8, 42), None),           # odd differences 1, 3, 5 -> offsets 1, 2, 3
    "zyx_far_end": ((4, 8, 42), (1, 3, 5)),  # the window ends on the last plane, row and column of t2
    "zyx_near_end": ((4, 8, 42), (0, 0, 0)),  # ... starts on the first, in a larger t2
}
CHANNELS = [(1, 1), (1, 3), (3, 1), (3, 3)]


def setup(geometry, C1, C2):
    big, offs = GEOMETRY[geometry]
    ceil = HF.crop_offsets(SMALL, big)
    if offs is None:
        offs = ceil
        assert offs == O.crop_offsets(SMALL, big) and any(offs)
    assert all(o + s <= b for o, s, b in zip(offs, SMALL, big))
    assert (SMALL[0] * SMALL[1] * SMALL[2]) % 256 and (big[0] * big[1] * big[2]) % 256
    t1 = torch.randn(N, C1, *SMALL, generator=g(11))
    t2 = torch.randn(N, C2, *big, generator=g(12))
    return big, offs, offs == ceil, t1, t2


def window(t, offs):
    (oz, oy, ox), (d, h, w) = offs, SMALL
    return t[:, :, oz:oz + d, oy:oy + h, ox:ox + w]


@pytest.mark.parametrize("C1,C2", CHANNELS)
@pytest.mark.parametrize("geometry", list(GEOMETRY))
def test_crop_concat_fwd(geometry, C1, C2):
    big, offs, is_ceil, t1, t2 = setup(geometry, C1, C2)
    out = Placed((N, C1 + C2) + SMALL)
    a, b = Placed(t1.shape, src=t1), Placed(t2.shape, src=t2)
    _lib.call("dram_crop_concat_fwd", p(a.t), p(b.t), p(out.t), N, C1, C2, *SMALL, *big, *offs, stream())
    torch.cuda.synchronize()
    assert out.intact() and a.intact() and b.intact()
    got = out.t.cpu()
    assert torch.equal(got, torch.cat([t1, window(t2, offs)], 1))
    if is_ceil:
        assert torch.equal(got, O.crop_concat_5d(t1, t2))


@pytest.mark.parametrize("C1,C2", CHANNELS)
@pytest.mark.parametrize("geometry", list(GEOMETRY))
def test_crop_concat_bwd(geometry, C1, C2):
    """dt1 = dout[:, :C1]; dt2 = dout[:, C1:] inside the window and exactly 0 outside.  Either output may be NULL
    (include/dram_hip.h): the other one is the same."""
    big, offs, is_ceil, t1, t2 = setup(geometry, C1, C2)
    dout = torch.randn(N, C1 + C2, *SMALL, generator=g(13))
    dout[dout == 0] = 1.0                          # so that "0 outside the window" cannot be met by a copied value
    d = Placed(dout.shape, src=dout)

    def run(want1, want2):
        dt1, dt2 = Placed(t1.shape), Placed(t2.shape)
        _lib.call("dram_crop_concat_bwd", p(d.t), p(dt1.t) if want1 else None, p(dt2.t) if want2 else None, N, C1, C2, *SMALL, *big,
                  *offs, stream())
        torch.cuda.synchronize()
        assert dt1.intact() and dt2.intact() and d.intact()
        return dt1.t.cpu(), dt2.t.cpu()

    dt1, dt2 = run(True, True)
    assert torch.equal(dt1, dout[:, :C1])
    inside = torch.zeros(N, C2, *big, dtype=torch.bool)
    window(inside, offs)[:] = True
    assert int(inside.sum()) == N * C2 * SMALL[0] * SMALL[1] * SMALL[2] and not bool(inside.all())
    assert bool((dt2[~inside] == 0).all())
    assert torch.equal(window(dt2, offs), dout[:, C1:])
    assert int((dt2 != 0).sum()) == int(inside.sum())
    if is_ceil:     # the oracle's autograd
        r1, r2 = t1.clone().requires_grad_(True), t2.clone().requires_grad_(True)
        O.crop_concat_5d(r1, r2).backward(dout)
        assert torch.equal(dt1, r1.grad) and torch.equal(dt2, r2.grad)
    only1, none2 = run(True, False)
    assert torch.equal(only1, dt1) and bool(torch.isnan(none2).all())
    none1, only2 = run(False, True)
    assert torch.equal(only2, dt2) and bool(torch.isnan(none1).all())


def test_crop_window_outside_the_second_tensor_is_refused():
    big = (4, 8, 42)
    for offs in ((2, 0, 0), (0, 4, 0), (0, 0, 6), (-1, 0, 0)):
        dt2 = Placed((N, 1) + big)
        dout = torch.ones(N, 2, *SMALL, device=DEV)
        rc = _lib.lib.dram_crop_concat_bwd(p(dout), None, p(dt2.t), N, 1, 1, *SMALL, *big, *offs, stream())
        torch.cuda.synchronize()
        assert rc == -1 and b"crop window outside" in _lib.lib.dram_last_error()
        assert dt2.intact() and bool(torch.isnan(dt2.t).all())
