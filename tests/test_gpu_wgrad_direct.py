"""The two direct (27-tap) backward-weights kernels, conv3d_k3_wgrad_kernel (dword staging, any shape, the only one whose
channel tile may straddle the two tensors of a virtual concat) and conv3d_k3_wgrad_vec_kernel (16-byte staging), run
in-process: every volume here has D = 1, which has no plane pair for the Winograd kernels, so wgrad_plan sends it to the direct
family without an environment switch.  Each launch is bracketed by the library's launch counters (K3_WGRAD_DIRECT /
K3_WGRAD_VEC), so a case proves which kernel produced the dW it checks.

  pairs     the same 16 channels as one tensor (vec kernel) and as an 8 ++ 8 concat of two full-size tensors (scalar kernel,
            tile straddling both): same boxes, same split, same MFMA order -> the two dW are bit-equal.  64 output channels
            (64 co x 32 ci tile) and 128 (128 co x 16 ci tile).
  tails     a ragged x box with channel tails in both tile directions; a cropped second source on either kernel.
  pipeline  more boxes than blocks per tile: the box loop's `has_next` arm (load next, compute, barrier, store, barrier).

Bound against the fp64 reference: the 1e-4 (max-abs over max |reference|, and relative L2) that the backward-weights checks of
tests/test_gpu_parity.py use for these kernels.  The expected family and split of every case follow from wgrad_plan alone and
are confirmed without a device in the first test.
"""
import ctypes
import re

import pytest
import torch

N = 2
TOL = 1e-4
DHW = (1, 8, 32)
SKIP_DHW = (3, 11, 38)          # centre crop offsets (1, 2, 3)
BIG_DHW = (1, 64, 256)          # 512 boxes over two samples (the plan picks 32 x 2 x 1 at D = 1, not 16 x 2 x 2); 4 tiles at 64 -> 128
BIG_SCALAR_DHW = (1, 64, 252)   # the same boxes with a ragged last one per row: the scalar kernel

DIRECT, VEC = "conv3d_k3_wgrad_kernel", "conv3d_k3_wgrad_vec_kernel"
# (label, C1, C2, Cout, dhw, kernel)
PLAN = [
    ("pair64 one tensor", 16, 0, 64, DHW, VEC),
    ("pair64 8 ++ 8", 8, 8, 64, DHW, DIRECT),
    ("pair128 one tensor", 16, 0, 128, DHW, VEC),
    ("pair128 8 ++ 8", 8, 8, 128, DHW, DIRECT),
    ("tails ragged x", 20, 0, 72, (1, 8, 20), DIRECT),
    ("tails crop 64", 16, 16, 64, DHW, DIRECT),
    ("tails crop 128", 16, 16, 128, DHW, VEC),
    ("pipeline vec", 64, 0, 128, BIG_DHW, VEC),
    ("pipeline scalar", 64, 0, 128, BIG_SCALAR_DHW, DIRECT),
]


def _choice(c1, c2, co, dhw):
    """(family, kernel base name, (BX, BY, BZ)) of the launch for x = x1[N, c1] ++ x2[N, c2]."""
    from dram_amd import _lib
    buf = ctypes.create_string_buffer(96)
    kind = _lib.lib.dram_conv3d_k3_wgrad_choice(N, c1, c2, co, *dhw, 0, buf, len(buf))
    name = buf.value.decode()
    assert kind >= 0, name
    box = tuple(int(v) for v in re.findall(r"\d+", name.split("<", 1)[1])[:3])
    return kind, name.split("<")[0], box


def _split_and_boxes(ci, co, dhw):
    """Blocks per (ci, co) tile -- the workspace holds one partial dW per block of a tile -- and boxes of the volume."""
    from dram_amd import _lib
    slab = co * ci * 27 * 4
    ws = _lib.lib.dram_conv3d_k3_wgrad_ws_bytes(N, ci, co, *dhw)
    assert ws % slab == 0
    bx, by, bz = _choice(ci, 0, co, dhw)[2]
    d, h, w = dhw
    return ws // slab, N * -(-w // bx) * -(-h // by) * -(-d // bz)


def test_plan_without_a_device():
    """Every case runs the kernel it means to test, and the pipeline cases give a block more than one box."""
    from dram_amd import functional as HF
    family = {DIRECT: HF.K3_WGRAD_DIRECT, VEC: HF.K3_WGRAD_VEC}
    for label, c1, c2, co, dhw, kernel in PLAN:
        kind, base, _ = _choice(c1, c2, co, dhw)
        assert (base, kind) == (kernel, family[kernel]), label
    assert HF.crop_offsets(DHW, SKIP_DHW) == (1, 2, 3)
    # a pair shares its boxes and its split
    for co in (64, 128):
        assert _choice(16, 0, co, DHW)[2] == _choice(8, 8, co, DHW)[2]
    for dhw in (BIG_DHW, BIG_SCALAR_DHW):
        split, boxes = _split_and_boxes(64, 128, dhw)
        assert 1 <= split < boxes, (dhw, split, boxes)


def _rand(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _wgrad(x1, x2, dy, kernel):
    """dW of the library for x1 ++ crop(x2), asserting that exactly one launch of `kernel`'s family produced it."""
    from dram_amd import functional as HF
    family = {DIRECT: HF.K3_WGRAD_DIRECT, VEC: HF.K3_WGRAD_VEC}[kernel]
    dhw, co = tuple(dy.shape[2:]), dy.shape[1]
    ci = x1.shape[1] + (x2.shape[1] if x2 is not None else 0)
    src = HF.CatView(x1.cuda(), None if x2 is None else x2.cuda(), dhw, channels=ci)
    w = torch.empty(co, ci, 3, 3, 3, device="cuda")
    before = HF.conv_launch_counts()
    dw = HF.conv3d_k3_launch_wgrad(src, dy.cuda(), w)
    torch.cuda.synchronize()
    after = HF.conv_launch_counts()
    moved = {k: after[k] - before[k] for k in range(HF.K3_KINDS) if after[k] != before[k]}
    assert moved == {family: 1}, (kernel, moved)
    return dw.cpu()


def _ref(x1, x2, dy):
    """fp64 dW[co][ci][3][3][3] of a D = 1 volume: the kz = 0 and kz = 2 planes only ever meet the zero padding."""
    n, co, d, h, w = dy.shape
    assert d == 1
    x = x1.double()
    if x2 is not None:
        assert (d, h, w) == DHW and tuple(x2.shape[2:]) == SKIP_DHW
        oz, oy, ox = 1, 2, 3        # ceil of half the size difference per axis, written out: independent of the library
        x = torch.cat([x, x2[:, :, oz:oz + d, oy:oy + h, ox:ox + w].double()], 1)
    xp = torch.nn.functional.pad(x[:, :, 0], (1, 1, 1, 1))
    g = dy.double()[:, :, 0].permute(1, 0, 2, 3).reshape(co, -1)
    ref = torch.zeros(co, x.shape[1], 3, 3, 3, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            ref[:, :, 1, ky, kx] = g @ xp[:, :, ky:ky + h, kx:kx + w].permute(1, 0, 2, 3).reshape(x.shape[1], -1).T
    return ref


def _check(got, ref, what):
    scale = max(ref.abs().max().item(), 1e-30)
    mx = (got.double() - ref).abs().max().item() / scale
    l2 = ((got.double() - ref).norm() / max(ref.norm().item(), 1e-30)).item()
    print(f"{what}: max-rel {mx:.3e}, rel-L2 {l2:.3e}")
    assert mx <= TOL and l2 <= TOL, f"{what}: max-rel {mx:.3e}, rel-L2 {l2:.3e} > {TOL}"


@pytest.mark.gpu
@pytest.mark.parametrize("co", [64, 128])
def test_one_tensor_and_straddling_concat_are_bit_equal(co):
    """16 channels on the vec kernel and as 8 ++ 8 on the scalar kernel (src_mode 2: every load is the sum of one tensor's
    value and the other's out-of-range zero): the same products in the same order."""
    x, dy = _rand(11, N, 16, *DHW), _rand(12, N, co, *DHW)
    one = _wgrad(x, None, dy, VEC)
    cat = _wgrad(x[:, :8].contiguous(), x[:, 8:].contiguous(), dy, DIRECT)
    assert torch.equal(one, cat)
    _check(one, _ref(x, None, dy), f"vec, 16 -> {co}")


@pytest.mark.gpu
def test_ragged_box_and_channel_tails():
    """W = 20 in 32-wide boxes, 20 of 2 x 16 input channels, 72 of 128 output channels."""
    x, dy = _rand(21, N, 20, 1, 8, 20), _rand(22, N, 72, 1, 8, 20)
    _check(_wgrad(x, None, dy, DIRECT), _ref(x, None, dy), "scalar, 20 -> 72, W = 20")


@pytest.mark.gpu
@pytest.mark.parametrize("co,kernel", [(64, DIRECT), (128, VEC)])
def test_cropped_second_source(co, kernel):
    """16 ++ crop of [16, 3, 11, 38]: the 32-channel tile of 64 output channels straddles the two tensors (scalar kernel); the
    16-channel tiles of 128 output channels lie inside one each (vec kernel, the second tile reads the crop window)."""
    x1, x2, dy = _rand(31, N, 16, *DHW), _rand(32, N, 16, *SKIP_DHW), _rand(33, N, co, *DHW)
    _check(_wgrad(x1, x2, dy, kernel), _ref(x1, x2, dy), f"16 ++ crop 16 -> {co}")


@pytest.mark.gpu
@pytest.mark.parametrize("dhw,kernel", [(BIG_DHW, VEC), (BIG_SCALAR_DHW, DIRECT)])
def test_more_boxes_than_blocks(dhw, kernel):
    """64 -> 128 over 512 boxes: 4 tiles share at most 1024 blocks, so a block walks several boxes through the pipeline."""
    split, boxes = _split_and_boxes(64, 128, dhw)
    assert 1 <= split < boxes, (split, boxes)
    x, dy = _rand(41, N, 64, *dhw), _rand(42, N, 128, *dhw)
    _check(_wgrad(x, None, dy, kernel), _ref(x, None, dy), f"{kernel}, 64 -> 128, {dhw}, split {split} of {boxes} boxes")
