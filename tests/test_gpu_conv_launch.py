"""The three host launch helpers of the 3x3x3 conv (functional.conv3d_k3_launch_fwd / _bwd_data / _wgrad): the kernel name
the KernelTimer records for a call is the kernel that ran.

Each helper derives the facts of its name query (source tensors, crop x offset, 16-byte alignment, destination split, lazy
or not) from the objects it launches on.  The library's launch counters say which family really ran: around ONE helper call
with a timer installed exactly one family's counter moves, and it is the family of the single recorded key; the same call
with TIMER = None (no name query at all) moves the same counter and gives bit-equal outputs.

All shapes: N = 2, (D, H, W) = (4, 8, 32), Cout = 64 -- the smallest volume the 32-wide (z,y) forward kernel accepts.  The
expected forward names follow from the library's own rules (checked without a device in the first test):
  (a) 16 aligned channels                         -> conv3d_k3_fwd_wzy_kernel
  (b) 8 channels ++ crop of [2, 8, 6, 11, 38]     -> crop x offset ceil(6 / 2) = 3, not a multiple of 4: the z-only kernel on
                                                     the same boxes, conv3d_k3_fwd_wz_kernel<32, 4, 2, false>
  (c) (a) one float into a larger buffer          -> data_ptr() % 16 == 4: the z-only kernel as well
  (d) fused forward of (a) with statistics        -> conv3d_k3_fwd_wzy_kernel
Backward-weights with a lazy source: for (b)'s 8 + 8 channels the library has no on-load path (the concat boundary is no
multiple of 16: dram_conv3d_k3_wgrad_lazy_ok is 0 and a launch with coefficients is an argument error), so -- as the engine
does -- the skip source is materialised first; the recorded key still equals conv_wgrad_kernel_name(..., lazy=True), which
names the direct kernel for that shape.  The truly lazy launch runs on 16 ++ crop of [2, 16, 6, 11, 38] with coefficients on
the skip source only: one call, two per-source launches, its family's counter moves by two.
"""
import ctypes

import pytest
import torch

N, DHW, CO = 2, (4, 8, 32), 64
SKIP_DHW = (6, 11, 38)
WZ_SAME_BOXES = "conv3d_k3_fwd_wz_kernel<32, 4, 2, false>"


def _family(name):
    """K3_* family of a kernel name as the choice queries write it."""
    from dram_amd import functional as HF
    base = name.split("<")[0]
    if base == "conv3d_k3_wgrad_wz_kernel":
        assert name.endswith(("true>", "false>")), name
        return HF.K3_WGRAD_WZ_LAZY if name.endswith("true>") else HF.K3_WGRAD_WZ
    return {"conv3d_k3_fwd_kernel": HF.K3_FWD_DIRECT, "conv3d_k3_fwd_wz_kernel": HF.K3_FWD_WZ,
            "conv3d_k3_fwd_wzy_kernel": HF.K3_FWD_WZY, "conv3d_k3_fwd_wzy16_kernel": HF.K3_FWD_WZY,
            "conv3d_k3_wgrad_kernel": HF.K3_WGRAD_DIRECT, "conv3d_k3_wgrad_vec_kernel": HF.K3_WGRAD_VEC,
            "conv3d_k3_wgrad_c1_kernel": HF.K3_WGRAD_C1, "conv3d_k3_fwd_c1_kernel": HF.K3_FWD_C1,
            "conv3d_k3_fwd_c1w_kernel": HF.K3_FWD_C1, "conv3d_k3_wgrad_wzy_kernel": HF.K3_WGRAD_WZY}[base]


def test_expected_names_and_families_without_a_device():
    """The names the GPU cases expect are what the library's choice gives for their facts, and _family maps every one of
    them to the kind the query itself returns."""
    from dram_amd import _lib
    from dram_amd import functional as HF

    def fwd(ci, co, dst=None, fused=0, src=(0, 0, 0, 0, 0, 0)):
        buf = ctypes.create_string_buffer(96)
        kind = _lib.lib.dram_conv3d_k3_fwd_choice_src(ci, co, *DHW, *(dst or (co, 0, 0, 0, 0)), fused, *src, buf, len(buf))
        assert kind == _family(buf.value.decode()), buf.value
        return buf.value.decode()

    def wgrad(c1, c2, lazy):
        buf = ctypes.create_string_buffer(96)
        kind = _lib.lib.dram_conv3d_k3_wgrad_choice(N, c1, c2, CO, *DHW, int(lazy), buf, len(buf))
        assert kind == _family(buf.value.decode()), buf.value
        return buf.value.decode()

    assert HF.crop_offsets(DHW, SKIP_DHW) == (1, 2, 3)
    assert fwd(16, CO) == "conv3d_k3_fwd_wzy_kernel"                                        # (a)
    assert fwd(16, CO, src=(8, *SKIP_DHW, 3, 0)) == WZ_SAME_BOXES                            # (b)
    assert fwd(16, CO, src=(0, 0, 0, 0, 0, 1)) == WZ_SAME_BOXES                              # (c)
    assert fwd(16, CO, fused=1) == "conv3d_k3_fwd_wzy_kernel"                                # (d)
    fwd(CO, 16), fwd(CO, 16, dst=(8, 8, *SKIP_DHW))                                          # the backward-data launches
    for c1, c2 in ((16, 0), (8, 8), (16, 16)):
        for lazy in (False, True):
            wgrad(c1, c2, lazy)
    assert not _lib.lib.dram_conv3d_k3_wgrad_lazy_ok(N, 8, 8, CO, *DHW)
    assert wgrad(8, 8, True) == wgrad(8, 8, False)
    assert _lib.lib.dram_conv3d_k3_wgrad_lazy_ok(N, 16, 16, CO, *DHW)
    assert _family(wgrad(16, 16, True)) == HF.K3_WGRAD_WZY


def _one_call(fn):
    """Run the helper call `fn() -> output tensors` once with a KernelTimer and once without; returns (key, family's launch
    count of the timed call, outputs of the timed call)."""
    from dram_amd import functional as HF
    saved, timer = HF.TIMER, HF.KernelTimer()
    before = HF.conv_launch_counts()
    HF.TIMER = timer
    try:
        timed = fn()
        mid = HF.conv_launch_counts()
        HF.TIMER = None
        plain = fn()
    finally:
        HF.TIMER = saved
    after = HF.conv_launch_counts()
    torch.cuda.synchronize()
    assert len(timer.records) == 1
    key = timer.records[0][0]
    moved = {k: mid[k] - before[k] for k in range(HF.K3_KINDS) if mid[k] != before[k]}
    assert list(moved) == [_family(key)], (key, moved)
    assert {k: after[k] - mid[k] for k in range(HF.K3_KINDS) if after[k] != mid[k]} == moved, key
    assert len(timed) == len(plain)
    for a, b in zip(timed, plain):
        assert torch.equal(a, b), key
    return key, moved[_family(key)], timed


@pytest.fixture(scope="module")
def data():
    """Inputs shared by the cases (never written to)."""
    g = torch.Generator().manual_seed(7)
    r = lambda *shape: torch.randn(*shape, generator=g).cuda()
    d = {"x16": r(N, 16, *DHW), "x8": r(N, 8, *DHW), "skip8": r(N, 8, *SKIP_DHW), "skip16": r(N, 16, *SKIP_DHW),
         "w": r(CO, 16, 3, 3, 3) / (16 * 27) ** 0.5, "w32": r(CO, 32, 3, 3, 3) / (32 * 27) ** 0.5, "dy": r(N, CO, *DHW),
         "coef8": torch.rand(N * 8 * 2, generator=g).cuda() + 0.3, "coef16": torch.rand(N * 16 * 2, generator=g).cuda() + 0.3}
    buf = torch.zeros(d["x16"].numel() + 4, device="cuda")
    d["x16_off"] = buf[1:1 + d["x16"].numel()].view(d["x16"].shape)
    d["x16_off"].copy_(d["x16"])
    return d


def _fwd(src, w, lazy=None, stats=False):
    from dram_amd import _lib
    from dram_amd import functional as HF

    def fn():
        y = torch.empty((N, CO) + DHW, device="cuda")
        nparts = _lib.lib.dram_conv3d_k3_stats_parts(w.shape[1], CO, *DHW) if stats else 0
        parts = torch.zeros(N * CO * nparts * 3, device="cuda") if stats else None
        HF.conv3d_k3_launch_fwd(src, HF._pack(w, 0), None, y, lazy, parts, nparts)
        return (y, parts) if stats else (y,)
    return fn


@pytest.mark.gpu
def test_plain_source_forward_and_backward(data):
    """(a): forward on the (z,y) kernel; its backward-data and backward-weights keys are the library's names for them."""
    from dram_amd import functional as HF
    x, w, dy = data["x16"], data["w"], data["dy"]
    assert x.data_ptr() % 16 == 0
    src = HF.CatView(x, None, DHW, channels=16)
    key, _, _ = _one_call(_fwd(src, w))
    assert key == "conv3d_k3_fwd_wzy_kernel"

    def bwd_data():
        dx = torch.empty_like(x)
        HF.conv3d_k3_launch_bwd_data(dy, HF._pack(w, 1), dx)
        return (dx,)
    key, _, _ = _one_call(bwd_data)
    assert key == HF.conv_fwd_kernel_name(DHW, 16, CO)
    key, _, (dw,) = _one_call(lambda: (HF.conv3d_k3_launch_wgrad(src, dy, w),))
    assert key == HF.conv_wgrad_kernel_name(N, DHW, CO, 16) and dw.shape == w.shape


@pytest.mark.gpu
def test_cropped_skip_source_and_split_destination(data):
    """(b): a crop window at x offset 3 sends the forward to the z-only kernel; backward-data writes dx1 and the window of dx2
    only."""
    from dram_amd import functional as HF
    x, skip, w, dy = data["x8"], data["skip8"], data["w"], data["dy"]
    src = HF.CatView(x, skip, DHW, channels=16)
    assert src.off == (1, 2, 3) and x.data_ptr() % 16 == 0 and skip.data_ptr() % 16 == 0
    key, _, _ = _one_call(_fwd(src, w))
    assert key == WZ_SAME_BOXES

    def bwd_data():
        dx1, dx2 = torch.empty_like(x), HF.conv3d_k3_dx2(skip, DHW)
        HF.conv3d_k3_launch_bwd_data(dy, HF._pack(w, 1), dx1, dx2)
        return dx1, dx2
    key, _, (dx1, dx2) = _one_call(bwd_data)
    assert key == HF.conv_fwd_kernel_name(DHW, 16, CO, dst_split=(8, 8) + SKIP_DHW)
    window = (slice(None), slice(None), slice(1, 1 + DHW[0]), slice(2, 2 + DHW[1]), slice(3, 3 + DHW[2]))
    assert float(dx1.abs().min()) > 0 and float(dx2[window].abs().min()) > 0
    rest = dx2.clone()
    rest[window] = 0
    assert float(rest.abs().max()) == 0.0


@pytest.mark.gpu
def test_misaligned_source(data):
    """(c): a contiguous view one float into its buffer is off 16-byte alignment: the z-only kernel, same result as (a)."""
    from dram_amd import functional as HF
    x, w = data["x16_off"], data["w"]
    assert x.is_contiguous() and x.data_ptr() % 16 == 4
    key, _, (y,) = _one_call(_fwd(HF.CatView(x, None, DHW, channels=16), w))
    assert key == WZ_SAME_BOXES
    y_a = _fwd(HF.CatView(data["x16"], None, DHW), w)()[0]
    torch.testing.assert_close(y, y_a, rtol=1e-4, atol=1e-4)       # (two Winograd forms of the same fp32 conv)


@pytest.mark.gpu
def test_fused_forward_and_lazy_backward_weights(data):
    """(d): the fused forward with a statistics buffer; backward-weights with coefficients on the skip source."""
    from dram_amd import _lib
    from dram_amd import functional as HF
    w, dy = data["w"], data["dy"]
    key, _, _ = _one_call(_fwd(HF.CatView(data["x16"], None, DHW, channels=16), w, lazy=(None, 0, None, 0), stats=True))
    assert key == "conv3d_k3_fwd_wzy_kernel"

    # (b)'s sources: no on-load path for an 8 + 8 concat, so the lazy skip is materialised (what the engine does)
    x, skip, coef = data["x8"], data["skip8"], data["coef8"]
    assert not _lib.lib.dram_conv3d_k3_wgrad_lazy_ok(N, 8, 8, CO, *DHW)
    act = torch.empty_like(skip)
    _lib.call("dram_row_affine_act", skip.data_ptr(), coef.data_ptr(), act.data_ptr(), 1, N * 8, skip[0, 0].numel(), HF._stream())
    key, _, _ = _one_call(lambda: (HF.conv3d_k3_launch_wgrad(HF.CatView(x, act, DHW, channels=16), dy, w),))
    assert key == HF.conv_wgrad_kernel_name(N, DHW, CO, 8, 8, lazy=True)

    # 16 + 16 channels: the lazy path proper, one lazy source of two -> one launch per source
    x, skip, coef, w32 = data["x16"], data["skip16"], data["coef16"], data["w32"]
    src = HF.CatView(x, skip, DHW, channels=32)
    key, launches, (dw,) = _one_call(lambda: (HF.conv3d_k3_launch_wgrad(src, dy, w32, (None, 0, coef, 1)),))
    assert key == HF.conv_wgrad_kernel_name(N, DHW, CO, 16, 16, lazy=True)
    assert _family(key) == HF.K3_WGRAD_WZY and launches == 2 and dw.shape == w32.shape
