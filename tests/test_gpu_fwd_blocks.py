"""The forward / backward-data kernels of conv3d_k3.hip that take their item decode from csrc/fwd_device.h -- the direct 27-tap
kernel, the Winograd-z kernel and the two first-layer kernels -- run in-process on the smallest shapes that reach each arm of
the block scaffold they repeat (decode, filter tile, input chunk, split-destination store).  No environment switch: the direct kernel is reached through D = 1 or Cin < 8, the z-only kernel through Cout % 64 != 0.
Every launch is bracketed by the library's launch counters (K3_FWD_DIRECT / K3_FWD_WZ / K3_FWD_C1): exactly one moves, by one, so a
case proves which family produced what it checks; the instantiation of every case is asked of the library without a device in the
first test.

  D1   fwd 10 -> 40, (1, 8, 32), bias        three K chunks with a partial last one (`has_next` arm, zero rows of the filter tile);
                                             Cout tail inside a 64-channel tile; bias
  D2   fwd 3 ++ crop 4 -> 8, (4, 8, 16)      a K chunk that straddles the two sources; crop offsets (1, 2, 2)
  D3   bwd-data 4 -> 5 + window of 3         split destination; dx2 outside its window stays exactly 0
  D4   fused 8 ++ 8 -> 32, (1, 8, 20)        on-load transform incl. the zero padding of the activated tensor (second source without
                                             ReLU: a * 0 + b != 0); ragged x box; statistics partials
  W1   fwd 10 -> 40, (3, 8, 32), bias        partial chunk; odd D (half-empty last plane pair); Cout tail
  W2   fused 6 ++ 10 -> 32, (4, 10, 10)      100 of 128 lanes; chunk straddling the sources; statistics arm of the epilogue
  W3   bwd-data 16 -> 8 + window of 8        split destination on the z-only kernel
  W4   fused 8 -> 72, (2, 16, 8)             single chunk (no `has_next`); second channel tile holding 8 of 64 channels
  C1   fwd 1 -> 40, (5, 9, 35)               partial second channel tile (`cmask`); ragged boxes on every axis; 8 partials per box
  C1W  fwd 1 -> 40, (5, 6, 100)              the wide form's 16-byte stores with a partial tile; 16 partials per box

Outputs against torch.nn.functional.conv3d in fp64 over the activated and cropped sources, with `check` of test_gpu_parity.py
(max-abs over max |reference| and relative L2, both <= 1e-4: the bound the project uses for these kernels).  Statistics as
test_conv3d_k3_wzy_fused checks them: after Chan's combine of the partials in fp64 the counts equal D*H*W exactly, the mean of y
is within 1e-5 and M2 within 1e-4 relative.  Output and partial buffers start as NaN, so an unwritten voxel or slot fails.
"""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_parity import check, rel_err

N = 2
DIRECT, WZ, C1 = "conv3d_k3_fwd_kernel", "conv3d_k3_fwd_wz_kernel", "conv3d_k3_fwd_c1_kernel"

# name: (kernel, C1, C2, shape of the second tensor beyond (D, H, W), Cout, (D, H, W), mode); mode "bwd": the launch is the
# backward-data of a conv C1 + C2 -> Cout, i.e. a forward Cout -> C1 + C2 whose DESTINATION is split
CASES = {
    "D1": (DIRECT + "<32, 4, 2, 2, false>", 10, 0, None, 40, (1, 8, 32), "bias"),
    "D2": (DIRECT + "<16, 4, 4, 1, false>", 3, 4, (2, 3, 3), 8, (4, 8, 16), "plain"),
    "D3": (DIRECT + "<8, 8, 4, 1, false>", 5, 3, (2, 3, 3), 4, (4, 8, 8), "bwd"),
    "D4": (DIRECT + "<32, 4, 2, 1, true>", 8, 8, (2, 3, 4), 32, (1, 8, 20), "fused+stats"),
    "W1": (WZ + "<32, 4, 2, false>", 10, 0, None, 40, (3, 8, 32), "bias"),
    "W2": (WZ + "<10, 10, 1, true>", 6, 10, (2, 3, 3), 32, (4, 10, 10), "fused+stats"),
    "W3": (WZ + "<16, 8, 1, false>", 8, 8, (2, 3, 3), 16, (4, 16, 16), "bwd"),
    "W4": (WZ + "<8, 16, 2, true>", 8, 0, None, 72, (2, 16, 8), "fused"),
    "C1": (C1, 1, 0, None, 40, (5, 9, 35), "c1"),
    "C1W": ("conv3d_k3_fwd_c1w_kernel", 1, 0, None, 40, (5, 6, 100), "c1"),
}
CROP = (1, 2, 2)        # ceil of half of every `beyond` above, written out: independent of the library


def _family(kernel):
    from dram_amd import functional as HF
    return {DIRECT: HF.K3_FWD_DIRECT, WZ: HF.K3_FWD_WZ, C1: HF.K3_FWD_C1, "conv3d_k3_fwd_c1w_kernel": HF.K3_FWD_C1}[kernel.split("<")[0]]


def _rand(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _inputs(name):
    """CPU tensors of a case: x1, x2 (or None; for "bwd": the shapes of dx1, dx2), w[Cout][C1 + C2][3][3][3]."""
    _, c1, c2, beyond, co, dhw, _ = CASES[name]
    seed = 100 * (list(CASES).index(name) + 1)
    x1 = _rand(seed + 1, N, c1, *dhw)
    x2 = _rand(seed + 2, N, c2, *(a + b for a, b in zip(dhw, beyond))) if c2 else None
    w = _rand(seed + 3, co, c1 + c2, 3, 3, 3) / ((c1 + c2) * 27) ** 0.5
    return x1, x2, w


def test_kernel_of_every_case_without_a_device():
    """The library's own choice (dram_conv3d_k3_fwd_choice_src, the fwd_choice a launch goes through) names the intended
    instantiation and family for every case."""
    from dram_amd import functional as HF
    for name, (kernel, c1, c2, beyond, co, dhw, mode) in CASES.items():
        x1, x2, _ = _inputs(name)
        if mode == "bwd":       # Cout -> C1 + C2 from a plain dy into the split destination
            got = HF.conv_fwd_kernel_name(dhw, c1 + c2, co, dst_split=(c1, c2, *x2.shape[2:]), src=(x1, None, 0))
        else:
            assert x2 is None or HF.crop_offsets(dhw, tuple(x2.shape[2:])) == CROP, name
            got = HF.conv_fwd_kernel_name(dhw, co, c1 + c2, fused=mode.startswith("fused"), src=(x1, x2, CROP[2] if c2 else 0))
        assert got == kernel, name
        if mode == "c1":        # ... and with statistics (the fused entry point, no operand transform)
            assert HF.conv_fwd_kernel_name(dhw, co, 1, fused=True, src=(x1, None, 0)) == kernel, name


def _counted(name, launch):
    """Run `launch` and assert that exactly one launch of the case's family happened."""
    from dram_amd import functional as HF
    before = HF.conv_launch_counts()
    launch()
    torch.cuda.synchronize()
    after = HF.conv_launch_counts()
    moved = {k: after[k] - before[k] for k in range(HF.K3_KINDS) if after[k] != before[k]}
    assert moved == {_family(CASES[name][0]): 1}, (name, moved)


def _act(t, cf, relu):
    """fp64 operand of a lazily normalised source: act(a * t + b) per (sample, channel) row, cf = [row][a, b]."""
    if cf is None:
        return t.double()
    c = cf.view(t.shape[0], t.shape[1], 2).double()
    v = t.double() * c[:, :, 0, None, None, None] + c[:, :, 1, None, None, None]
    return torch.relu(v) if relu else v


def _window(x2, dhw):
    return x2[:, :, CROP[0]:CROP[0] + dhw[0], CROP[1]:CROP[1] + dhw[1], CROP[2]:CROP[2] + dhw[2]]


def _report(got, ref, what):
    mx, l2 = rel_err(got, ref)
    print(f"{what}: max-rel {mx:.3e}, rel-L2 {l2:.3e}")
    check(got, ref, what)


def _check_stats(parts, nparts, y, dhw, what):
    """Chan's combine of the {mean, M2, count} partials in fp64 against the moments of the y the launch wrote."""
    rows = y.shape[0] * y.shape[1]
    q = parts.view(rows, nparts, 3).double().cpu()
    assert bool(torch.isfinite(q).all()), what
    cnt = q[:, :, 2].sum(1)
    mean = (q[:, :, 0] * q[:, :, 2]).sum(1) / cnt
    m2 = (q[:, :, 1] + q[:, :, 2] * (q[:, :, 0] - mean[:, None]) ** 2).sum(1)
    r = y.double().cpu().view(rows, -1)
    dmean = (mean - r.mean(1)).abs().max().item()
    dm2 = ((m2 - ((r - r.mean(1, keepdim=True)) ** 2).sum(1)).abs() / m2).max().item()
    print(f"{what}: statistics mean diff {dmean:.3e}, M2 rel diff {dm2:.3e}")
    assert bool((cnt == dhw[0] * dhw[1] * dhw[2]).all()), what
    assert dmean < 1e-5, what
    assert dm2 < 1e-4, what


def _forward(name, x1, x2, w, bias=None, lazy=None, stats=False):
    """y (NaN-initialised) and the statistics partials of one counted forward launch."""
    from dram_amd import functional as HF
    from dram_amd import _lib
    _, c1, c2, _, co, dhw, _ = CASES[name]
    src = HF.CatView(x1.cuda(), None if x2 is None else x2.cuda(), dhw, channels=c1 + c2)
    assert src.off == (CROP if c2 else (0, 0, 0))
    wt = HF._pack(w.cuda(), 0)
    y = torch.full((N, co, *dhw), float("nan"), device="cuda")
    nparts = _lib.lib.dram_conv3d_k3_stats_parts(c1 + c2, co, *dhw) if stats else 0
    parts = torch.full((N * co * nparts * 3,), float("nan"), device="cuda") if stats else None
    b = None if bias is None else bias.cuda()
    torch.cuda.synchronize()
    _counted(name, lambda: HF.conv3d_k3_launch_fwd(src, wt, b, y, lazy=lazy, parts=parts, nparts=nparts))
    return y, parts, nparts


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["D1", "W1", "D2"])
def test_plain_forward(name):
    _, c1, c2, _, co, dhw, mode = CASES[name]
    x1, x2, w = _inputs(name)
    bias = _rand(7, co) if mode == "bias" else None
    xin = x1.double() if x2 is None else torch.cat([x1.double(), _window(x2, dhw).double()], 1)
    ref = F.conv3d(xin, w.double(), None if bias is None else bias.double(), padding=1)
    y, _, _ = _forward(name, x1, x2, w, bias=bias)
    _report(y, ref, f"{name} {CASES[name][0]}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["D4", "W2", "W4"])
def test_fused_forward(name):
    """Lazy sources: the first with ReLU, the second (a * x + b only) without, so that its zero padding differs from act(0)."""
    _, c1, c2, _, co, dhw, mode = CASES[name]
    x1, x2, w = _inputs(name)
    g = torch.Generator().manual_seed(9)
    coef1 = torch.rand(N * c1 * 2, generator=g) + 0.5
    coef2 = torch.rand(N * c2 * 2, generator=g) - 0.2 if c2 else None
    xin = _act(x1, coef1, True)
    if c2:
        xin = torch.cat([xin, _act(_window(x2, dhw), coef2, False)], 1)
    ref = F.conv3d(xin, w.double(), None, padding=1)
    stats = mode.endswith("stats")
    y, parts, nparts = _forward(name, x1, x2, w, lazy=(coef1.cuda(), 1, None if coef2 is None else coef2.cuda(), 0), stats=stats)
    _report(y, ref, f"{name} {CASES[name][0]}")
    if stats:
        _check_stats(parts, nparts, y, dhw, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["D3", "W3"])
def test_backward_data_into_a_split_destination(name):
    """dx of y = conv3d(x1 ++ crop(x2), w) from dy: channels [0, C1) into dx1, the rest into the crop window of dx2, which holds NaN
    inside the window and 0 outside before the launch."""
    from dram_amd import functional as HF
    _, c1, c2, _, co, dhw, _ = CASES[name]
    x1, x2, w = _inputs(name)
    dy = _rand(8, N, co, *dhw)
    ref = F.conv_transpose3d(dy.double(), w.double(), None, padding=1)
    dx1 = torch.full(tuple(x1.shape), float("nan"), device="cuda")
    dx2 = torch.zeros(tuple(x2.shape), device="cuda")
    _window(dx2, dhw).fill_(float("nan"))
    wt = HF._pack(w.cuda(), 1)
    dyd = dy.cuda()
    torch.cuda.synchronize()
    _counted(name, lambda: HF.conv3d_k3_launch_bwd_data(dyd, wt, dx1, dx2))
    _report(dx1, ref[:, :c1], f"{name} {CASES[name][0]} dx1")
    _report(_window(dx2, dhw), ref[:, c1:], f"{name} dx2 window")
    outside = dx2.cpu().clone()
    _window(outside, dhw).zero_()
    assert bool((outside == 0).all()), name


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["C1", "C1W"])
def test_first_layer(name):
    """Once with bias, once through the fused entry point with statistics (plain source)."""
    _, _, _, _, co, dhw, _ = CASES[name]
    x1, _, w = _inputs(name)
    bias = _rand(7, co)
    ref = F.conv3d(x1.double(), w.double(), None, padding=1)
    y, _, _ = _forward(name, x1, None, w, bias=bias)
    _report(y, ref + bias.double()[None, :, None, None, None], f"{name} bias")
    y, parts, nparts = _forward(name, x1, None, w, lazy=(None, 0, None, 0), stats=True)
    boxes = {"C1": (32, 8, 4, 8), "C1W": (128, 4, 4, 16)}[name]
    assert nparts == -(-dhw[2] // boxes[0]) * -(-dhw[1] // boxes[1]) * -(-dhw[0] // boxes[2]) * boxes[3], name
    _report(y, ref, f"{name} statistics launch")
    _check_stats(parts, nparts, y, dhw, name)
