"""General 3-D convolution (HipConv3d kind "gen", csrc/conv3d_gen.hip) against torch.nn.functional.conv3d + autograd
in float64 on CPU: forward, dX, dW and dbias for kernels 1..7, paddings 0..k-1 and strides 1 / 2 per axis, odd
spatial sizes and channel counts; which kernels the standard and general convs reach; the limits; and DC3D networks
built with the reference's kernel_sizes / padding_list knobs against the oracle."""
import pytest
import torch
import torch.nn.functional as F

import models
from dram_amd import engine
from dram_amd import functional as HF
from dram_amd.modules import HipConv3d
from oracle import dram_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (kernel, stride, padding)
GEOMS = [
    ((5, 5, 5), (1, 1, 1), (2, 2, 2)),
    ((7, 7, 7), (1, 1, 1), (3, 3, 3)),
    ((1, 3, 3), (1, 1, 1), (0, 1, 1)),
    ((3, 1, 1), (1, 1, 1), (1, 0, 0)),
    ((2, 2, 2), (2, 2, 2), (0, 0, 0)),
    ((3, 3, 3), (1, 1, 1), (0, 0, 0)),
    ((3, 3, 3), (2, 2, 2), (1, 1, 1)),
    ((3, 3, 3), (1, 2, 2), (1, 1, 1)),
    ((1, 1, 1), (1, 1, 1), (1, 1, 1)),
    ((1, 1, 1), (2, 2, 2), (0, 0, 0)),      # backward-data phases that no tap reaches
    ((7, 5, 3), (2, 1, 2), (6, 0, 2)),
    ((4, 2, 6), (2, 2, 1), (3, 1, 5)),
]
# (Cin, Cout, bias, spatial)
CHANNELS = [
    (1, 17, True, (13, 18, 21)),
    (3, 64, False, (13, 18, 21)),
    (64, 1, True, (13, 18, 21)),
    (64, 64, True, (9, 10, 11)),
]


def _ids(v):
    k, s, p = v
    return "k{}{}{}_s{}{}{}_p{}{}{}".format(*k, *s, *p)


def _run_case(k, s, p, ci, co, bias, size, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, ci, *size, generator=g, dtype=torch.float64)
    w = torch.randn(co, ci, *k, generator=g, dtype=torch.float64) / (ci * k[0] * k[1] * k[2]) ** 0.5
    b = torch.randn(co, generator=g, dtype=torch.float64) if bias else None
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True) if bias else None
    yr = F.conv3d(xr, wr, br, stride=s, padding=p)
    gy = torch.randn(yr.shape, generator=g, dtype=torch.float64)
    (yr * gy).sum().backward()

    xd = x.float().to(DEV).requires_grad_(True)
    wd = w.float().to(DEV).requires_grad_(True)
    bd = b.float().to(DEV).requires_grad_(True) if bias else None
    yd = HF.conv3d_gen(xd, wd, bd, s, p)
    yd.backward(gy.float().to(DEV))
    torch.cuda.synchronize()
    pairs = [("y", yd, yr), ("dx", xd.grad, xr.grad), ("dw", wd.grad, wr.grad)]
    if bias:
        pairs.append(("db", bd.grad, br.grad))
    for name, got, ref in pairs:
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        err = (got.detach().double().cpu() - ref.detach()).abs().max().item()
        scale = ref.detach().abs().max().item()
        assert err <= 1e-5 * scale, f"{name}: max abs err {err:.3e} > 1e-5 * {scale:.3e}"


@pytest.mark.parametrize("geom", GEOMS, ids=_ids)
@pytest.mark.parametrize("chans", CHANNELS, ids=lambda c: f"{c[0]}to{c[1]}{'_bias' if c[2] else ''}")
def test_conv_gen_matches_torch(geom, chans):
    k, s, p = geom
    ci, co, bias, size = chans
    _run_case(k, s, p, ci, co, bias, size)


def test_conv_gen_batch_one_tiny_volume():
    # output of a single voxel per axis; channel counts off every tile size
    _run_case((3, 3, 3), (2, 2, 2), (0, 0, 0), 5, 33, True, (3, 4, 3))


def _counts():
    return HF.conv_gen_launch_counts()


def test_standard_convs_do_not_reach_the_general_kernels():
    torch.manual_seed(0)
    x = torch.randn(2, 8, 9, 10, 11, device=DEV, requires_grad=True)
    for k, p, bias in (((3, 3, 3), (1, 1, 1), False), ((3, 3, 3), (1, 1, 1), True), ((1, 1, 1), (0, 0, 0), True)):
        conv = HipConv3d(8, 16, kernel_size=k, padding=p, bias=bias).to(DEV)
        before = _counts()
        y = conv(x)
        y.sum().backward()
        torch.cuda.synchronize()
        assert _counts() == before, k
        with torch.no_grad():
            direct = HF.conv3d_k3(x, conv.weight, conv.bias) if k == (3, 3, 3) else HF.conv3d_k1(x, conv.weight, conv.bias)
            assert torch.equal(conv(x), direct)


@pytest.mark.parametrize("geom", GEOMS, ids=_ids)
def test_general_convs_reach_the_general_kernels(geom):
    k, s, p = geom
    conv = HipConv3d(3, 5, kernel_size=k, stride=s, padding=p, bias=True).to(DEV)
    x = torch.randn(1, 3, 9, 8, 7, device=DEV, requires_grad=True)
    before = _counts()
    conv(x).sum().backward()
    torch.cuda.synchronize()
    after = _counts()
    assert after[HF.GEN_FWD] == before[HF.GEN_FWD] + 1
    assert after[HF.GEN_BWD_DATA] > before[HF.GEN_BWD_DATA]
    assert after[HF.GEN_WGRAD] == before[HF.GEN_WGRAD] + 1


@pytest.mark.parametrize("kw", [dict(kernel_size=3, padding=1, dilation=2), dict(kernel_size=3, padding=1, groups=2),
                                dict(kernel_size=3, padding=1, stride=3), dict(kernel_size=9, padding=4),
                                dict(kernel_size=3, padding=3), dict(kernel_size=3, padding=1, padding_mode="reflect")])
def test_unsupported_geometry_raises(kw):
    conv = HipConv3d(4, 4, **kw).to(DEV)
    with pytest.raises(NotImplementedError, match="supported"):
        conv(torch.randn(1, 4, 12, 12, 12, device=DEV))


def test_output_below_one_is_a_value_error():
    conv = HipConv3d(2, 2, kernel_size=5, padding=0).to(DEV)
    with pytest.raises(ValueError, match="output size"):
        conv(torch.randn(1, 2, 4, 8, 8, device=DEV))


# ------------------------------------------------------------------------------------------------ model level
_SLIM_CHANS = dict(n_layers=3, in_ch_list=[1, 4, 8, 8, 16, 16, 8], base_ch_list=[4, 4, 8, 8, 8, 8, 4],
                   end_ch_list=[4, 8, 8, 8, 8, 4, 4], stacking=3, checkpoint_layers=[0, 1, 0, 1, 0, 1, 0], dropout=0.0,
                   upsample_ksize=(3, 3, 3), upsample_sf=(2, 2, 2), out_ch=1)
MODEL_CASES = {
    "valid": (dict(_SLIM_CHANS, kernel_sizes=[(3, 3)] * 7, padding_list=[(0, 0)] * 7), (92, 92, 92)),
    "k5k3": (dict(_SLIM_CHANS, kernel_sizes=[(5, 3)] * 7, padding_list=[(2, 1)] * 7), (24, 24, 24)),
    "k133": (dict(_SLIM_CHANS, kernel_sizes=[((1, 3, 3), (1, 3, 3))] * 7,
                  padding_list=[((0, 1, 1), (0, 1, 1))] * 7), (16, 24, 24)),
}


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("name", list(MODEL_CASES))
def test_dc3d_geometry_matches_oracle(name, training):
    cfg, size = MODEL_CASES[name]
    torch.manual_seed(1)
    model = models.DC3D(**cfg)
    assert not engine.supports(model)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 1, *size, generator=g)
    gout = torch.randn(2, 1, *size, generator=g)

    params, buffers = O.split_state_dict(sd)
    params = {k: v.double().requires_grad_(True) for k, v in params.items()}
    buffers = {k: (v.double() if v.is_floating_point() else v) for k, v in buffers.items()}
    with torch.set_grad_enabled(True):
        ref = O.dc3d_forward(cfg, params, buffers, x.double(), training=training, norm_method="bn")
        (ref * gout.double()).sum().backward()

    model = model.to(DEV).train(training)
    out, _ = model(x.to(DEV))
    (out * gout.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert out.shape == ref.shape
    assert _rel(out, ref) < 1e-4, "output"
    for k, p in model.named_parameters():
        assert _rel(p.grad, params[k].grad) < 1e-4, k
    for k, b in model.named_buffers():
        if b.is_floating_point():
            assert _rel(b, buffers[k]) < 1e-4, k
        else:
            assert int(b) == int(buffers[k]), k
