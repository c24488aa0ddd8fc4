"""GPU tests of the general max-pool (dram_maxpool3d_fwd / _bwd, functional.max_pool3d, HipMaxPool3d with any supported
geometry): bit for bit against torch's own CPU max_pool3d, the refusals of the C entry points, the reference's
ConvPoolBlock5d with other pools and its DC3D as an anisotropic network (tests/golden/pool_geometry.npz,
scripts/make_golden_pool.py).

Why equality is a fair demand: the inputs are integer-valued (randint(-3, 4): ties in nearly every window, so the first-maximum
rule decides where the gradient goes) and so are the upstream gradients (randint(-8, 9)): the sums over overlapping windows --
at most 27 terms of magnitude <= 8 -- are exact in fp32 in any order."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dram_amd.configs import SLIM
from test_gpu_misc import check as check_block, _sub
from test_gpu_parity import check as check_model, check_grads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# kernel, stride, padding, input shape
CASES = [
    ((1, 2, 2), (1, 2, 2), 0, (2, 3, 5, 9, 70)),          # anisotropic, odd extents, rows wider than a wavefront
    (3, 2, 1, (2, 2, 7, 9, 11)),                          # overlapping windows that hang over every border
    (3, 2, 1, (1, 2, 6, 10, 67)),
    (3, 1, 1, (1, 2, 5, 6, 66)),                          # every input in up to 27 windows
    (2, 3, 0, (2, 2, 8, 9, 10)),                          # gaps: inputs that no window covers
    ((2, 3, 4), (2, 1, 3), (1, 1, 2), (1, 3, 6, 7, 13)),  # all axes different
    (5, 4, 2, (1, 1, 9, 9, 9)),                           # largest window, idx up to 124
    (2, 2, 1, (1, 2, 5, 5, 5)),                           # the 2x2x2 window with padding: not the dedicated kernel's
    (3, 2, 1, (100, 3, 3, 4, 5)),                         # 300 planes on grid.y
]


def _ints(shape, seed, lo, hi):
    return torch.randint(lo, hi, shape, generator=torch.Generator().manual_seed(seed)).float()


def _same(got, ref, what):
    got, ref = got.detach().cpu().numpy(), ref.detach().numpy()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(got, ref, equal_nan=True), (what, int((~((got == ref) | ((got != got) & (ref != ref)))).sum()))


def _against_torch(x, k, s, p, what):
    """Forward and backward of functional.max_pool3d against torch's CPU max_pool3d on the same values."""
    from dram_amd import functional as HF
    xr = x.clone().requires_grad_(True)
    yr = F.max_pool3d(xr, k, s, p)
    gy = _ints(tuple(yr.shape), 7, -8, 9)
    yr.backward(gy)
    xg = x.to(DEV).requires_grad_(True)
    y = HF.max_pool3d(xg, k, s, p)
    assert type(y.grad_fn).__name__ == "MaxPoolFnBackward"
    y.backward(gy.to(DEV))
    _same(y, yr, f"{what}: output")
    _same(xg.grad, xr.grad, f"{what}: input gradient")
    return y


@pytest.mark.parametrize("k, s, p, shape", CASES)
def test_equals_torch(k, s, p, shape):
    _against_torch(_ints(shape, 3, -3, 4), k, s, p, f"pool {k} / {s} / {p} on {shape}")


@pytest.mark.parametrize("k, s, p, shape", CASES[:6])
def test_equals_torch_with_nans(k, s, p, shape):
    """A NaN in the window propagates, and the last NaN in scan order takes the gradient, as in ATen."""
    x = _ints(shape, 4, -3, 4)
    x[torch.rand(shape, generator=torch.Generator().manual_seed(5)) < 0.05] = float("nan")
    y = _against_torch(x, k, s, p, f"pool {k} / {s} / {p} on {shape} with NaNs")
    assert bool(torch.isnan(y).any()) and not bool(torch.isnan(y).all())


def test_equals_torch_on_real_values():
    """randn inputs: no ties; the integer-valued upstream gradient keeps the backward sums exact."""
    x = torch.randn((2, 2, 7, 9, 11), generator=torch.Generator().manual_seed(6))
    _against_torch(x, 3, 2, 1, "pool 3 / 2 / 1 on randn")


def test_gaps_are_zero_whatever_dx_held():
    """Stride above the kernel: the elements that no window covers come back as +0, not as what the allocation held."""
    from dram_amd import _lib
    N, C, D, H, W = 2, 2, 8, 9, 10
    geom = (N, C, D, H, W, 2, 2, 2, 3, 3, 3, 0, 0, 0)
    st = torch.cuda.current_stream().cuda_stream
    x = _ints((N, C, D, H, W), 8, -3, 4)
    xr = x.clone().requires_grad_(True)
    yr = F.max_pool3d(xr, 2, 3, 0)
    gy = _ints(tuple(yr.shape), 9, -8, 9)
    yr.backward(gy)
    xd, gd = x.to(DEV), gy.to(DEV)
    out = torch.full(yr.shape, float("nan"), device=DEV)
    idx = torch.full(yr.shape, 255, dtype=torch.uint8, device=DEV)
    dx = torch.full(x.shape, float("nan"), device=DEV)
    _lib.call("dram_maxpool3d_fwd", xd.data_ptr(), out.data_ptr(), idx.data_ptr(), *geom, st)
    _lib.call("dram_maxpool3d_bwd", gd.data_ptr(), idx.data_ptr(), dx.data_ptr(), *geom, st)
    _same(out, yr, "output")
    assert int(idx.max()) <= 7
    _same(dx, xr.grad, "input gradient over a NaN-filled dx")
    covered = torch.zeros(D, H, W, dtype=torch.bool)
    for z in range(0, D - 1, 3):
        for y in range(0, H - 1, 3):
            for xx in range(0, W - 1, 3):
                covered[z:z + 2, y:y + 2, xx:xx + 2] = True
    gaps = dx.cpu()[:, :, ~covered]
    assert gaps.numel() > 0 and bool((gaps == 0).all()) and not bool(torch.signbit(gaps).any())


def test_2x2x2_still_runs_the_dedicated_kernels():
    """HipMaxPool3d(2, 2, 0) -- more than one block of outputs -- is MaxPool2Fn, and the general kernels give the same."""
    from dram_amd import functional as HF
    from dram_amd.modules import HipMaxPool3d
    x = _ints((1, 1, 20, 20, 70), 10, -3, 4)
    xg = x.to(DEV).requires_grad_(True)
    y = HipMaxPool3d(2, 2, 0)(xg)
    assert type(y.grad_fn).__name__ == "MaxPool2FnBackward"
    assert torch.equal(y, HF.max_pool3d_2(x.to(DEV)))
    gy = _ints(tuple(y.shape), 11, -8, 9)
    y.backward(gy.to(DEV))
    xr = x.clone().requires_grad_(True)
    yr = F.max_pool3d(xr, 2, 2, 0)
    yr.backward(gy)
    _same(y, yr, "dedicated 2x2x2: output")
    _same(xg.grad, xr.grad, "dedicated 2x2x2: input gradient")
    _against_torch(x, 2, 2, 0, "general kernels on 2 / 2 / 0")
    z = HipMaxPool3d((1, 2, 2))(x.to(DEV).requires_grad_(True))
    assert type(z.grad_fn).__name__ == "MaxPoolFnBackward"
    _same(z, F.max_pool3d(x, (1, 2, 2)), "module with (1, 2, 2)")


@pytest.mark.parametrize("over", [dict(kw=6), dict(sh=0), dict(pd=2), dict(D=2, kd=5, pd=0)])
def test_refusals_touch_nothing(over):
    """Kernel 6, stride 0, padding above kernel/2, output extent 0: DRAM_EINVAL, and no buffer is written."""
    from dram_amd import _lib
    geom = dict(dict(N=1, C=2, D=8, H=8, W=8, kd=3, kh=3, kw=3, sd=2, sh=2, sw=2, pd=1, ph=1, pw=1), **over)
    st = torch.cuda.current_stream().cuda_stream
    n = 2 * 10 * 10 * 10                                  # more than any of these shapes could address
    x = torch.zeros(n, device=DEV)
    out, dx = torch.full((n,), 7.0, device=DEV), torch.full((n,), 7.0, device=DEV)
    idx = torch.full((n,), 201, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.DramHipError, match=r"failed \(-1\)"):
        _lib.call("dram_maxpool3d_fwd", x.data_ptr(), out.data_ptr(), idx.data_ptr(), *geom.values(), st)
    with pytest.raises(_lib.DramHipError, match=r"failed \(-1\)"):
        _lib.call("dram_maxpool3d_bwd", x.data_ptr(), idx.data_ptr(), dx.data_ptr(), *geom.values(), st)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((dx == 7.0).all()) and bool((idx == 201).all())


def test_functional_checks_its_input():
    from dram_amd import functional as HF
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HF.max_pool3d(torch.zeros(1, 1, 8, 8, 8), 3, 2, 1)
    with pytest.raises(ValueError, match="output size"):
        HF.max_pool3d(torch.zeros(1, 1, 2, 8, 8, device=DEV), 5, 1, 0)
    x = _ints((2, 3, 6, 7, 9), 12, -3, 4)
    xt = x.to(DEV).transpose(3, 4)                        # non-contiguous: made contiguous, like every other op
    _same(HF.max_pool3d(xt, 3, 2, 1), F.max_pool3d(x.transpose(3, 4), 3, 2, 1), "non-contiguous input")


@pytest.mark.parametrize("i, geom", enumerate([((1, 2, 2), (1, 2, 2), 0), (3, 2, 1), ((2, 3, 2), (2, 1, 2), (1, 1, 0))]))
def test_convpool_block_golden(golden_dir, i, geom):
    """The reference's ConvPoolBlock5d with these pools: same helper and tolerance as tests/test_gpu_misc.py's convpool_prelu."""
    import parts
    z = np.load(os.path.join(golden_dir, "pool_geometry.npz"))
    tag = f"block/{i}/"
    blk = parts.ConvPoolBlock5d([3, 4], [4, 6], 0, (3, 3), False, (1, 1), *geom, dropout=0.0, norm_method="bn")
    blk.load_state_dict({k: torch.from_numpy(v) for k, v in _sub(z, tag + "sd/").items()})
    blk = blk.cuda()
    x = torch.from_numpy(z[tag + "in0"]).cuda().requires_grad_(True)
    y, pooled = blk(x)
    assert type(pooled.grad_fn).__name__ == "MaxPoolFnBackward"
    check_block(y, z[tag + "out/y"], "y")
    check_block(pooled, z[tag + "out/pooled"], "pooled")
    t = lambda k: torch.from_numpy(z[tag + k]).cuda()
    ((y * t("gout/y")).sum() + (pooled * t("gout/pooled")).sum()).backward()
    check_block(x.grad, z[tag + "gin0"], "gin")
    for k, p in blk.named_parameters():
        check_block(p.grad, z[tag + "gparam/" + k], "gparam/" + k)


def test_anisotropic_network_golden(golden_dir):
    """DC3D(**SLIM, upsample_sf=(1, 2, 2)) with the three pools swapped for (1, 2, 2): takes the per-op path and reproduces the
    reference's dense output (1e-4, as tests/test_gpu_parity.py holds dc3d_slim.npz's) and gradients (check_grads of that
    file: every error against fp64 within 3x the reference's own fp32 noise, floor 5e-4; the fp64 values are the fixture's).
    The weights are seed 0's HeNorm(fan_in) ones -- 1.0 MB, which the fixture holds as checksums like dc3d_full.npz does --
    re-created here and checked against those."""
    import models
    from dram_amd.modules import HipMaxPool3d
    z = np.load(os.path.join(golden_dir, "pool_geometry.npz"))
    tag = "aniso/"
    torch.manual_seed(0)
    model = models.DC3D(**dict(SLIM, upsample_sf=(1, 2, 2)))
    model.init(models.HeNorm(mode="fan_in"))
    for ds in model.ds_modules:
        ds.maxpool = HipMaxPool3d((1, 2, 2))
    sums = _sub(z, tag + "sdsum/")
    assert set(sums) == set(model.state_dict())
    for k, v in model.state_dict().items():
        vf = v.double()
        assert np.allclose([vf.sum().item(), (vf * vf).sum().item()], sums[k], rtol=1e-12, atol=1e-12), k
    model = model.to(DEV).train()
    x = torch.from_numpy(z[tag + "x"]).to(DEV).requires_grad_(True)
    d0, d1 = model(x, None)
    assert d0 is d1 and "DC3DFusedFn" not in type(d0.grad_fn).__name__
    check_model(d0, z[tag + "train_out"], "anisotropic train output")
    (d0 * torch.from_numpy(z[tag + "gout"]).to(DEV)).sum().backward()
    params = dict(model.named_parameters())
    ref32 = dict(_sub(z, tag + "grad/"), input=z[tag + "gin"])
    true64 = {k: torch.from_numpy(v).double() for k, v in dict(_sub(z, tag + "grad64/"), input=z[tag + "gin64"]).items()}
    hip = {k: (x.grad if k == "input" else params[k].grad) for k in ref32}
    noise = check_grads(hip, ref32, true64, "anisotropic network")
    print(f"\nanisotropic network: reference fp32-vs-fp64 gradient noise {noise:.2e}")
    for k, v in _sub(z, tag + "sd_after/").items():
        check_model(model.state_dict()[k].double(), v.astype(np.float64), f"anisotropic buffer {k}")
