"""Writes tests/golden/pool_geometry.npz: the reference's ConvPoolBlock5d with max-pool geometries other than 2 / 2 / 0, and
its DC3D as an anisotropic network (pooling and upsampling by (1, 2, 2)), run on the CPU.

Needs the reference checkout (see oracle/make_golden.py for where it is expected); nothing of it is copied: the fixture holds
state dicts, inputs, outputs and gradients.

  block/<i>/...   ConvPoolBlock5d([3, 4], [4, 6], 0, (3, 3), False, (1, 1), pk, ps, pp, dropout=0.0, norm_method="bn") for
                  BLOCK_CASES[i] = (pk, ps, pp) on an input [2, 3, 5, 8, 10], in the layout of oracle/make_golden.py:_block_case
                  (sd/, in0, out/{y,pooled}, gout/{y,pooled}, gin0, gparam/, sd_after/, eval/{y,pooled}); block/<i>/geometry
                  holds pk, ps, pp as a 3 x 3 array.
  aniso/...       DC3D(**SLIM, upsample_sf=(1, 2, 2)) whose three ds_modules[i].maxpool are nn.MaxPool3d((1, 2, 2)); seed 0,
                  HeNorm(fan_in), input [1, 1, 8, 16, 16] (seed 1), train mode.  x, train_out, gout, gin (the input's gradient),
                  grad/<k> for the parameter subset GRAD_KEYS (the one dc3d_slim.npz keeps for its "ln" / "in" cases),
                  sd_after/ (BatchNorm buffers after the step).  The state dict itself (1.0 MB of fp32 noise, above what a
                  committed file may hold next to the rest) is stored as sdsum/<k> = (sum, sum of squares) in fp64, like
                  dc3d_full.npz: a test re-creates the weights from the same seed and checks them against these.
                  grad64/<k>, gin64: the same gradients from a float64 run of the same model, rounded to fp32 for the file's
                  size (6e-8 relative) -- early-layer gradients of a BatchNorm U-Net carry ReLU-mask-flip noise in fp32
                  (tests/test_gpu_parity.py:check_grads), which is judged against fp64 with the reference's own fp32 error as
                  the yardstick.

    python scripts/make_golden_pool.py
"""
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import make_golden as MG  # noqa: E402

BLOCK_CASES = (((1, 2, 2), (1, 2, 2), 0), (3, 2, 1), ((2, 3, 2), (2, 1, 2), (1, 1, 0)))
GRAD_KEYS = ("top_layer.weight", "top_layer.bias", "ds_modules.0.conv_blocks.0.0.weight",
             "ds_modules.1.conv_blocks.1.0.weight", "bg.conv_blocks.0.1.weight", "bg.conv_blocks.0.1.bias",
             "us_modules.0.conv_blocks.0.0.weight", "us_modules.2.conv_blocks.1.0.weight")


def _t3(v):
    return tuple(v) if isinstance(v, tuple) else (v,) * 3


def gen_blocks(parts, arrs):
    g = torch.Generator().manual_seed(4711)
    for i, (pk, ps, pp) in enumerate(BLOCK_CASES):
        torch.manual_seed(31 + i)
        blk = parts.ConvPoolBlock5d([3, 4], [4, 6], 0, (3, 3), False, (1, 1), pk, ps, pp, dropout=0.0, norm_method="bn")
        for m in blk.modules():                      # non-trivial affine parameters
            if isinstance(m, torch.nn.BatchNorm3d):
                m.weight.data = torch.rand(m.weight.shape, generator=g) + 0.5
                m.bias.data = torch.randn(m.bias.shape, generator=g) * 0.3
        x = torch.randn(2, 3, 5, 8, 10, generator=g)
        MG._block_case(f"block/{i}", blk, [x], ["y", "pooled"], arrs, seed=40 + i)
        arrs[f"block/{i}/geometry"] = np.array([_t3(pk), _t3(ps), _t3(pp)], dtype=np.int64)
        print(f"block/{i}: pool {pk} / {ps} / {pp}: pooled {tuple(arrs[f'block/{i}/out/pooled'].shape)}")


def gen_aniso(models, arrs):
    tag = "aniso"
    torch.manual_seed(0)
    model = models.DC3D(**dict(MG.SLIM, upsample_sf=(1, 2, 2)))
    model.init(models.HeNorm(mode="fan_in"))
    for ds in model.ds_modules:
        ds.maxpool = torch.nn.MaxPool3d((1, 2, 2))
    for k, v in model.state_dict().items():
        vf = v.double()
        arrs[f"{tag}/sdsum/{k}"] = np.array([vf.sum().item(), (vf * vf).sum().item()])
    x = torch.rand((1, 1, 8, 16, 16), generator=torch.Generator().manual_seed(1))
    arrs[f"{tag}/x"] = MG._np(x)
    m64 = copy.deepcopy(model).double().train()
    model.train()
    xr = x.clone().requires_grad_(True)
    d0, d1 = model(xr, None)
    assert d0 is d1 and tuple(d0.shape) == tuple(x.shape)
    arrs[f"{tag}/train_out"] = MG._np(d0)
    gout = torch.randn(d0.shape, generator=torch.Generator().manual_seed(2)) / d0.numel()
    arrs[f"{tag}/gout"] = MG._np(gout)
    (d0 * gout).sum().backward()
    x64 = x.double().requires_grad_(True)
    e0, _ = m64(x64, None)
    (e0 * gout.double()).sum().backward()
    arrs[f"{tag}/gin"], arrs[f"{tag}/gin64"] = MG._np(xr.grad), MG._np(x64.grad.float())
    grads, grads64 = dict(model.named_parameters()), dict(m64.named_parameters())
    for k in GRAD_KEYS:
        arrs[f"{tag}/grad/{k}"], arrs[f"{tag}/grad64/{k}"] = MG._np(grads[k].grad), MG._np(grads64[k].grad.float())
        err = ((grads[k].grad.double() - grads64[k].grad).abs().max() / grads64[k].grad.abs().max()).item()
        print(f"aniso: reference fp32 vs fp64 gradient {k}: {err:.2e}")
    for k, v in model.state_dict().items():
        if "running" in k or "num_batches" in k:
            arrs[f"{tag}/sd_after/{k}"] = MG._np(v)


def main():
    torch.set_num_threads(8)
    parts, models = MG._import_reference()
    arrs = {}
    gen_blocks(parts, arrs)
    gen_aniso(models, arrs)
    MG._save("pool_geometry", **arrs)


if __name__ == "__main__":
    main()
