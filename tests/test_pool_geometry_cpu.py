"""CPU checks of the general max-pool's host side: the output-size rule against torch's own max_pool3d, what HipMaxPool3d
refuses, argument errors of the C entry points (reported without a GPU), which networks the fused engine takes, and the layout
of tests/golden/pool_geometry.npz (scripts/make_golden_pool.py)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import models
from dram_amd import _lib, engine
from dram_amd import functional as HF
from dram_amd.configs import SLIM
from dram_amd.modules import HipMaxPool3d

GRAD_KEYS = ("top_layer.weight", "top_layer.bias", "ds_modules.0.conv_blocks.0.0.weight",
             "ds_modules.1.conv_blocks.1.0.weight", "bg.conv_blocks.0.1.weight", "bg.conv_blocks.0.1.bias",
             "us_modules.0.conv_blocks.0.0.weight", "us_modules.2.conv_blocks.1.0.weight")


def test_output_size_is_torchs():
    """Kernel 1..5 x stride 1..5 x padding 0..k/2 on one axis (the other two take kernel 1 / stride 1 / padding 0) x extents
    1..11, the axis moved through all three places: what torch's CPU max_pool3d accepts is accepted with the same size, what it
    rejects raises."""
    accepted = rejected = 0
    for k in range(1, 6):
        for s in range(1, 6):
            for p in range(0, k // 2 + 1):
                for n in range(1, 12):
                    axis = (k + s + p + n) % 3
                    size, kk, ss, pp = [3, 2, 4], [1, 1, 1], [1, 1, 1], [0, 0, 0]
                    size[axis], kk[axis], ss[axis], pp[axis] = n, k, s, p
                    try:
                        ref = tuple(F.max_pool3d(torch.zeros(1, 1, *size), tuple(kk), tuple(ss), tuple(pp)).shape[-3:])
                    except RuntimeError:
                        ref = None
                    if ref is None:
                        rejected += 1
                        with pytest.raises(ValueError, match="output size"):
                            HF.max_pool3d_geometry((1, 1, *size), tuple(kk), tuple(ss), tuple(pp))
                    else:
                        accepted += 1
                        assert HF.max_pool3d_geometry((1, 1, *size), tuple(kk), tuple(ss), tuple(pp)) == \
                            (tuple(kk), tuple(ss), tuple(pp), ref), (size, kk, ss, pp)
    assert accepted > 0 and rejected > 0


def test_geometry_normalises_like_torch():
    assert HF.max_pool3d_geometry((2, 3, 5, 9, 70), (1, 2, 2), None, 0) == ((1, 2, 2), (1, 2, 2), (0, 0, 0), (5, 4, 35))
    assert HF.max_pool3d_geometry((7, 9, 11), 3, 2, 1) == ((3, 3, 3), (2, 2, 2), (1, 1, 1), (4, 5, 6))
    assert HF.max_pool3d_geometry((6, 7, 13), [2, 3, 4], [2, 1, 3], [1, 1, 2])[3] == \
        tuple(F.max_pool3d(torch.zeros(1, 1, 6, 7, 13), (2, 3, 4), (2, 1, 3), (1, 1, 2)).shape[-3:])
    with pytest.raises(ValueError, match="half of the kernel"):       # torch: "pad should be at most half of effective kernel size"
        HF.max_pool3d_geometry((8, 8, 8), 3, 2, 2)
    with pytest.raises(RuntimeError):
        F.max_pool3d(torch.zeros(1, 1, 8, 8, 8), 3, 2, 2)
    for k, s in ((6, 2), ((2, 2, 7), 2), (2, 6)):
        with pytest.raises(NotImplementedError, match="supported: kernel 1..5, stride 1..5"):
            HF.max_pool3d_geometry((16, 16, 16), k, s, 0)
    with pytest.raises(ValueError):
        HF.max_pool3d_geometry((8, 8, 8), (2, 2), 2, 0)


@pytest.mark.parametrize("kw", [dict(kernel_size=2, dilation=2), dict(kernel_size=2, ceil_mode=True),
                                dict(kernel_size=2, return_indices=True), dict(kernel_size=6), dict(kernel_size=2, stride=6),
                                dict(kernel_size=(1, 2, 6), stride=(1, 2, 2))])
def test_module_limits(kw):
    """Refused before any tensor is looked at (a CPU tensor would be refused as well, by another error)."""
    with pytest.raises(NotImplementedError, match="supported"):
        HipMaxPool3d(**kw)(torch.zeros(1, 1, 12, 12, 12))


def test_module_geometry():
    assert HipMaxPool3d(2, 2, 0).is_2x2x2() and HipMaxPool3d(2).is_2x2x2() and HipMaxPool3d((2, 2, 2), (2, 2, 2)).is_2x2x2()
    for m in (HipMaxPool3d((1, 2, 2)), HipMaxPool3d(2, 2, 1), HipMaxPool3d(2, 1), HipMaxPool3d(3, 2, 1), HipMaxPool3d(2, dilation=2),
              HipMaxPool3d(2, ceil_mode=True), HipMaxPool3d(2, return_indices=True), HipMaxPool3d(6)):
        assert not m.is_2x2x2()
    assert HipMaxPool3d((1, 2, 2)).geometry() == ((1, 2, 2), (1, 2, 2), (0, 0, 0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):        # a supported geometry reaches the device check
        HipMaxPool3d(3, 2, 1)(torch.zeros(1, 1, 8, 8, 8))


GOOD = dict(N=1, C=2, D=8, H=8, W=8, kd=3, kh=3, kw=3, sd=2, sh=2, sw=2, pd=1, ph=1, pw=1)


@pytest.mark.parametrize("over, msg", [
    (dict(kw=6), "kernel 6"), (dict(kd=0), "kernel 0"), (dict(sh=0), "stride 0"), (dict(sd=6), "stride 6"),
    (dict(pw=2), "padding 2"), (dict(kh=2, ph=2), "padding 2"), (dict(pd=-1), "padding -1"),
    (dict(D=2, kd=5, pd=0), "output extent 0"), (dict(C=0), "empty tensor"), (dict(N=300, C=300), "N\\*C=90000 out of range"),
])
def test_bad_geometry_is_reported_without_a_gpu(over, msg):
    geom = [dict(GOOD, **over)[k] for k in GOOD]
    for entry in ("dram_maxpool3d_fwd", "dram_maxpool3d_bwd"):
        with pytest.raises(_lib.DramHipError, match=msg):
            _lib.call(entry, None, None, None, *geom, None)


def test_good_geometry_needs_pointers():
    for entry in ("dram_maxpool3d_fwd", "dram_maxpool3d_bwd"):
        with pytest.raises(_lib.DramHipError, match="null pointer"):
            _lib.call(entry, None, None, None, *GOOD.values(), None)


def test_engine_takes_only_the_2x2x2_pool():
    """The fused engine's _pool launches the 2x2x2 kernel whatever the module says: a network with another pool must take the
    per-op path."""
    model = models.DC3D(**SLIM)
    assert engine.supports(model)
    model.ds_modules[1].maxpool = HipMaxPool3d((1, 2, 2))
    assert not engine.supports(model)
    for other in (HipMaxPool3d(2, 2, 1), HipMaxPool3d(2, 1, 0), HipMaxPool3d(2, ceil_mode=True), HipMaxPool3d(2, dilation=2)):
        model = models.DC3D(**SLIM)
        model.ds_modules[2].maxpool = other
        assert not engine.supports(model)
    model = models.DC3D(**SLIM)
    model.ds_modules[0].maxpool = HipMaxPool3d((2, 2, 2), stride=None, padding=(0, 0, 0))
    assert engine.supports(model)


def test_fixture_layout(golden_dir):
    z = np.load(os.path.join(golden_dir, "pool_geometry.npz"))
    keys = set(z.files)
    geoms = [((1, 2, 2), (1, 2, 2), (0, 0, 0)), ((3, 3, 3), (2, 2, 2), (1, 1, 1)), ((2, 3, 2), (2, 1, 2), (1, 1, 0))]
    for i, geom in enumerate(geoms):
        tag = f"block/{i}/"
        assert tuple(map(tuple, z[tag + "geometry"].tolist())) == geom
        assert z[tag + "in0"].shape == (2, 3, 5, 8, 10) and z[tag + "out/y"].shape == (2, 6, 5, 8, 10)
        assert z[tag + "out/pooled"].shape == (2, 6) + HF.max_pool3d_geometry((5, 8, 10), *geom)[3]
        for k in ("gout/y", "gout/pooled", "gin0", "eval/y", "eval/pooled"):
            assert tag + k in keys, k
        assert z[tag + "gin0"].shape == z[tag + "in0"].shape and z[tag + "gout/pooled"].shape == z[tag + "out/pooled"].shape
        names = {k[len(tag + "sd/"):] for k in keys if k.startswith(tag + "sd/")}
        assert {"conv_blocks.0.0.weight", "conv_blocks.1.1.bias", "conv_blocks.1.1.running_var"} <= names
        assert {k[len(tag + "gparam/"):] for k in keys if k.startswith(tag + "gparam/")} == \
            {n for n in names if "running" not in n and "num_batches" not in n}
    tag = "aniso/"
    assert z[tag + "x"].shape == (1, 1, 8, 16, 16)
    for k in ("train_out", "gout", "gin", "gin64"):
        assert z[tag + k].shape == (1, 1, 8, 16, 16), k
    model = models.DC3D(**dict(SLIM, upsample_sf=(1, 2, 2)))
    assert {k[len(tag + "sdsum/"):] for k in keys if k.startswith(tag + "sdsum/")} == set(model.state_dict())
    shapes = {k: tuple(p.shape) for k, p in model.named_parameters()}
    for sub in ("grad/", "grad64/"):
        assert {k[len(tag + sub):] for k in keys if k.startswith(tag + sub)} == set(GRAD_KEYS)
        for k in GRAD_KEYS:
            assert z[tag + sub + k].shape == shapes[k] and z[tag + sub + k].dtype == np.float32
    assert os.path.getsize(os.path.join(golden_dir, "pool_geometry.npz")) < (1 << 20)
