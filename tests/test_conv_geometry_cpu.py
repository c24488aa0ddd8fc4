"""CPU checks of the general 3-D convolution's host side: argument errors of the C entry points (reported without a GPU),
HipConv3d's kind selection and its limits, and which networks the fused engine takes."""
import ctypes

import pytest

import models
from dram_amd import _lib, engine
from dram_amd import functional as HF
from dram_amd.configs import SLIM, ST_DRAM_REF_MODEL
from dram_amd.modules import HipConv3d

GOOD = dict(N=1, Cin=4, Cout=8, D=9, H=9, W=9, kz=3, ky=3, kx=3, sz=1, sy=1, sx=1, pz=0, py=0, px=0)


def _geom(**over):
    g = dict(GOOD, **over)
    return [g[k] for k in ("N", "Cin", "Cout", "D", "H", "W", "kz", "ky", "kx", "sz", "sy", "sx", "pz", "py", "px")]


@pytest.mark.parametrize("over, msg", [
    (dict(kx=8), "kernel size 8"), (dict(kz=0), "kernel size 0"), (dict(sy=3), "stride 3"),
    (dict(px=3), "padding 3"), (dict(kx=1, px=2), "padding 2"), (dict(pz=-1), "padding -1"), (dict(D=2, kz=5, pz=1), "output size below 1"),
    (dict(Cin=0), "non-positive"),
])
def test_bad_geometry_is_reported_without_a_gpu(over, msg):
    geom = _geom(**over)
    with pytest.raises(_lib.DramHipError, match=msg):
        _lib.call("dram_conv3d_fwd", None, None, None, None, *geom, None)
    with pytest.raises(_lib.DramHipError, match=msg):
        _lib.call("dram_conv3d_bwd_data", None, None, None, *geom, None)
    with pytest.raises(_lib.DramHipError, match=msg):
        _lib.call("dram_conv3d_wgrad", None, None, None, None, 0, *geom, None)
    assert _lib.lib.dram_conv3d_wgrad_ws_bytes(*geom) == 0


def test_good_geometry_needs_pointers_and_workspace():
    with pytest.raises(_lib.DramHipError, match="null pointer"):
        _lib.call("dram_conv3d_fwd", None, None, None, None, *_geom(), None)
    assert _lib.lib.dram_conv3d_wgrad_ws_bytes(*_geom()) > 0
    fake = ctypes.c_void_p(16)      # never dereferenced: the workspace check comes first
    with pytest.raises(_lib.DramHipError, match="workspace"):
        _lib.call("dram_conv3d_wgrad", fake, fake, fake, fake, 4, *_geom(), None)


def test_launch_counts_have_their_own_kinds():
    arr = (ctypes.c_ulonglong * HF.GEN_KINDS)()
    _lib.call("dram_conv3d_gen_launch_counts", ctypes.cast(arr, ctypes.c_void_p), HF.GEN_KINDS)
    assert HF.GEN_KINDS == 3


@pytest.mark.parametrize("kw, kind", [
    (dict(kernel_size=3, padding=1), 3), (dict(kernel_size=1, padding=0), 1),
    (dict(kernel_size=3, padding=0), "gen"), (dict(kernel_size=5, padding=2), "gen"),
    (dict(kernel_size=(1, 3, 3), padding=(0, 1, 1)), "gen"), (dict(kernel_size=3, padding=1, stride=2), "gen"),
    (dict(kernel_size=1, padding=0, stride=(1, 2, 2)), "gen"), (dict(kernel_size=2, stride=2), "gen"),
    (dict(kernel_size=7, padding=6), "gen"), (dict(kernel_size=1, padding=1), "gen"),
])
def test_kind(kw, kind):
    assert HipConv3d(2, 3, **kw)._kind() == kind


@pytest.mark.parametrize("kw", [dict(kernel_size=3, padding=1, dilation=2), dict(kernel_size=3, padding=1, groups=2),
                                dict(kernel_size=3, padding=1, stride=3), dict(kernel_size=9, padding=4),
                                dict(kernel_size=3, padding=3), dict(kernel_size=3, padding="same"),
                                dict(kernel_size=3, padding=1, padding_mode="circular")])
def test_kind_limits(kw):
    with pytest.raises(NotImplementedError, match="supported: kernel 1..7"):
        HipConv3d(2, 2, **kw)._kind()


def test_engine_covers_only_the_standard_network():
    assert engine.supports(models.DC3D(**SLIM))
    assert engine.supports(models.DC3D(**ST_DRAM_REF_MODEL))
    assert not engine.supports(models.DC3D(**dict(SLIM, padding_list=[(0, 0)] * 7)))
    assert not engine.supports(models.DC3D(**dict(SLIM, kernel_sizes=[(5, 3)] * 7, padding_list=[(2, 1)] * 7)))
    assert not engine.supports(models.DC3D(**dict(SLIM, kernel_sizes=[((1, 3, 3), (1, 3, 3))] * 7,
                                                  padding_list=[((0, 1, 1), (0, 1, 1))] * 7)))


def test_output_size():
    assert HF.conv_out_size((13, 18, 21), (3, 3, 3), (2, 2, 2), (1, 1, 1)) == (7, 9, 11)
    with pytest.raises(ValueError, match="output size"):
        HF.conv_out_size((4, 8, 8), (5, 5, 5), (1, 1, 1), (0, 0, 0))
