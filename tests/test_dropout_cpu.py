"""Device dropout without a GPU: the numpy restatement of its generator and mask (tests/philox_restatement.py) against the
published Random123 answers and against the statistics a Bernoulli mask must have, the module wiring of parts / modules, and
the argument checks of dram_dropout.  tests/test_gpu_dropout.py holds the kernel to the same restatement bit for bit."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from philox_restatement import dropout_mask, dropout_scale, philox4x32_10, threshold24

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

# Random123 kat_vectors, philox4x32 with 10 rounds: counter, key, output
KNOWN_ANSWERS = [
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


def _words(s):
    return [int(w, 16) for w in s.split()]


@pytest.mark.parametrize("ctr,key,out", KNOWN_ANSWERS)
def test_restatement_reproduces_random123_known_answers(ctr, key, out):
    got = [int(v) for v in philox4x32_10(_words(ctr), _words(key))]
    assert got == _words(out), [f"{v:08x}" for v in got]


def test_restatement_is_elementwise_over_counter_arrays():
    """The vectorised form (what dropout_mask uses) gives, per position, what the scalar call gives."""
    c0 = np.array([0, 0xFFFFFFFF, 0x243F6A88, 7], dtype=np.uint64)
    r = philox4x32_10((c0, 5, 0xFFFFFFFF, 1), (0xA4093822, 0x299F31D0))
    for j, v in enumerate(c0):
        one = philox4x32_10((int(v), 5, 0xFFFFFFFF, 1), (0xA4093822, 0x299F31D0))
        assert [int(w[j]) for w in r] == [int(w) for w in one]


@pytest.mark.parametrize("p,T", [(0.1, 1677722), (0.5, 8388608)])
def test_mask_statistics(p, T):
    """n = 2^20 elements, seed 1234.  With q = 1 - T / 2^24 the kept share, the share of adjacent pairs both kept and the
    agreement between the masks of offsets 0 and 4 (two consecutive calls) are each within 5 binomial standard deviations
    of q, q^2 and q^2 + (1 - q)^2: the bits are uniform, neighbours are independent, and so are consecutive calls."""
    n, seed = 1 << 20, 1234
    assert threshold24(p) == T
    q = 1.0 - T / 2.0 ** 24
    m0, m4 = dropout_mask(n, p, seed, 0), dropout_mask(n, p, seed, 4)
    assert m0.shape == (n,) and m0.dtype == bool

    def sigmas(share, expect, trials):
        return abs(share - expect) / math.sqrt(expect * (1.0 - expect) / trials)
    kept = sigmas(m0.mean(), q, n)
    pairs = sigmas((m0[:-1] & m0[1:]).mean(), q * q, n - 1)
    agree = sigmas((m0 == m4).mean(), q * q + (1 - q) ** 2, n)
    print(f"p={p}: kept {kept:.2f} sigma, adjacent pairs {pairs:.2f} sigma, offsets 0 / 4 agreement {agree:.2f} sigma")
    assert kept < 5 and pairs < 5 and agree < 5, (kept, pairs, agree)


def test_mask_edges_and_prefix_property():
    """p = 0 keeps everything, p = 1 nothing (threshold 2^24 is above every 24-bit value); the mask of a shorter tensor is a
    prefix of the mask of a longer one (it depends on the element index, not on n), for any n % 4."""
    assert dropout_mask(1001, 0.0, 9, 8).all()
    assert not dropout_mask(1001, 1.0, 9, 8).any()
    assert dropout_scale(1.0) == 0 and dropout_scale(0.5) == 2 and dropout_scale(0.1) == np.float32(1.0 / 0.9)
    full = dropout_mask(1027, 0.3, 2 ** 40 + 7, 2 ** 33 + 4)
    for n in (1, 3, 4, 5, 1023, 1024, 1025):
        assert np.array_equal(dropout_mask(n, 0.3, 2 ** 40 + 7, 2 ** 33 + 4), full[:n])
    assert not np.array_equal(full, dropout_mask(1027, 0.3, 2 ** 40 + 7, 4))        # the high offset word counts
    assert not np.array_equal(full, dropout_mask(1027, 0.3, 7, 2 ** 33 + 4))        # and the high seed word


def test_conv_stack_appends_hip_dropout():
    import parts
    from dram_amd.modules import HipDropout
    blk = parts.ConvBlock5d([3, 4], [4, 6], 0, (3, 3), False, (1, 1), dropout=0.1)
    for stage in blk.conv_blocks:
        assert len(stage) == 4
        assert isinstance(stage[3], HipDropout) and isinstance(stage[3], nn.Dropout) and stage[3].p == 0.1
    assert isinstance(blk.conv_blocks[0][3], HipDropout)
    plain = parts.ConvBlock5d([3, 4], [4, 6], 0, (3, 3), False, (1, 1), dropout=0.0)
    assert all(len(stage) == 3 for stage in plain.conv_blocks)
    # a dropout module has no parameters or buffers: the state-dict keys do not move
    assert list(blk.state_dict()) == list(plain.state_dict())


def test_no_other_dropout_is_constructed_in_a_model():
    import models
    from dram_amd.configs import SLIM
    from dram_amd.modules import HipDropout
    model = models.DC3D(**dict(SLIM, dropout=0.1))
    drops = [m for m in model.modules() if isinstance(m, nn.Dropout)]
    assert len(drops) == sum(len(b.conv_blocks) for b in list(model.ds_modules) + [model.bg] + list(model.us_modules))
    assert all(type(m) is HipDropout for m in drops)


def test_hip_dropout_identity_and_no_cpu_fallback():
    from dram_amd.modules import HipDropout
    t = torch.randn(2, 3, 4)
    assert HipDropout(0.3).eval()(t) is t
    assert HipDropout(0.0).train()(t) is t
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HipDropout(0.3).train()(t)


def test_dropout_constants():
    from dram_amd import functional as HF
    for p in (0.0, 0.1, 0.25, 0.5, 1.0):
        T, scale = HF.dropout_constants(p)
        assert T == threshold24(p) and np.float32(scale) == dropout_scale(p)
    with pytest.raises(ValueError):
        HF.dropout_constants(1.5)


def test_entry_point_argument_checks_without_a_gpu():
    from dram_amd import _lib
    buf = (np.zeros(8, dtype=np.float32)).ctypes.data     # never dereferenced: every call below stops at its check
    with pytest.raises(_lib.DramHipError, match="null pointer"):
        _lib.call("dram_dropout", None, buf, 4, 0, 1.0, 0, 0, None)
    with pytest.raises(_lib.DramHipError, match="null pointer"):
        _lib.call("dram_dropout", buf, None, 4, 0, 1.0, 0, 0, None)
    with pytest.raises(_lib.DramHipError, match="threshold24"):
        _lib.call("dram_dropout", buf, buf, 4, (1 << 24) + 1, 1.0, 0, 0, None)
    with pytest.raises(_lib.DramHipError, match="negative"):
        _lib.call("dram_dropout", buf, buf, -1, 0, 1.0, 0, 0, None)
    _lib.call("dram_dropout", None, None, 0, 1 << 24, 0.0, 0, 0, None)       # n == 0: nothing to do, no error
    assert "dram_dropout" in _lib.SIGNATURES and len(_lib.SIGNATURES["dram_dropout"][1]) == 8
    header = open(os.path.join(ROOT, "include", "dram_hip.h")).read()
    assert re.search(r"\bint\s+dram_dropout\s*\(", header)
    assert _lib.lib.dram_abi_version() == 2
