"""CPU-side checks of the device regression targets (dram_intreg_targets): the C-ABI surface, its argument checks (they
run before any launch), and the finalise arithmetic as tests/targets_restatement.py spells it against the host loop
dram_amd.train_step.regression_targets, bit for bit."""
import ctypes
import os

import numpy as np
import pytest
import torch

import targets_restatement as R
from test_host_cpu import _header_functions

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

# fp32 quotients of integers: 0, 5e-4, 0.001, 0.0099, 0.01, 0.03, 0.05, 0.2, 0.349, 0.35, 0.5, 0.9, 1.0
RATIO_NUM, RATIO_DEN = [0, 5, 10, 99, 100, 300, 500, 2000, 3490, 3500, 5000, 9000, 10000], 10000


def test_library_exports_the_targets_entry_points():
    decl = _header_functions()
    from dram_amd import _lib
    lib = ctypes.CDLL(os.path.join(ROOT, "bodyct-dram_amd", "libdram_hip.so"))
    for name, nargs in (("dram_intreg_targets_ws_bytes", 2), ("dram_intreg_targets", 13)):
        assert hasattr(lib, name), f"libdram_hip.so does not export {name}"
        assert decl[name] == nargs and len(_lib.SIGNATURES[name][1]) == nargs
    res, args = _lib.SIGNATURES["dram_intreg_targets"]
    P, I, L, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
    assert res is I and args == [P, P, P, P, ctypes.c_double, P, P, P, P, Z, I, L, P]
    assert _lib.SIGNATURES["dram_intreg_targets_ws_bytes"] == (Z, [I, L])


def test_targets_argument_errors_are_reported_without_a_gpu():
    from dram_amd import _lib
    q = 16                                  # a dummy non-null, 8-byte aligned pointer: every check comes before the launch
    fr = (ctypes.c_float * 6)(*([1.0 / 6] * 6))
    frp = ctypes.cast(fr, ctypes.c_void_p)
    N, S = 3, 5 * 7 * 9
    need = _lib.lib.dram_intreg_targets_ws_bytes(N, S)
    assert need >= N * 2 * 8 and _lib.lib.dram_intreg_targets_ws_bytes(0, S) == 0
    # several blocks per row at 40^3, and never fewer bytes than the 16-byte-pack launch of the same shape needs
    assert _lib.lib.dram_intreg_targets_ws_bytes(2, 40 ** 3) >= 2 * 16 * 2 * 8
    with pytest.raises(_lib.DramHipError, match="null pointer"):
        _lib.call("dram_intreg_targets", q, q, None, frp, 1e-2, q, q, q, q, need, N, S, None)
    with pytest.raises(_lib.DramHipError, match="null pointer"):
        _lib.call("dram_intreg_targets", q, q, q, None, 1e-2, q, q, q, q, need, N, S, None)
    with pytest.raises(_lib.DramHipError, match="bad dimensions"):
        _lib.call("dram_intreg_targets", q, q, q, frp, 1e-2, q, q, q, q, need, 0, S, None)
    with pytest.raises(_lib.DramHipError, match="8-byte aligned"):
        _lib.call("dram_intreg_targets", q, q, q, frp, 1e-2, q, q, q, q + 4, need, N, S, None)
    with pytest.raises(_lib.DramHipError, match="workspace too small"):
        _lib.call("dram_intreg_targets", q, q, q, frp, 1e-2, q, q, q, q, need - 1, N, S, None)


def test_cpu_tensors_fail_loudly():
    from dram_amd import functional as HF
    m = torch.ones((2, 1, 4, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HF.intreg_targets(m, m, torch.zeros(2, dtype=torch.int32), [1.0 / 6] * 6, 1e-2)


@pytest.mark.parametrize("band_width", [1e-2, 5e-2])
def test_restatement_equals_the_host_loop_bit_for_bit(band_width):
    from dram_amd.train_step import regression_targets
    ctss = np.repeat(np.arange(6), len(RATIO_NUM))
    num = np.tile(np.array(RATIO_NUM), 6)
    ratios = R.ratio(num, np.full_like(num, RATIO_DEN))
    assert ratios.dtype == np.float32
    want = regression_targets([float(c) for c in ctss], torch.from_numpy(ratios), band_width).numpy()
    got, branch = R.band(ctss, ratios, band_width)
    assert got.dtype == np.float32 and got.shape == want.shape == (len(ctss), 2)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    # the grid pins all three cases: the band meets the class interval, lies wholly below it, wholly above it
    assert {R.OVERLAP, R.BELOW, R.ABOVE} == set(branch.tolist())
    assert np.all(got[:, 0] <= got[:, 1])


def test_restatement_weight_keep_and_empty_lobe():
    freq = {0: 0.05, 1: 0.2, 2: 0.5, 3: 0.8, 4: 0.95, 5: 1.0 / 6}
    ctss = np.arange(6)
    w, k = R.weight_keep(ctss, freq)
    want_w = torch.clamp(torch.tensor([freq[int(c)] for c in ctss], dtype=torch.float32), 0.2, 0.8).numpy()
    assert np.array_equal(w.view(np.int32), want_w.view(np.int32))
    assert k.tolist() == [0.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    got, _ = R.band([2], R.ratio(np.array([0]), np.array([0])), 5e-2)
    assert np.isnan(got).all()
