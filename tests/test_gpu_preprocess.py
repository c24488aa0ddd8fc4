"""The device chunk loader (csrc/prep.hip, dram_amd/preprocess.py) against the oracle's restatements composed the way the
reference composes them (tests/preprocess_cases.py).  Every comparison is bit-exact: both sides run the same fp64 (threshold,
grid, lerps) and fp32 (windowing) operations in the same order with rounded products.  Parity with SimpleITK / skimage
themselves stays unpinned (libraries absent), as for dram_resample_volume and dram_scan_hist256."""
import numpy as np
import pytest
import torch

import preprocess_cases as PC
from dram_amd import _lib
from dram_amd.inference import binary_cam_threshold
from dram_amd.preprocess import ChunkLoader, resample_plan
from oracle import dram_oracle as O

pytestmark = pytest.mark.gpu
KEYS = ("#image", "#lobe_reference", "#pseudo_lesion_reference", "#vessel_reference")
_CACHE = {}


def _chunks():
    if "chunks" not in _CACHE:
        _CACHE["chunks"] = PC.make_chunks()
    return _CACHE["chunks"]


def _oracle(out_size):
    """The six chunks prepared on the host, once per output size (with the vessel masks; a run without them drops that key)."""
    if out_size not in _CACHE:
        plan = lambda spacing, size: resample_plan("fixed_size", None, out_size, spacing, size)
        _CACHE[out_size] = [PC.oracle_prepare(c, out_size, plan) for c in _chunks()]
    return _CACHE[out_size]


def _device(out_size, chunks):
    loader = ChunkLoader(out_size, PC.WINDOW, PC.PSEUDO_WINDOW, PC.PSEUDO_SCALER)
    out = loader(loader.pack(chunks))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("with_vessel", [True, False])
@pytest.mark.parametrize("out_size", PC.OUT_SIZES)
def test_ragged_batch_is_bit_exact(out_size, with_vessel):
    chunks = _chunks() if with_vessel else [{k: v for k, v in c.items() if k != "#vessel_reference"} for c in _chunks()]
    got = _device(out_size, chunks)
    ref = _oracle(out_size)
    assert ("#vessel_reference" in got) == with_vessel
    for k in KEYS[:3 + with_vessel]:
        assert got[k].shape == (6, 1) + tuple(out_size) and got[k].dtype == np.float32
    assert got["threshold"].dtype == np.float64
    for i, (r, th) in enumerate(ref):
        assert got["threshold"][i] == th, (i, got["threshold"][i], th)
        for k in KEYS[:3 + with_vessel]:
            g = got[k][i, 0]
            assert np.array_equal(g, r[k]), (i, k, int((g != r[k]).sum()), float(np.abs(g - r[k]).max()))
    # (5,5,5) upsampled: c = o * 5 / size_out is beyond size_in - 0.5 = 4.5 for the last outputs of every axis -> 0 in all outputs
    for k in KEYS[:3 + with_vessel]:
        v = got[k][2, 0]
        e = [int(np.ceil(4.5 * n / 5)) for n in out_size]                      # the first output index outside, per axis
        assert e[2] < out_size[2] and (v[e[0]:] == 0).all() and (v[:, e[1]:] == 0).all() and (v[:, :, e[2]:] == 0).all()
    assert (got["#image"][2, 0][:-2, :-2, :-2] != 0).any()
    assert got["#lobe_reference"][3].max() == 3.0 and got["#pseudo_lesion_reference"][3].max() == 1.0   # a label above 1 counts as lobe
    assert 0 < got["#pseudo_lesion_reference"].mean() < 1
    if out_size == PC.SHAPES[5]:                           # same size: the identity grid
        assert np.array_equal(got["#lobe_reference"][5, 0], _chunks()[5]["#lobe_reference"].astype(np.float32))


def _hists():
    rng = np.random.default_rng(3)
    sym = np.zeros(256, dtype=np.int64)
    sym[[10, 20, 30]] = [7, 7, 7]                          # var12 at t = 10..19 equals var12 at t = 20..29: the first maximum wins
    big = rng.integers(0, 1 << 20, 256).astype(np.int64)
    big[[40, 41, 200]] = [(1 << 33) + 12345, (1 << 34) + 1, (1 << 32) + 7]
    sparse = np.zeros(256, dtype=np.int64)
    sparse[rng.choice(256, 40, replace=False)] = rng.integers(1, 1000, 40)
    two = np.zeros(256, dtype=np.int64)
    two[[17, 230]] = [100, 3]
    one = np.zeros(256, dtype=np.int64)
    one[99] = 12
    top = np.zeros(256, dtype=np.int64)
    top[[254, 255]] = [3, 9]
    flat = np.full(256, 4, dtype=np.int64)                 # symmetric over the whole range: tied maxima around the middle
    return {"random": rng.integers(0, 5000, 256).astype(np.int64), "sparse": sparse, "two_bins": two, "one_bin": one,
            "zero": np.zeros(256, dtype=np.int64), "tied": sym, "flat": flat, "above_2^32": big, "top_bins": top}


def test_otsu256_on_hand_made_histograms():
    hists = _hists()
    names = list(hists)
    h = torch.as_tensor(np.stack([hists[n] for n in names])).cuda()
    st = torch.cuda.current_stream().cuda_stream
    # the tie is real: the numpy restatement sees equal between-class variances at two thresholds and takes the first
    hs = hists["tied"].astype(np.float64)
    var = lambda t: hs[:t + 1].sum() * hs[t + 1:].sum() * ((hs[:t + 1] * np.arange(t + 1)).sum() / hs[:t + 1].sum()
                                                         - (hs[t + 1:] * np.arange(t + 1, 256)).sum() / hs[t + 1:].sum()) ** 2
    assert var(10) == var(20) and O.threshold_otsu_u8(np.repeat(np.arange(256), hists["tied"]).astype(np.uint8)) == 10.0
    for scaler in (1.0, 0.75):
        th = torch.full((len(names),), -1.0, dtype=torch.float64, device="cuda")
        _lib.call("dram_otsu256", h.data_ptr(), len(names), scaler, th.data_ptr(), st)
        got = th.cpu().numpy()
        for i, n in enumerate(names):
            if n == "zero":
                assert got[i] == np.inf                     # the reference raises IndexError here (documented deviation)
            else:
                assert got[i] == binary_cam_threshold(hists[n], scaler), (n, scaler, got[i], binary_cam_threshold(hists[n], scaler))
    assert binary_cam_threshold(hists["top_bins"], 1.0) == 254 / 255.0 and binary_cam_threshold(hists["one_bin"], 0.75) == 99 / 255.0


def test_chunk_hist256_per_sample():
    chunks = _chunks()
    loader = ChunkLoader(PC.OUT_SIZES[0], PC.WINDOW)
    packed = loader.pack(chunks)
    st = torch.cuda.current_stream().cuda_stream
    N = len(chunks)
    hist = torch.full((N, 256), -1, dtype=torch.int64, device="cuda")
    _lib.call("dram_chunk_hist256", packed.d_scans.data_ptr(), packed.d_lobes.data_ptr(), packed.d_table.data_ptr(), N,
              hist.data_ptr(), *PC.PSEUDO_WINDOW, st)
    got = hist.cpu().numpy()
    one = torch.empty(256, dtype=torch.int64, device="cuda")
    for i, c in enumerate(chunks):
        scan, lobe = c["#image"], c["#lobe_reference"]
        w = O.windowing(scan, from_span=PC.PSEUDO_WINDOW, to_span=(0, 1))[lobe > 0]
        view = O.windowing(w, from_span=(0, 1), to_span=(0, 255)).astype(np.uint8)          # binary_cam's 8-bit view
        assert np.array_equal(got[i], np.bincount(view, minlength=256)), i
        scan_d, lobe_d = torch.as_tensor(scan).cuda(), torch.as_tensor(lobe).cuda()
        _lib.call("dram_scan_hist256", scan_d.data_ptr(), lobe_d.data_ptr(), one.data_ptr(), *PC.PSEUDO_WINDOW, scan.size, st)
        assert np.array_equal(got[i], one.cpu().numpy()), i
        assert got[i].sum() == int((lobe > 0).sum())


def test_chunk_hist256_past_one_lap():
    """N = 2, so 512 blocks per sample; chunk 1 starts at element 105 and holds 1,055,700: the stride loop of
    chunk_hist_kernel takes a second, partly filled step, and the lobe has voxels in both (asserted on the host)."""
    chunks = PC.make_hist_chunks()
    start = PC.hist_second_lap_start()
    lobe1 = chunks[1]["#lobe_reference"].ravel()
    assert lobe1[:start].any() and lobe1[start:].any()
    packed = ChunkLoader(PC.OUT_SIZES[0], PC.WINDOW).pack(chunks)
    assert packed.offsets == [0, 105]
    st = torch.cuda.current_stream().cuda_stream
    hist = torch.full((2, 256), -1, dtype=torch.int64, device="cuda")
    _lib.call("dram_chunk_hist256", packed.d_scans.data_ptr(), packed.d_lobes.data_ptr(), packed.d_table.data_ptr(), 2,
              hist.data_ptr(), *PC.PSEUDO_WINDOW, st)
    got = hist.cpu().numpy()
    for i, c in enumerate(chunks):
        assert np.array_equal(got[i], PC.hist_expected(c)), i
        assert got[i].sum() == int((c["#lobe_reference"] > 0).sum())
    one = torch.full((256,), -1, dtype=torch.int64, device="cuda")
    scan_d, lobe_d = torch.as_tensor(chunks[1]["#image"]).cuda(), torch.as_tensor(chunks[1]["#lobe_reference"]).cuda()
    _lib.call("dram_scan_hist256", scan_d.data_ptr(), lobe_d.data_ptr(), one.data_ptr(), *PC.PSEUDO_WINDOW, scan_d.numel(), st)
    assert np.array_equal(got[1], one.cpu().numpy())


@pytest.mark.parametrize("with_vessel", [True, False])
@pytest.mark.parametrize("out_size", PC.ROW_REGIME_SIZES)
def test_ragged_batch_is_bit_exact_in_every_rows_regime(out_size, with_vessel):
    """rows = 63 with output quads shared by two blocks, an x table of two strides with rows = 7, one row per block at
    Wo = 2048 (tests/preprocess_cases.py: ROW_REGIME_SIZES)."""
    chunks = _chunks() if with_vessel else [{k: v for k, v in c.items() if k != "#vessel_reference"} for c in _chunks()]
    got = _device(out_size, chunks)
    ref = _oracle(out_size)
    assert ("#vessel_reference" in got) == with_vessel
    for i, (r, th) in enumerate(ref):
        assert got["threshold"][i] == th, (i, got["threshold"][i], th)
        for k in KEYS[:3 + with_vessel]:
            g = got[k][i, 0]
            assert g.shape == tuple(out_size) and g.dtype == np.float32
            assert np.array_equal(g, r[k]), (i, k, int((g != r[k]).sum()), float(np.abs(g - r[k]).max()))
    assert 0 < got["#pseudo_lesion_reference"].mean() < 1 and (got["#image"] != 0).any()


def _prepare_raw(packed, th, out_size, outs, vessel=True):
    """dram_chunk_prepare itself on four output pointers (image, lobe, lesion, vessel); returns the status."""
    Do, Ho, Wo = out_size
    return _lib.lib.dram_chunk_prepare(packed.d_scans.data_ptr(), packed.d_lobes.data_ptr(), packed.d_vessels.data_ptr() if vessel else None,
                                       packed.d_table.data_ptr(), th.data_ptr(), len(packed), Do, Ho, Wo, float(PC.WINDOW[0]),
                                       float(PC.WINDOW[1]), *PC.PSEUDO_WINDOW, outs[0], outs[1], outs[2], outs[3] if vessel else None,
                                       torch.cuda.current_stream().cuda_stream)


def test_an_output_row_above_the_cap_is_refused_and_nothing_is_written():
    out_size = (1, 2, PC.MAX_WO + 1)
    loader = ChunkLoader(PC.OUT_SIZES[0], PC.WINDOW)
    packed = loader.pack(_chunks())
    th = torch.full((len(packed),), 0.5, dtype=torch.float64, device="cuda")
    out = torch.full((4, len(packed)) + out_size, -7.0, device="cuda")
    assert _prepare_raw(packed, th, out_size, [o.data_ptr() for o in out]) != 0
    assert b"Wo up to 2048" in _lib.lib.dram_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7).all())
    at_cap = (1, 2, PC.MAX_WO)                                                       # one less is accepted and fills every output
    assert _prepare_raw(packed, th, at_cap, [o.data_ptr() for o in out]) == 0
    torch.cuda.synchronize()
    filled = out.view(4, -1)[:, :len(packed) * 2 * PC.MAX_WO]
    assert bool((filled != -7).all()) and bool((out.view(4, -1)[:, len(packed) * 2 * PC.MAX_WO:] == -7).all())


def test_outputs_one_float_off_16_bytes_give_the_same_bits():
    """Every output pointer 4 bytes past a 16-byte boundary: each quad takes the element-wise stores.  Same bits as the aligned
    run, guard words on both sides of every output untouched."""
    out_size = PC.ROW_REGIME_SIZES[0]
    loader = ChunkLoader(out_size, PC.WINDOW, PC.PSEUDO_WINDOW, PC.PSEUDO_SCALER)
    packed = loader.pack(_chunks())
    aligned = loader(packed)
    n = aligned["#image"].numel()
    front, back = 5, 27                                                              # 20 bytes: one float past 16-byte alignment
    bufs = [torch.full((front + n + back,), -7.0, device="cuda") for _ in range(4)]
    ptrs = [b.data_ptr() + 4 * front for b in bufs]
    assert all(b.data_ptr() % 16 == 0 for b in bufs) and all(p % 16 == 4 for p in ptrs)
    assert _prepare_raw(packed, aligned["threshold"], out_size, ptrs) == 0
    torch.cuda.synchronize()
    for k, b in zip(KEYS, bufs):
        assert torch.equal(b[front:front + n].view(torch.int32), aligned[k].reshape(-1).view(torch.int32)), k
        assert bool((b[:front] == -7).all()) and bool((b[front + n:] == -7).all()), k
    assert bool((aligned["#image"] != 0).any()) and bool((aligned["#vessel_reference"] != 0).any())


def test_outputs_do_not_depend_on_the_packing_order():
    fwd = _device(PC.OUT_SIZES[1], _chunks())
    rev = _device(PC.OUT_SIZES[1], _chunks()[::-1])
    for k in KEYS + ("threshold",):
        assert np.array_equal(fwd[k], rev[k][::-1]), k


def test_batch_from_chunks_trains():
    import models
    from dram_amd.configs import SLIM
    from dram_amd.train_step import Batch, DataParallelTrainer, regression_targets
    size = (16, 16, 16)
    chunks = [c for i, c in enumerate(_chunks()) if i != 3]                # lobes of {0, 1}: the ratio's sums are exact integers
    ctss = [0.0, 1.0, 2.0, 3.0, 5.0]
    freq = {k: 1.0 / 6 for k in range(6)}
    loader = ChunkLoader(size, PC.WINDOW, PC.PSEUDO_WINDOW, PC.PSEUDO_SCALER)
    batch = Batch.from_chunks(chunks, ctss, freq, loader, band_width=1e-2)
    assert len(batch) == 5 and batch.images.shape == (5, 1) + size and batch.images.is_cuda
    plan = lambda spacing, cur: resample_plan("fixed_size", None, size, spacing, cur)
    ref = [PC.oracle_prepare(c, size, plan)[0] for c in chunks]
    lobes = torch.from_numpy(np.stack([r["#lobe_reference"] for r in ref]))
    lesions = torch.from_numpy(np.stack([r["#pseudo_lesion_reference"] for r in ref]))
    assert torch.equal(batch.images.cpu()[:, 0], torch.from_numpy(np.stack([r["#image"] for r in ref])))
    ratio = (lesions * lobes).view(5, -1).sum(-1) / lobes.view(5, -1).sum(-1)
    assert torch.equal(batch.targets.cpu(), regression_targets(ctss, ratio, 1e-2))
    torch.manual_seed(3)
    m = models.DC3D(**SLIM)
    m.init(models.HeNorm(mode="fan_in"))
    m = m.cuda().train()
    tr = DataParallelTrainer(m, torch.optim.SGD(m.parameters(), lr=1e-3))
    reg, seg = tr.step(batch)
    assert torch.isfinite(reg).all() and torch.isfinite(seg).all()


def test_argument_errors_launch_nothing():
    st = torch.cuda.current_stream().cuda_stream
    loader = ChunkLoader(PC.OUT_SIZES[0], PC.WINDOW)
    packed = loader.pack(_chunks())
    N = len(packed)
    hist = torch.full((N, 256), -7, dtype=torch.int64, device="cuda")
    th = torch.full((N,), -7.0, dtype=torch.float64, device="cuda")
    out = torch.full((2, N) + PC.OUT_SIZES[0], -7.0, device="cuda")
    s, l, t = packed.d_scans.data_ptr(), packed.d_lobes.data_ptr(), packed.d_table.data_ptr()
    D, H, W = PC.OUT_SIZES[0]
    prep = lambda n, tab, w0, w1: _lib.lib.dram_chunk_prepare(s, l, None, tab, None, n, D, H, W, w0, w1, -1150, 350,
                                                              out[0].data_ptr(), out[1].data_ptr(), None, None, st)
    calls = [lambda: _lib.lib.dram_chunk_hist256(s, l, t, 0, hist.data_ptr(), -1150, 350, st),
             lambda: _lib.lib.dram_chunk_hist256(s, l, None, N, hist.data_ptr(), -1150, 350, st),
             lambda: _lib.lib.dram_chunk_hist256(s, l, t, N, hist.data_ptr(), 350, 350, st),
             lambda: _lib.lib.dram_otsu256(hist.data_ptr(), 0, 0.75, th.data_ptr(), st),
             lambda: _lib.lib.dram_otsu256(None, N, 0.75, th.data_ptr(), st),
             lambda: prep(0, t, -1000.0, -300.0), lambda: prep(N, None, -1000.0, -300.0), lambda: prep(N, t, -300.0, -300.0),
             lambda: prep(N, t, -300.0, -1000.0)]
    for i, c in enumerate(calls):
        assert c() != 0, i
        assert _lib.lib.dram_last_error(), i
    torch.cuda.synchronize()
    assert (hist == -7).all() and (th == -7).all() and (out == -7).all()            # nothing was launched, not even the memset
    assert prep(N, t, -1000.0, -300.0) == 0                                          # the same call with good arguments runs
    torch.cuda.synchronize()
    assert (out != -7).all()
