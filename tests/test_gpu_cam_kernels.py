"""The three kernels of csrc/infer_cam.hip one by one, through the C ABI: dram_lobe_chunk_masks, dram_lobe_cam_max and
dram_lobe_cam_paste, each against the plain restatement of tests/cam_cases.py (which tests/test_cam_cpu.py ties to torch's CPU
ops and to the oracle).  Volume (14, 37, 45), R = 6 and 12, C = 6 and 1, L = 1 and 8; the boxes and what is planted in them
are described at cam_cases.CHUNKS_8 / kernel_inputs: a box of 3100 voxels whose maximum sits at its last voxel, outside the
lobe; a maximum at an outside-lobe voxel; overlapping boxes of different labels; a one-plane box; boxes thinner than R; a
class-0 chunk; an all-non-positive channel; ties and NaNs in `pool`.

The mask and the classes are compared bit for bit; the maximum and the heat map within cam_cases.max_tol / quotient_tol
(derived there).  Every output is handed over filled with a sentinel, so that an element the kernel did not write shows, and
`pool` is fed directly, so that no summation order can flip a near tie."""
import ctypes

import numpy as np
import pytest
import torch

import cam_cases as CK

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(R, C, L) for R in CK.RS for C in (6, 1) for L in (1, 8)]


def call(name, *args):
    from dram_amd import _lib
    _lib.call(name, *args, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def dev(a):
    return torch.tensor(np.ascontiguousarray(a)).to(DEV)


def chunk_array(chunks):
    return (ctypes.c_int * (7 * len(chunks)))(*[v for c in chunks for v in c])


@pytest.mark.parametrize("R", CK.RS)
@pytest.mark.parametrize("L", [1, 8])
def test_lobe_chunk_masks_bit_exact(R, L):
    """out = 1.0 / 0.0 exactly as the nearest-neighbour resample of (lobe == label) on the crop -> R^3 grid, 0.0 beyond the
    buffer of a crop thinner than R (boxes 1 and 2); the output starts as NaN, and the slots past L stay NaN."""
    chunks, _, _, lobe, _ = CK.kernel_inputs(R, 6, L)
    ref = CK.chunk_mask_ref(lobe, chunks, R)
    D, H, W = lobe.shape
    out = torch.full((L + 1, 1, R, R, R), float("nan"), dtype=torch.float32, device=DEV)
    lobe_d = dev(lobe)
    call("dram_lobe_chunk_masks", lobe_d.data_ptr(), out.data_ptr(), chunk_array(chunks), L, D, H, W, R)
    got = out.cpu().numpy()
    assert np.isnan(got[L]).all()
    assert np.array_equal(got[:L, 0], ref), int((got[:L, 0] != ref).sum())
    if L == 8:
        assert not got[1, 0][:, :, int(np.ceil(1.5 * R / 2)):].any() and got[1, 0].any()


def run_cam_max(dense_d, pool_d, chunks, C, R):
    L = len(chunks)
    cls = torch.full((L + 1,), -7, dtype=torch.int32, device=DEV)
    mx = torch.full((L + 1,), float("nan"), dtype=torch.float32, device=DEV)          # (the entry point zeroes its L slots)
    call("dram_lobe_cam_max", dense_d.data_ptr(), pool_d.data_ptr(), chunk_array(chunks), L, C, R, cls.data_ptr(), mx.data_ptr())
    assert int(cls[L]) == -7 and bool(torch.isnan(mx[L]))
    return cls[:L], mx[:L]


@pytest.mark.parametrize("R,C,L", SHAPES)
def test_lobe_cam_max_classes_exact_and_maximum_over_the_box(R, C, L):
    """cls = torch.max's arg-max of every pool row (ties: first; NaN: first NaN), exact.  max = the maximum of
    relu(resize(dense[l, cls])) over the whole box: chunk 0's is the 9.0 planted at the box's last voxel, which the lobe does
    not cover; chunk 4's lies at an outside-lobe voxel too; chunk 2's is exactly 0 (nothing positive)."""
    chunks, dense, pool, lobe, htp0 = CK.kernel_inputs(R, C, L)
    _, _, cls_ref, max_ref, _ = CK.cam_ref(dense, pool, lobe, chunks, R, htp0)
    cls, mx = run_cam_max(dev(dense), dev(pool), chunks, C, R)
    assert cls.cpu().tolist() == cls_ref
    got = mx.cpu().numpy().astype(np.float64)
    for l in range(L):
        bound = CK.max_tol(np.abs(dense[l, cls_ref[l]]).max())
        print(f"cam-kernel-accuracy: cam_max R={R} C={C} L={L} chunk {l}: |err| {abs(got[l] - max_ref[l]):.3e} (bound {bound:.3e})")
        assert abs(got[l] - max_ref[l]) <= bound, l
    if C == 6:
        assert max_ref[0] == CK.SENTINEL_PEAK
        if L == 8:
            assert got[CK.NON_POSITIVE] == 0.0 and not np.signbit(got[CK.NON_POSITIVE])


@pytest.mark.parametrize("R,C,L", SHAPES)
def test_lobe_cam_paste_values_zeros_nans_and_untouched_voxels(R, C, L):
    """htp starts as a sentinel of distinct negative numbers.  Bit for bit: every voxel outside all boxes, and every voxel of
    a box that does not carry that chunk's label, keeps its sentinel; a class-0 chunk writes 0.0 over it; the all-non-positive
    chunk writes NaN where the reference gives NaN.  Elsewhere |got - ref| <= quotient_tol, also where boxes overlap.  The
    class and the maximum come from dram_lobe_cam_max on the device, as in LobeInference."""
    chunks, dense, pool, lobe, htp0 = CK.kernel_inputs(R, C, L)
    ref, written, cls_ref, max_ref, tol = CK.cam_ref(dense, pool, lobe, chunks, R, htp0)
    D, H, W = lobe.shape
    dense_d, lobe_d, htp_d = dev(dense), dev(lobe), dev(htp0)
    cls, mx = run_cam_max(dense_d, dev(pool), chunks, C, R)
    call("dram_lobe_cam_paste", dense_d.data_ptr(), lobe_d.data_ptr(), htp_d.data_ptr(), chunk_array(chunks), cls.data_ptr(),
         mx.data_ptr(), L, C, D, H, W, R)
    got = htp_d.cpu().numpy()
    assert np.array_equal(got[~written], htp0[~written])
    nan_ref = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan_ref)
    if C == 6 and L == 8:
        assert nan_ref.any()
    ok = written & ~nan_ref
    err = np.abs(got.astype(np.float64) - ref)
    print(f"cam-kernel-accuracy: cam_paste R={R} C={C} L={L}: max err {err[ok].max():.3e} (bound up to {tol[ok].max():.3e})")
    assert (err[ok] <= tol[ok]).all(), np.unravel_index(np.where(ok, err - tol, -1).argmax(), err.shape)
    for l, c in enumerate(chunks):
        if cls_ref[l] == 0:
            sel = np.zeros(lobe.shape, dtype=bool)
            sel[CK.K.box(c)] = lobe[CK.K.box(c)] == c[6]
            assert (got[sel] == 0).all() and sel.any()
