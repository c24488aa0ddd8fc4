"""The whole-scan inference kernels of csrc/infer.hip one by one, through the C ABI: dram_label_bboxes, dram_lobe_chunks,
dram_lobe_paste, dram_lung_hist256, dram_threshold_mask, and dram_scan_hist256 / dram_mask_overlap past their grid caps,
each against the plain restatement of tests/infer_kernel_cases.py (which tests/test_infer_kernels_cpu.py ties to the oracle
and to torch's CPU ops).  tests/test_gpu_inference.py sees these kernels only through a model and the loose end-to-end
checks; the inputs here are built so that a one-voxel error changes a result: both paths and both bands of the bounding-box
kernel, non-zero chunk origins, non-cubic and overlapping boxes, foreign labels inside a box, a steep heat map, every 8-bit
bin edge, and sizes past the 2048 x 256 x 16 and 4096 x 256 grid caps.

Integer and comparison results are compared bit for bit.  Every output handed over is filled with a sentinel first (NaN for
floats, 0xAB for bytes, -7 for integers), so that an element the kernel did not write shows."""
import ctypes

import numpy as np
import pytest
import torch

import infer_kernel_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def call(name, *args):
    from dram_amd import _lib
    _lib.call(name, *args, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def dev(a):
    return torch.tensor(np.ascontiguousarray(a)).to(DEV)            # (a copy: the shared inputs are read-only arrays)


def chunk_array(chunks):
    return (ctypes.c_int * (7 * len(chunks)))(*[v for c in chunks for v in c])


# ------------------------------------------------------------------------------------------------ bounding boxes
def run_bboxes(lobe_d, nlabels):
    """All 255 rows are handed over filled with -7: the rows past nlabels must still hold it."""
    D, H, W = lobe_d.shape
    boxes = torch.full((255 * 6,), -7, dtype=torch.int32, device=DEV)
    call("dram_label_bboxes", lobe_d.data_ptr(), boxes.data_ptr(), nlabels, D, H, W)
    got = boxes.cpu().numpy().reshape(255, 6)
    assert (got[nlabels:] == -7).all()
    return got[:nlabels]


def misaligned(lobe):
    """The same map one byte into a larger buffer: 16-byte loads are not possible, the kernel has to take its scalar path."""
    buf = torch.full((lobe.size + 64,), 0xAB, dtype=torch.uint8, device=DEV)
    view = buf[1:1 + lobe.size].view(lobe.shape)
    view.copy_(torch.as_tensor(lobe))
    assert view.data_ptr() % 16 == 1 and view.is_contiguous()
    return view


@pytest.mark.parametrize("nlabels,extra", K.BBOX_NLABELS, ids=["n255", "n6_with_7_and_200"])
@pytest.mark.parametrize("name", sorted(K.BBOX_MAPS))
def test_label_bboxes_bit_exact(name, nlabels, extra):
    """Every map of infer_kernel_cases.BBOX_MAPS with nlabels = 255, and with nlabels = 6 on a map that also holds labels 7
    and 200 (they must neither be reported nor widen a box): H = 70 is two bands of 64 + 6 rows with label 3 in the second
    only and label 1 in both; a uniform group of 16 next to a mixed one; single voxels at the first and the last element;
    W = 32 on an aligned map is the vector path, W = 33 the scalar one; two labels alternating inside a group; the empty map."""
    lobe = K.BBOX_MAPS[name](extra)
    lobe_d = dev(lobe)
    if lobe.shape[2] % 16 == 0:
        assert lobe_d.data_ptr() % 16 == 0                                    # the vector path's condition
    got = run_bboxes(lobe_d, nlabels)
    assert np.array_equal(got, K.bboxes_ref(lobe, nlabels)), name


@pytest.mark.parametrize("nlabels,extra", K.BBOX_NLABELS, ids=["n255", "n6_with_7_and_200"])
def test_label_bboxes_scalar_paths_equal_the_vector_path(nlabels, extra):
    """The (3, 70, 32) map: aligned (vector path), the same bytes one byte into a larger buffer (scalar path by alignment),
    and the same content at W = 33 (scalar path by width), where only label 5's voxel at (D-1, H-1, W-1) sits one column
    further.  The three results against the restatement and against each other."""
    lobe = K.bbox_band_map(32, extra)
    vec = run_bboxes(dev(lobe), nlabels)
    view = misaligned(lobe)
    by_alignment = run_bboxes(view, nlabels)
    by_width = run_bboxes(dev(K.bbox_band_map(33, extra)), nlabels)
    ref = K.bboxes_ref(lobe, nlabels)
    assert np.array_equal(by_alignment, ref) and np.array_equal(vec, ref)
    assert np.array_equal(by_alignment, vec)
    moved = vec.copy()
    moved[4, 2] += 1
    moved[4, 5] += 1
    assert np.array_equal(by_width, moved)


# ------------------------------------------------------------------------------------------------ crop -> R^3
def run_chunks(scan, lobe, chunks, R):
    D, H, W = scan.shape
    out = torch.full((len(chunks), R, R, R), float("nan"), dtype=torch.float32, device=DEV)
    scan_d, lobe_d = dev(scan), dev(lobe)
    call("dram_lobe_chunks", scan_d.data_ptr(), lobe_d.data_ptr(), out.data_ptr(), chunk_array(chunks), len(chunks), D, H, W,
         R, K.WINDOW[0], K.WINDOW[1])
    return out.cpu().numpy()


def check_chunks(got, ref, what):
    """Absolute 1e-5 on values in [0, 1]: the tolerance of tests/test_gpu_inference.py::
    test_crop_resampling_grid_follows_the_itk_call for the same kernel against the same oracle function."""
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    err = np.abs(got.astype(np.float64) - ref)
    print(f"infer-kernel-accuracy: lobe_chunks {what}: max err {err.max():.3e} (bound 1e-5)")
    assert err.max() <= 1e-5, (what, np.unravel_index(err.argmax(), err.shape))


@pytest.mark.parametrize("constant_scan", [False, True], ids=["random_scan", "scan_at_window_max"])
def test_lobe_chunks_three_chunks_at_nonzero_origins(constant_scan):
    """Volume (14, 37, 45), R = 12 (1728 outputs: six full blocks and 192), L = 3 in one call: A upsampled along z and
    downsampled along y and x, with a checkerboard of its label and a foreign one in its box; B overlapping A's box with
    another label; C four voxels along x, so output column 11 holds the default value 0.  The scan has values below, inside
    and above the window, or is constant at the window maximum: then chunk A is the resampled checkerboard itself."""
    scan, lobe = K.chunk_volume(constant_scan)
    ref = K.lobe_chunks_ref(scan, lobe, K.CHUNKS_ABC, K.CHUNK_R, K.WINDOW)
    got = run_chunks(scan, lobe, K.CHUNKS_ABC, K.CHUNK_R)
    check_chunks(got, ref, "A, B, C")
    assert (got[2][:, :, 11] == 0).all() and (got[2][:, :, 10] != 0).any()
    if constant_scan:
        assert got[0, 0, 0, 0] == 1.0 and 0.3 < got[0].mean() < 0.7 and got[0].std() > 0.1


def test_lobe_chunks_eight_chunks_keep_their_slots():
    """L = MAX_CHUNKS = 8 distinct chunks: slot l of the output belongs to chunk l (the reference slots differ pairwise by
    more than 0.1 somewhere: tests/test_infer_kernels_cpu.py)."""
    scan, lobe = K.chunk_volume()
    ref = K.lobe_chunks_ref(scan, lobe, K.CHUNKS_8, K.CHUNK_R, K.WINDOW)
    check_chunks(run_chunks(scan, lobe, K.CHUNKS_8, K.CHUNK_R), ref, "8 chunks")


# ------------------------------------------------------------------------------------------------ paste
def test_lobe_paste_values_and_untouched_voxels():
    """Volume (14, 37, 45), R = 6, L = 3, dense = 4 * randn; boxes (5, 20, 31) -- 3100 voxels: a grid tail of 28 --, (9, 7, 2)
    overlapping it, and one with a single plane along z.  htp starts as a sentinel pattern of distinct negative numbers.
    Bit for bit: every voxel outside all boxes, and every voxel inside a box whose label is not that chunk's, still holds
    its sentinel.  Every voxel with lobe == label in a box was written, and holds its own label's value also where two
    boxes overlap: |got - ref| <= 16 * 2^-24 against the fp64 restatement (derivation at infer_kernel_cases.PASTE_TOL: 4 ulp
    for the fp32 sigmoid, assuming expf within 2 ulp, and 11 roundings of the combination, on values below 1)."""
    dense, lobe, htp0 = K.paste_inputs()
    ref, written = K.lobe_paste_ref(dense, lobe, K.PASTE_CHUNKS, K.PASTE_R, htp0)
    D, H, W = K.VOLUME
    dense_d, lobe_d, htp_d = dev(dense), dev(lobe), dev(htp0)
    call("dram_lobe_paste", dense_d.data_ptr(), lobe_d.data_ptr(), htp_d.data_ptr(), chunk_array(K.PASTE_CHUNKS),
         len(K.PASTE_CHUNKS), D, H, W, K.PASTE_R)
    got = htp_d.cpu().numpy()
    assert np.array_equal(got[~written], htp0[~written])                       # untouched, bit for bit
    assert (got[written] > 0).all()                                            # written: no sentinel left
    err = np.abs(got.astype(np.float64) - ref)
    worst = np.unravel_index(err.argmax(), err.shape)
    print(f"infer-kernel-accuracy: lobe_paste: max err {err.max():.3e} at {worst} (bound {K.PASTE_TOL:.3e})")
    assert err.max() <= K.PASTE_TOL, (err.max(), worst)
    p, q = K.PASTE_CHUNKS[:2]
    both = tuple(slice(max(p[k], q[k]), min(p[k] + p[k + 3], q[k] + q[k + 3])) for k in range(3))
    for l, c in enumerate((p, q)):                                             # in the overlap each voxel holds its own label's value
        sel = lobe[both] == c[6]
        alone, _ = K.lobe_paste_ref(dense[l:l + 1], lobe, (c,), K.PASTE_R, htp0)   # this chunk pasted on its own
        assert sel.any() and np.abs(got[both][sel].astype(np.float64) - alone[both][sel]).max() <= K.PASTE_TOL


# ------------------------------------------------------------------------------------------------ lung histogram
def run_lung_hist(htp, lobe):
    hist = torch.full((256,), -7, dtype=torch.int64, device=DEV)
    ssum = torch.full((1,), float("nan"), dtype=torch.float64, device=DEV)
    htp_d, lobe_d = dev(htp), dev(lobe)
    call("dram_lung_hist256", htp_d.data_ptr(), lobe_d.data_ptr(), hist.data_ptr(), ssum.data_ptr(), htp.size)
    return hist.cpu().numpy(), float(ssum.item())


def check_lung_hist(what, htp, lobe, check_sum=True):
    """Counts bit for bit, count == hist.sum(), and the fp64 sum within count * 2^-53 * sum |htp| of the exactly rounded
    reference sum (the device adds its fp64 partials in an unspecified order: infer_kernel_cases.hist_sum_bound)."""
    ref_hist, ref_sum, sum_abs, count = K.lung_hist_ref(htp, lobe)
    hist, ssum = run_lung_hist(htp, lobe)
    assert np.array_equal(hist, ref_hist), (what, np.flatnonzero(hist != ref_hist)[:8])
    assert int(hist.sum()) == count
    if check_sum:
        bound = K.hist_sum_bound(count, sum_abs)
        print(f"infer-kernel-accuracy: lung_hist256 {what}: |sum - ref| {abs(ssum - ref_sum):.3e} (bound {bound:.3e}, sum {ref_sum:.6e})")
        assert abs(ssum - ref_sum) <= bound, (what, ssum, ref_sum)
    return ssum


def test_lung_hist_bin_edges():
    """n = 256 * 16 + 77: for every k the fp32 k / 255 and its two neighbours, -0.0, a negative value, 1.0, its upper
    neighbour, 7.5 and +inf, the rest uniform; about 40 % of the voxels outside the lungs.  With +inf the sum is +inf; the
    bounded sum check runs on a copy that holds 0.5 there.

    NaN is not part of the input: lung_hist_kernel puts a NaN voxel into bin 0 (HIP's fmaxf(NaN, 0) is 0) and the NaN
    poisons the sum, while the reference's np.uint8(cam * 255) of a NaN is platform-defined; no reference is asserted."""
    htp, lobe, inf_at = K.bin_edge_input()
    assert check_lung_hist("bin edges, with +inf", htp, lobe, check_sum=False) == float("inf")
    finite = htp.copy()
    finite[inf_at] = 0.5
    check_lung_hist("bin edges", finite, lobe)


def test_lung_hist_past_the_grid_cap():
    """n = 2048 * 256 * 16 + 4099: the grid is capped at 2048 blocks, every thread walks 16 voxels and the first 4099 a
    seventeenth; the last 4099 voxels are all inside the lungs."""
    check_lung_hist("past the cap", K.past_cap_htp(), K.past_cap_lobe())


def test_lung_hist_one_voxel_outside_the_lungs():
    hist, ssum = run_lung_hist(np.array([0.75], dtype=np.float32), np.array([0], dtype=np.uint8))
    assert not hist.any() and ssum == 0.0


# ------------------------------------------------------------------------------------------------ threshold
def test_threshold_mask_is_strict_past_the_grid_cap():
    """n = 4096 * 256 + 300 with th = float32(128 / 255): th itself and the value below give 0, the value above 1, NaN 0 --
    in the first block, in the middle and in the 300 voxels past the 4096-block cap."""
    htp = K.threshold_input()
    mask = torch.full((htp.size,), 0xAB, dtype=torch.uint8, device=DEV)
    htp_d = dev(htp)
    call("dram_threshold_mask", htp_d.data_ptr(), mask.data_ptr(), float(K.THRESHOLD), htp.size)
    got = mask.cpu().numpy()
    ref = K.threshold_ref(htp, K.THRESHOLD).astype(np.uint8)
    assert np.array_equal(got, ref), np.flatnonzero(got != ref)[:8]
    # the threshold handed over as the fp64 128 / 255 (what LobeInference passes): rounded to fp32 at the C boundary
    mask.fill_(0xAB)
    call("dram_threshold_mask", htp_d.data_ptr(), mask.data_ptr(), 128 / 255, htp.size)
    assert np.array_equal(mask.cpu().numpy(), ref)


# ------------------------------------------------------------------------------------------------ the counting kernels
def test_scan_hist_past_the_grid_cap():
    """dram_scan_hist256 at n = 2048 * 256 * 16 + 4099 against np.bincount of the oracle's 8-bit view (windowing with the
    default span, then binary_cam's windowing to 0..255 and truncation): bit for bit."""
    scan, lobe = K.past_cap_scan(), K.past_cap_lobe()
    hist = torch.full((256,), -7, dtype=torch.int64, device=DEV)
    scan_d, lobe_d = dev(scan), dev(lobe)
    call("dram_scan_hist256", scan_d.data_ptr(), lobe_d.data_ptr(), hist.data_ptr(), K.POST_WINDOW[0], K.POST_WINDOW[1], scan.size)
    got, ref = hist.cpu().numpy(), K.scan_hist_ref(scan, lobe)
    assert np.array_equal(got, ref), np.flatnonzero(got != ref)[:8]
    assert int(got.sum()) == int((lobe > 0).sum())


def test_mask_overlap_past_the_grid_cap():
    """dram_mask_overlap at n = 2048 * 256 * 16 + 4099 on masks whose set voxels hold 1, 7 or 255: intersection, union and the
    two sizes against numpy's logical counts."""
    a, b = K.past_cap_masks()
    counts = torch.full((4,), -7, dtype=torch.int64, device=DEV)
    a_d, b_d = dev(a), dev(b)
    call("dram_mask_overlap", a_d.data_ptr(), b_d.data_ptr(), counts.data_ptr(), a.size)
    assert counts.cpu().numpy().tolist() == K.mask_overlap_ref(a, b).tolist()
