"""Inputs and host restatements of tests/test_gpu_infer_kernels.py (checked against the oracle and torch's CPU ops by
tests/test_infer_kernels_cpu.py).  Host code only: numpy and torch on the CPU.

The kernels of csrc/infer.hip around the model call of LobeInference -- label_bboxes, lobe_chunks, lobe_paste, lung_hist256,
threshold_mask -- and the two counting kernels of the post-processing tail -- scan_hist256, mask_overlap -- each get a plain
restatement here, written from the reference's formulas (evaluate_scan, job_runner.py:729-770; find_crops / binary_cam,
utils.py:226-254) and from ATen's published align-corners rule, not from the kernels.  Integer and comparison work is checked
bit for bit; the two float results have the tolerances derived at PASTE_TOL and hist_sum_bound below."""
import functools
import math

import numpy as np

from oracle import dram_oracle as O

INT_MAX = 0x7fffffff
U = 2.0 ** -24                       # unit roundoff of fp32

# the constants of csrc/infer.hip that the shapes are sized against
BBOX_ROWS = 64                       # rows per block of label_bboxes_kernel
MAX_CHUNKS = 8                       # chunks per lobe_chunks / lobe_paste call
HIST_GRID_CAP = 2048 * 256 * 16      # lung_hist256, scan_hist256, mask_overlap: <= 2048 blocks x 256 threads x 16 voxels
THRESHOLD_GRID_CAP = 4096 * 256      # threshold_mask (and lesion_post): <= 4096 blocks of 256
N_PAST_HIST_CAP = HIST_GRID_CAP + 4099
N_PAST_THRESHOLD_CAP = THRESHOLD_GRID_CAP + 300

VOLUME = (14, 37, 45)                # H != W and neither a multiple of anything
WINDOW = (-1000.0, -300.0)


def rng(seed):
    return np.random.default_rng(seed)


# ------------------------------------------------------------------------------------------------ bounding boxes
def bboxes_ref(lobe, nlabels):
    """(nlabels, 6) int32: min z, y, x and max z, y, x (inclusive) of every label 1..nlabels; (INT_MAX x 3, -1 x 3) for an
    absent label (csrc/infer.hip: "min > max when the label is absent")."""
    out = np.empty((nlabels, 6), dtype=np.int32)
    out[:, :3], out[:, 3:] = INT_MAX, -1
    for label in range(1, nlabels + 1):
        idx = np.argwhere(lobe == label)
        if len(idx):
            out[label - 1, :3], out[label - 1, 3:] = idx.min(0), idx.max(0)
    return out


def crop_from_box(box, shape, spacing, border):
    """The border-and-clamp arithmetic of LobeInference.run on one row of bboxes_ref -> (start, size) per axis."""
    start, size = [], []
    for lo, hi, n, sp in zip(box[:3], box[3:], shape, spacing):
        pad = int(math.ceil(border / sp)) if border > 0 else 0
        a, b = max(0, int(lo) - pad), min(n, int(hi) + 1 + pad)
        start.append(a)
        size.append(b - a)
    return start, size


def bbox_band_map(W, extra_labels=False):
    """(3, 70, W) for W >= 32.  H = 70: two bands of 64 + 6 rows.
      label 1  a solid block over rows 60..67: both bands
      label 2  row (0, 10): 16 voxels at x = 16..31 (one uniform group of the vector path) preceded by the mixed group
               [0, 2, 2, 6, 0, 2, 0, 0, 6, 2, 2, 2, 0, 0, 2, 0] at x = 0..15 (label 6 there: label 5 has to stay one voxel)
      label 3  rows 66..69 only: the second band only
      label 4  one voxel at (0, 0, 0)
      label 5  one voxel at (D-1, H-1, W-1): the last element of the last band
    extra_labels: also labels 7 and 200 (above nlabels = 6), 200 both as a uniform group of 16 and inside a mixed group, 7 at
    the far end of a row, all OUTSIDE the other labels' boxes so that counting them would widen a box; and label 6 (the last
    one that nlabels = 6 tracks) as a uniform group of 16 as well."""
    D, H = 3, 70
    m = np.zeros((D, H, W), dtype=np.uint8)
    m[1, 60:68, 4:12] = 1
    m[0, 10, 0:16] = [0, 2, 2, 6, 0, 2, 0, 0, 6, 2, 2, 2, 0, 0, 2, 0]
    m[0, 10, 16:32] = 2
    m[2, 66:70, 20:25] = 3
    m[0, 0, 0] = 4
    m[D - 1, H - 1, W - 1] = 5
    if extra_labels:
        m[2, 30, 16:32] = 200
        m[1, 40, 16:32] = 6                                                           # label == nlabels as a uniform group
        m[1, 5, 0:16] = [200, 0, 7, 0, 0, 200, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]      # label 1's box grows to row 5, x = 15
        m[0, 69, W - 1] = 7
    return m


def bbox_interleaved_map(W):
    """One row alternating 17 / 40 (as tests/test_gpu_inference.py::test_lobe_inference_arbitrary_labels has it): every
    voxel of a group of 16 is another label than its neighbour."""
    m = np.zeros((2, 3, W), dtype=np.uint8)
    m[1, 1, 0:W:2] = 17
    m[1, 1, 1:W:2] = 40
    return m


# id -> map; "misaligned" is built by the GPU test from "vector" (a view one byte into a larger buffer)
BBOX_MAPS = {
    "vector": lambda extra: bbox_band_map(32, extra),
    "scalar_by_width": lambda extra: bbox_band_map(33, extra),
    "interleaved_vector": lambda extra: _with_extra(bbox_interleaved_map(48), extra),
    "interleaved_scalar": lambda extra: _with_extra(bbox_interleaved_map(44), extra),
    "empty": lambda extra: np.zeros((2, 70, 32), dtype=np.uint8),
}
# (nlabels, whether the map also holds labels 7 and 200)
BBOX_NLABELS = ((255, False), (6, True))


def _with_extra(m, extra):
    if extra:
        m[0, 0, 0], m[0, 2, 5] = 7, 200
        m[0, 1, 3] = 2
    return m


# ------------------------------------------------------------------------------------------------ crop -> R^3
CHUNK_R = 12                          # R^3 = 1728: not a multiple of 256
#            z0  y0  x0  dz  dy  dx  label
CHUNKS_ABC = ((2, 3, 5, 7, 25, 30, 1),      # A: upsampled along z (7 -> 12), downsampled along y and x
              (6, 20, 25, 8, 15, 18, 2),    # B: overlaps A's box (z 6..8, y 20..27, x 25..34), another label
              (1, 30, 40, 5, 6, 4, 3))      # C: 4 voxels along x < R: output column 11 (c = 3.67 >= 3.5) is the default 0
CHUNKS_8 = tuple((l + 1, 2 * l + 1, 3 * l + 2, 3 + l % 3, 4 + l % 4, 5 + l % 5, (1, 4)[l % 2]) for l in range(MAX_CHUNKS))   # (labels 1 / 4: box A's checkerboard)


def chunk_volume(constant_scan=False):
    """scan (int16) with values below, inside and above WINDOW -- or constant at the window maximum -- and a lobe map of
    random labels 0..3 with a checkerboard of label 1 and the foreign label 4 inside box A."""
    g = rng(21)
    scan = g.integers(-1400, 100, size=VOLUME).astype(np.int16)
    if constant_scan:
        scan[:] = int(WINDOW[1])
    lobe = g.integers(0, 4, size=VOLUME).astype(np.uint8)
    z0, y0, x0, dz, dy, dx, _ = CHUNKS_ABC[0]
    zz, yy, xx = np.meshgrid(np.arange(dz), np.arange(dy), np.arange(dx), indexing="ij")
    lobe[z0:z0 + dz, y0:y0 + dy, x0:x0 + dx] = np.where((zz + yy + xx) % 2 == 0, 1, 4)
    return scan, lobe


def box(c):
    return tuple(slice(c[a], c[a] + c[a + 3]) for a in range(3))


def lobe_chunks_ref(scan, lobe, chunks, R, window):
    """(L, R, R, R) float32: per chunk, crop the box, put the window minimum where lobe != label (the reference writes
    -2048 HU, which clips to it), window to [0, 1] in fp32 as csrc/infer.hip documents -- (clip(v) - wmin) * (1 / (wmax -
    wmin)) --, then the oracle's resample_itk_linear to R^3."""
    wmin, wmax = np.float32(window[0]), np.float32(window[1])
    inv = np.float32(1.0) / (wmax - wmin)
    out = np.empty((len(chunks), R, R, R), dtype=np.float32)
    for l, c in enumerate(chunks):
        v = scan[box(c)].astype(np.float32)
        v[lobe[box(c)] != c[6]] = wmin
        img = (np.clip(v, wmin, wmax) - wmin) * inv
        assert img.dtype == np.float32
        out[l] = O.resample_itk_linear(img, (R, R, R))
    return out


# ------------------------------------------------------------------------------------------------ paste
PASTE_R = 6
PASTE_CHUNKS = ((3, 10, 8, 5, 20, 31, 1),      # 3100 voxels: 12 blocks of 256 + 28
                (1, 25, 30, 9, 7, 2, 2),       # overlaps the first box in z 3..7, y 25..29, x 30..31
                (12, 2, 3, 1, 9, 11, 3))       # one plane along z: scale 0
# sigmoid in fp32 (expf within 2 ulp, one add, one divide: about 4 ulp) + 8 products and 7 adds of values in [0, 1] whose
# weights sum to 1 (11 roundings), each ulp <= 2^-24 on values below 1; rounded up to a power of two
PASTE_TOL = 16 * U


def paste_inputs():
    """dense (3, R, R, R) = 4 * randn: sigmoid spans (0, 1) with steep gradients; lobe: random labels 0..4 everywhere, so
    about a fifth of every box carries the chunk's label and both labels occur in the overlap; htp0: a sentinel pattern of
    distinct negative integers (a pasted value lies in (0, 1))."""
    g = rng(31)
    dense = (4.0 * g.standard_normal((len(PASTE_CHUNKS), PASTE_R, PASTE_R, PASTE_R))).astype(np.float32)
    lobe = g.integers(0, 5, size=VOLUME).astype(np.uint8)
    n = int(np.prod(VOLUME))
    htp0 = -(1.0 + np.arange(n, dtype=np.float32)).reshape(VOLUME)
    return dense, lobe, htp0


def ac_axis(n_in, n_out):
    """ATen's align-corners source index of one axis, in fp32 as ATen evaluates it for float tensors
    (area_pixel_compute_scale, compute_source_index_and_lambda): scale = (in - 1) / (out - 1) or 0 when out == 1,
    src = scale * o, i0 = int(src) clamped to the last element, i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1.
    Returns (i0, i1, l0, l1), the weights as the fp32 numbers they are."""
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0.0)
    src = scale * np.arange(n_out, dtype=np.float32)
    assert src.dtype == np.float32
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0.astype(np.float32)
    l0 = np.float32(1.0) - l1
    assert l0.dtype == np.float32
    return i0, i1, l0, l1


def trilinear_ac_ref(vol, size):
    """vol (R, R, R) float64 -> size, trilinear with align_corners: fp32 index rule (ac_axis), the 8-term combination in fp64."""
    (z0, z1, a0, a1), (y0, y1, b0, b1), (x0, x1, c0, c1) = (ac_axis(vol.shape[a], size[a]) for a in range(3))
    a0, a1 = a0.astype(np.float64)[:, None, None], a1.astype(np.float64)[:, None, None]
    b0, b1 = b0.astype(np.float64)[None, :, None], b1.astype(np.float64)[None, :, None]
    c0, c1 = c0.astype(np.float64)[None, None, :], c1.astype(np.float64)[None, None, :]
    at = lambda z, y, x: vol[np.ix_(z, y, x)]
    return (a0 * (b0 * (c0 * at(z0, y0, x0) + c1 * at(z0, y0, x1)) + b1 * (c0 * at(z0, y1, x0) + c1 * at(z0, y1, x1))) +
            a1 * (b0 * (c0 * at(z1, y0, x0) + c1 * at(z1, y0, x1)) + b1 * (c0 * at(z1, y1, x0) + c1 * at(z1, y1, x1))))


def lobe_paste_ref(dense, lobe, chunks, R, htp0):
    """(htp float64, written bool): a copy of htp0 with interp(sigmoid(dense[l])) written where lobe == label inside chunk
    l's box (job_runner.py:765-770), the chunks in order; sigmoid and the combination in fp64."""
    htp = htp0.astype(np.float64).copy()
    written = np.zeros(htp.shape, dtype=bool)
    for l, c in enumerate(chunks):
        assert dense[l].shape == (R, R, R)
        probs = trilinear_ac_ref(1.0 / (1.0 + np.exp(-dense[l].astype(np.float64))), c[3:6])
        sel = lobe[box(c)] == c[6]
        htp[box(c)][sel] = probs[sel]
        written[box(c)][sel] = True
    return htp, written


# ------------------------------------------------------------------------------------------------ lung histogram
def lung_hist_ref(htp, lobe):
    """binary_cam's 8-bit view of the heat map inside the lungs (utils.py:233) as fp32 operations: bin = int(float32(clip(v,
    0, 1)) * float32(255)).  Returns (hist int64[256], the exactly rounded fp64 sum of htp over lobe > 0, sum |htp| there,
    the voxel count)."""
    v = htp[lobe > 0]
    prod = np.clip(v, 0, 1).astype(np.float32) * np.float32(255)
    assert prod.dtype == np.float32
    hist = np.bincount(prod.astype(np.int64), minlength=256).astype(np.int64)
    assert hist.shape == (256,)
    v64 = v.astype(np.float64)
    return hist, math.fsum(v64), math.fsum(np.abs(v64)), int(v.size)


def hist_sum_bound(count, sum_abs):
    """The device adds `count` fp64 terms in an unspecified order: at most `count` roundings of 2^-53 relative to a partial
    sum that never exceeds sum |htp|."""
    return count * 2.0 ** -53 * sum_abs


def f32_neighbours(v):
    v = np.float32(v)
    return np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))


HIST_EXTRAS = (-0.0, -0.25, 1.0, float(np.nextafter(np.float32(1), np.float32(2))), 7.5, float("inf"))
N_BIN_EDGES = 256 * 16 + 77


def bin_edge_input():
    """n = 256 * 16 + 77.  For every k in 0..255 the fp32 k / 255 and its two fp32 neighbours (positions 3k .. 3k + 2), then
    HIST_EXTRAS, the rest uniform in [0, 1); the order is then shuffled.  lobe: random 0 / 1..5 with about 40 % zeros, except
    that of the planted values only every fourth is outside the lungs and none of the extras.  Returns (htp, lobe, position of
    +inf)."""
    g = rng(41)
    n = N_BIN_EDGES
    planted = [x for k in range(256) for x in f32_neighbours(np.float32(k) / np.float32(255))]
    planted += [np.float32(x) for x in HIST_EXTRAS]
    htp = g.random(n, dtype=np.float32)
    htp[:len(planted)] = planted
    lobe = np.where(g.random(n) < 0.4, 0, g.integers(1, 6, size=n)).astype(np.uint8)
    idx = np.arange(len(planted))
    lobe[:len(planted)] = np.where(idx % 4 == 3, 0, 1 + idx % 5)
    lobe[len(planted) - len(HIST_EXTRAS):len(planted)] = 3
    perm = g.permutation(n)
    htp, lobe = htp[perm], lobe[perm]
    inf_at = int(np.flatnonzero(np.isinf(htp))[0])
    return htp, lobe, inf_at


@functools.lru_cache(maxsize=None)
def past_cap_lobe():
    """uint8[N_PAST_HIST_CAP]: 1..5 for the last 4099 voxels and for about half of the others, else 0."""
    g = rng(42)
    n = N_PAST_HIST_CAP
    lobe = np.where(g.random(n) < 0.5, 0, g.integers(1, 6, size=n)).astype(np.uint8)
    lobe[-4099:] = g.integers(1, 6, size=4099)
    lobe.setflags(write=False)
    return lobe


@functools.lru_cache(maxsize=None)
def past_cap_htp():
    htp = rng(43).random(N_PAST_HIST_CAP, dtype=np.float32)
    htp.setflags(write=False)
    return htp


# ------------------------------------------------------------------------------------------------ threshold
THRESHOLD = np.float32(128) / np.float32(255)


def threshold_ref(htp, th):
    return htp > np.float32(th)


def threshold_input():
    """n = 4096 * 256 + 300 uniform values with th, its two fp32 neighbours and NaN planted in the first block, in the middle
    and in the tail past the grid cap."""
    n = N_PAST_THRESHOLD_CAP
    htp = rng(51).random(n, dtype=np.float32)
    special = list(f32_neighbours(THRESHOLD)) + [np.float32("nan")]
    for start in (0, 517 * 256 + 3, THRESHOLD_GRID_CAP + 1, n - 4):
        htp[start:start + 4] = special
    return htp


# ------------------------------------------------------------------------------------------------ the counting kernels of the tail
POST_WINDOW = (-1150, 350)


def scan_hist_ref(scan, lobe, window=POST_WINDOW):
    """The 8-bit histogram LesionSegTest.run's brightness gate is built on, with the oracle's own steps:
    O.lesion_post_process windows the scan with O.windowing and O.binary_cam takes the 8-bit view of that."""
    w_scan = O.windowing(scan[lobe > 0], from_span=window, to_span=(0, 1))
    view8 = O.windowing(w_scan, from_span=(0, 1), to_span=(0, 255)).astype(np.uint8)
    return np.bincount(view8, minlength=256).astype(np.int64)


@functools.lru_cache(maxsize=None)
def past_cap_scan():
    scan = rng(61).integers(-1400, 600, size=N_PAST_HIST_CAP).astype(np.int16)
    scan.setflags(write=False)
    return scan


def past_cap_masks():
    """Two uint8 masks whose set voxels hold 1, 7 or 255 (non-zero = set), the last 4099 voxels of both set."""
    g = rng(62)
    n = N_PAST_HIST_CAP
    vals = np.array([0, 0, 1, 7, 255], dtype=np.uint8)
    a, b = vals[g.integers(0, 5, size=n)], vals[g.integers(0, 5, size=n)]
    a[-4099:], b[-4099:] = 1, 255
    return a, b


def mask_overlap_ref(a, b):
    x, y = a > 0, b > 0
    return np.array([np.logical_and(x, y).sum(), np.logical_or(x, y).sum(), x.sum(), y.sum()], dtype=np.int64)
