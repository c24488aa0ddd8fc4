"""Inputs and host restatements of tests/test_gpu_cam_kernels.py and tests/test_gpu_cam_inference.py (checked against torch's
CPU ops and the oracle by tests/test_cam_cpu.py).  Host code only: numpy on the CPU.

The lobe-wise class head of the reference's inference entry point, LesionSegTest.run (job_runner.py:985-1004), restated
plainly from those lines, from pooling_dense_features (models.py:37-49) and from ATen's published align-corners rule -- not
from the kernels of csrc/infer_cam.hip:
    t_lobe_chunk = nearest-neighbour resample of (lobe == label) on the crop -> R^3 grid          chunk_mask_ref
    pool = (dense * mask).sum() / mask.sum() per channel                                            pool_ref
    cls = torch.max(pool, dim=-1)[-1]: first occurrence of the maximum, a NaN counts as the maximum  argmax_ref
    dense = relu(F.interpolate(dense, crop_size, 'trilinear', align_corners=True))[cls]
    dense = dense / dense.max()  (over the crop box);  zero when cls == 0;  paste where lobe == label   cam_ref
Integer and mask results are compared bit for bit; the float tolerances are derived at max_tol / quotient_tol."""
import numpy as np

import infer_kernel_cases as K

U = K.U                               # unit roundoff of fp32
VOLUME = K.VOLUME                     # (14, 37, 45)
MAX_CHUNKS = K.MAX_CHUNKS
RS = (6, 12)
# the constants of csrc/infer_cam.hip that the shapes are sized against
CAM_MAX_BLOCK_VOXELS = 256 * 8        # lobe_cam_max: voxels per block of 256 threads and grid step (below its grid cap)

#             z0  y0  x0  dz  dy  dx  label
CHUNKS_8 = (K.PASTE_CHUNKS[0],               # 0: (5, 20, 31) = 3100 voxels: 12 blocks of 256 + 28; two blocks of lobe_cam_max
            K.PASTE_CHUNKS[1],               # 1: overlaps box 0 with another label; 2 voxels along x < R
            K.PASTE_CHUNKS[2],               # 2: one plane along z: scale 0 on the way back, 1 voxel < R on the way in
            (0, 0, 0, 14, 8, 9, 4),          # 3: the whole depth from the origin; overlaps box 2 (labels 3 / 4)
            (2, 30, 1, 6, 7, 25, 1),         # 4: label 1 again, away from box 0
            (8, 12, 40, 6, 20, 5, 2),        # 5: up to the last column
            (0, 31, 27, 3, 6, 18, 3),        # 6: up to the last row
            (9, 30, 28, 5, 7, 12, 4))        # 7: up to the last plane and row
CHUNKS_1 = CHUNKS_8[:1]
PLANTED_LAST = 0                      # the class's channel peaks at the LAST voxel of the box, which is outside the lobe
PLANTED_OUTSIDE = 4                   # the box maximum lies at a voxel that does not carry the chunk's label
CLS0 = 1                              # pool row whose maximum is channel 0: zeros over the sentinel
NON_POSITIVE = 2                      # the class's channel is <= 0 everywhere: 0 / 0 = NaN
TIE = 3                               # pool row [1, 3, 3, 2, 3, 0]: class 1
NAN_ROW = 5                           # pool row [1, 7, nan, 9, nan, 2]: class 2
TIE_WITH_0 = 6                        # pool row [5, 5, 5, -1, 5, 5]: class 0
SENTINEL_PEAK = 9.0


def overlap(p, q):
    return all(max(p[k], q[k]) < min(p[k] + p[k + 3], q[k] + q[k + 3]) for k in range(3))


# ------------------------------------------------------------------------------------------------ the resampled lobe mask
def fixed_size_nearest_axis(n_in, n_out):
    """One axis of Resample('fixed_size') with interpolator='nearest' (data_transforms.py:170-187 -> utils.resample): output
    voxel o sits at the continuous input index c = o * n_in / n_out (the grid of the image chunk, oracle.resample_itk_linear),
    is inside the buffer while c < n_in - 0.5 and then takes voxel floor(c + 0.5) (ITK: RoundHalfIntegerUp).  fp64."""
    c = np.arange(n_out, dtype=np.float64) * float(n_in) / float(n_out)
    return np.minimum((c + 0.5).astype(np.int64), n_in - 1), c < n_in - 0.5


def chunk_mask_ref(lobe, chunks, R):
    """(L, R, R, R) float32 of 0 / 1: t_lobe_chunk of every chunk; 0 (ITK's default value) outside the crop's buffer."""
    out = np.zeros((len(chunks), R, R, R), dtype=np.float32)
    for l, c in enumerate(chunks):
        binary = lobe[K.box(c)] == c[6]
        (iz, okz), (iy, oky), (ix, okx) = (fixed_size_nearest_axis(c[3 + a], R) for a in range(3))
        ok = okz[:, None, None] & oky[None, :, None] & okx[None, None, :]
        out[l] = np.where(ok, binary[np.ix_(iz, iy, ix)], False)
    return out


def pool_ref(dense, mask):
    """models.py:45-47 in fp64: (dense * mask).sum() / mask.sum() per (chunk, channel); mask (L, R, R, R)."""
    d, m = dense.astype(np.float64), mask.astype(np.float64)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        return (d * m).reshape(d.shape[0], d.shape[1], -1).sum(-1) / np.broadcast_to(m, d.shape).reshape(d.shape[0], d.shape[1], -1).sum(-1)


# ------------------------------------------------------------------------------------------------ class and heat map
def argmax_ref(row):
    """torch.max(row, dim=-1)[-1] on the CPU, from ATen's published kernel: a value replaces the running maximum when it is
    not <= it and the scan stops at a NaN -- the first occurrence of the maximum wins, and the first NaN beats everything."""
    best, idx = row[0], 0
    for k, v in enumerate(row):
        if not v <= best:
            best, idx = v, k
            if v != v:
                break
    return idx


def ac_axis(n_in, n_out, dtype=np.float32):
    """ATen's align-corners source index of one axis (area_pixel_compute_scale, compute_source_index_and_lambda), evaluated
    in `dtype`: fp32 is what ATen does for float tensors (and the kernels), fp64 what it does for double tensors.
    Returns (i0, i1, l0, l1) with the weights as the numbers of that type that they are."""
    scale = dtype(n_in - 1) / dtype(n_out - 1) if n_out > 1 else dtype(0.0)
    src = scale * np.arange(n_out, dtype=dtype)
    assert src.dtype == dtype
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0.astype(dtype)
    l0 = dtype(1.0) - l1
    assert l0.dtype == dtype
    return i0, i1, l0, l1


def trilinear_ac_ref(vol, size, dtype=np.float32):
    """vol (R, R, R) -> size, trilinear with align_corners: index rule in `dtype`, the 8-term combination in fp64."""
    vol = vol.astype(np.float64)
    (z0, z1, a0, a1), (y0, y1, b0, b1), (x0, x1, c0, c1) = (ac_axis(vol.shape[a], size[a], dtype) for a in range(3))
    a0, a1 = a0.astype(np.float64)[:, None, None], a1.astype(np.float64)[:, None, None]
    b0, b1 = b0.astype(np.float64)[None, :, None], b1.astype(np.float64)[None, :, None]
    c0, c1 = c0.astype(np.float64)[None, None, :], c1.astype(np.float64)[None, None, :]
    at = lambda z, y, x: vol[np.ix_(z, y, x)]
    return (a0 * (b0 * (c0 * at(z0, y0, x0) + c1 * at(z0, y0, x1)) + b1 * (c0 * at(z0, y1, x0) + c1 * at(z0, y1, x1))) +
            a1 * (b0 * (c0 * at(z1, y0, x0) + c1 * at(z1, y0, x1)) + b1 * (c0 * at(z1, y1, x0) + c1 * at(z1, y1, x1))))


def cam_chunk_ref(dense_l, cls, size, dtype=np.float32):
    """job_runner.py:993-1000 for one lobe: (the normalised map over the crop box, its maximum before the division, the
    ReLU'd map before the division).  Resize, ReLU, select, max, divide (0 / 0 = NaN, as torch), zero when cls == 0.
    (Selecting the channel first is the same thing: the resize and the ReLU act per channel.)"""
    relu = np.maximum(trilinear_ac_ref(dense_l[cls], size, dtype), 0.0)
    mx = relu.max()
    with np.errstate(invalid="ignore", divide="ignore"):
        out = relu / mx
    if cls == 0:
        out = np.zeros_like(out)
    return out, mx, relu


def cam_ref(dense, pool, lobe, chunks, R, htp0, dtype=np.float32):
    """(htp float64, written bool, cls list, max list, tol float64): a copy of htp0 with every chunk's normalised map
    written where lobe == label inside its box, the chunks in order; tol holds quotient_tol at every written voxel."""
    htp = htp0.astype(np.float64).copy()
    written = np.zeros(htp.shape, dtype=bool)
    tol = np.zeros(htp.shape, dtype=np.float64)
    clss, maxs = [], []
    for l, c in enumerate(chunks):
        assert dense[l].shape[1:] == (R, R, R)
        cls = argmax_ref(pool[l])
        out, mx, relu = cam_chunk_ref(dense[l], cls, c[3:6], dtype)
        sel = lobe[K.box(c)] == c[6]
        htp[K.box(c)][sel] = out[sel]
        written[K.box(c)][sel] = True
        t = quotient_tol(relu, mx, np.abs(dense[l, cls]).max()) if cls != 0 and mx > 0 else np.zeros_like(relu)
        tol[K.box(c)][sel] = t[sel]
        clss.append(cls)
        maxs.append(mx)
    return htp, written, clss, maxs, tol


# ------------------------------------------------------------------------------------------------ tolerances (derived, not measured)
def max_tol(dense_abs_max):
    """|device relu(resize(x))(v) - restatement|: both sides share the fp32 index rule and weights, the restatement combines
    in fp64, the device in fp32 with 8 products and 7 adds = 15 roundings, each at most u = 2^-24 relative to a partial result
    that the convex weights keep within max |x| (PASTE_TOL's argument, with the values no longer confined to [0, 1]); ReLU and
    the maximum over voxels are 1-Lipschitz, so the same bound holds for the box maximum.  Rounded up to 16 u max |x| for the
    second-order terms."""
    return 16 * U * float(dense_abs_max)


def quotient_tol(v, m, dense_abs_max):
    """|device v / m - restatement| with both v and m carrying max_tol (d): first order (dv + (v / m) dm) / m, the denominator
    taken at m - d so that the bound holds for the device's own m, plus the one rounding of the fp32 division, u (v / m) <= u."""
    d = max_tol(dense_abs_max)
    assert m > 1e3 * d, "the maximum has to stand clear of its own error"
    return (d + (v / m) * d) / (m - d) + U


# ------------------------------------------------------------------------------------------------ the whole scan
DENSE_TOL = 1e-4                      # tests/test_gpu_inference.py: the model's output through the device path against the oracle
MIN_GAP = 100 * DENSE_TOL             # top-2 gap of every pool row that the class-level test asks of its inputs


def scan_tol(v, m, dense_abs_max):
    """quotient_tol with the model's own error in place of the interpolation's: the dense output agrees with the oracle's to
    d = DENSE_TOL * max(1, max |dense|) (the bound tests/test_gpu_inference.py holds the same models to), the resize is a convex
    combination and ReLU and max are 1-Lipschitz, so v and m both carry d (+ max_tol for the resize itself)."""
    d = DENSE_TOL * max(1.0, float(dense_abs_max)) + max_tol(dense_abs_max)
    assert m > 1e2 * d, "the maximum has to stand clear of its own error"
    return (d + (v / m) * d) / (m - d) + U


def cam_scan_ref(forward, scan, lobe, spacing, R, window=K.WINDOW, border=5.0):
    """LesionSegTest.run's loop over the lobes (job_runner.py:954-1004) with the oracle's pieces for everything up to the
    model -- find_crops, mask to -2048, windowing, resample_itk_linear, as O.evaluate_scan has them -- `forward(image, mask) ->
    dense [1, C, R, R, R]` (torch, CPU) for the model, and the restatement above for the head.  Every label of the map is
    visited.  Returns (htp float64, tol float64, {label: cls}, {label: pool row}, {label: max |dense|})."""
    import torch
    from oracle import dram_oracle as O
    htp = np.zeros(scan.shape, dtype=np.float64)
    tol = np.zeros(scan.shape, dtype=np.float64)
    clss, pools, absmax = {}, {}, {}
    for label in (int(v) for v in np.unique(lobe)[1:]):
        sl = O.find_crops(lobe == label, spacing, border)
        chunk = tuple(s.start for s in sl) + tuple(s.stop - s.start for s in sl) + (label,)
        lobe_chunk = lobe[sl] == label
        scan_chunk = scan[sl].astype(np.float32).copy()
        scan_chunk[~lobe_chunk] = -2048
        img = O.windowing(scan_chunk, from_span=window, to_span=(0.0, 1.0)).astype(np.float32)
        mask = chunk_mask_ref(lobe, (chunk,), R)
        with torch.no_grad():
            dense = forward(torch.from_numpy(O.resample_itk_linear(img, (R,) * 3))[None, None],
                            torch.from_numpy(mask)[None]).numpy()
        pool = pool_ref(dense, mask)[0]
        cls = argmax_ref(pool)
        out, mx, relu = cam_chunk_ref(dense[0], cls, chunk[3:6])
        htp[sl][lobe_chunk] = out[lobe_chunk]
        if cls != 0:
            tol[sl][lobe_chunk] = scan_tol(relu, mx, np.abs(dense[0]).max())[lobe_chunk]
        clss[label], pools[label], absmax[label] = cls, pool, float(np.abs(dense[0]).max())
    return htp, tol, clss, pools, absmax


# ------------------------------------------------------------------------------------------------ inputs of the kernel tests
def pool_rows(C, L):
    """pool (L, C) float32 fed to lobe_cam_max directly: random rows with the planted ones (C = 6)."""
    g = K.rng(72)
    pool = g.standard_normal((L, C)).astype(np.float32)
    if C == 6:
        pool[PLANTED_LAST % L] = [0.5, -1.0, 0.25, 2.0, 1.0, -3.0]          # class 3
        if L == MAX_CHUNKS:
            pool[PLANTED_OUTSIDE] = [-2.0, -1.0, -0.5, -4.0, -0.75, -0.25]  # class 5, all negative
            pool[CLS0] = [4.0, 1.0, 3.0, -2.0, 0.0, 3.5]
            pool[NON_POSITIVE] = [0.0, 1.0, 6.0, 2.0, 3.0, 4.0]             # class 2
            pool[TIE] = [1.0, 3.0, 3.0, 2.0, 3.0, 0.0]
            pool[NAN_ROW] = [1.0, 7.0, np.nan, 9.0, np.nan, 2.0]
            pool[TIE_WITH_0] = [5.0, 5.0, 5.0, -1.0, 5.0, 5.0]
    elif L == MAX_CHUNKS:
        pool[NAN_ROW] = np.nan                                              # C = 1: still class 0
    return pool


def kernel_inputs(R, C, L):
    """dense (L, C, R, R, R) = 4 * randn; lobe: random labels 0..4 everywhere (about a fifth of every box carries the chunk's
    label, and both labels occur in an overlap); htp0: K.paste_inputs' sentinel of distinct negative numbers; pool rows as
    above.  Planted in the class's channel (C = 6):
      chunk 0  dense[R-1, R-1, R-1] = 9: with align_corners the last voxel of the box IS that corner, so the box maximum is 9
               at the last voxel of the last partial block; that voxel's label is set to a foreign one
      chunk 4  the voxel where the class's map peaks is given a foreign label
      chunk 2  the class's channel is -|x|: every value of its map is <= 0."""
    chunks = CHUNKS_8 if L == MAX_CHUNKS else CHUNKS_1
    assert len(chunks) == L
    g = K.rng(71 + R)
    dense = (4.0 * g.standard_normal((L, C, R, R, R))).astype(np.float32)
    lobe = g.integers(0, 5, size=VOLUME).astype(np.uint8)
    pool = pool_rows(C, L)
    cls = [argmax_ref(pool[l]) for l in range(L)]
    c0 = chunks[PLANTED_LAST]
    dense[PLANTED_LAST, cls[PLANTED_LAST], R - 1, R - 1, R - 1] = SENTINEL_PEAK
    last = tuple(c0[a] + c0[a + 3] - 1 for a in range(3))
    lobe[last] = (c0[6] + 1) % 5
    if L == MAX_CHUNKS:
        dense[NON_POSITIVE, cls[NON_POSITIVE]] = -np.abs(dense[NON_POSITIVE, cls[NON_POSITIVE]])
        c4 = chunks[PLANTED_OUTSIDE]
        relu = cam_chunk_ref(dense[PLANTED_OUTSIDE], cls[PLANTED_OUTSIDE], c4[3:6])[2]
        peak = np.unravel_index(int(relu.argmax()), relu.shape)
        lobe[tuple(c4[a] + peak[a] for a in range(3))] = 0
    n = int(np.prod(VOLUME))
    htp0 = -(1.0 + np.arange(n, dtype=np.float32)).reshape(VOLUME)
    return chunks, dense, pool, lobe, htp0
