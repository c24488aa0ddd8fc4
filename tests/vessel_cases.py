"""Inputs, derived tolerances and the numpy mirror of the device's eigen-solver for tests/test_vessel_cpu.py and
tests/test_gpu_vessel.py.  Everything is generated from seeds; nothing here touches the GPU."""
import functools

import numpy as np

import vessel_restatement as VR

# tile constants of csrc/vessel.hip
VX_T = 256          # x pass: outputs along x per block
VX_ROWS = 4         # x pass: rows per block
VA_TX = 64          # axis passes: columns per block
VA_LT = 64          # axis passes: outputs along the filtered axis per block
MAX_RADIUS = 32     # dram_vessel_max_radius()
JACOBI_SWEEPS = 5   # VES_JACOBI_SWEEPS of csrc/vessel_device.h

# name: (shape, sv (z, y, x) in voxels, dtype, clip).  Each pass needs two tiles and a ragged tail along its filtered axis and
# along one other axis:  x pass: W = 2 * 256 + 3 and 2 * 4 + 1 rows;  y pass: H = W = 2 * 64 + 3;  z pass: D = 2 * 64 + 3 and
# H * W = 3 * 47 = 2 * 64 + 13 columns.  "short": the y axis (9) is shorter than its radius (12).  "cap": radius 32 along y.
HESSIAN_CASES = {
    "x_tiles_D1": ((1, 9, 515), (0.6, 1.1, 2.3), np.int16, (-1150.0, 350.0)),
    "y_tiles": ((2, 131, 131), (0.8, 2.9, 1.3), np.float32, None),
    "z_tiles": ((131, 3, 47), (2.3, 0.7, 1.4), np.int16, None),
    "short": ((5, 9, 33), (0.8, 2.9, 1.3), np.float32, (-1150.0, 350.0)),
    "cap": ((3, 70, 40), (1.0, 8.0, 0.3), np.int16, (-1150.0, 350.0)),
    "radius0": ((4, 6, 10), (0.1, 0.12, 0.11), np.float32, None),
}


@functools.lru_cache(maxsize=None)
def hessian_input(name):
    shape, _, dtype, _ = HESSIAN_CASES[name]
    rng = np.random.default_rng(sorted(HESSIAN_CASES).index(name) + 11)
    v = rng.uniform(-2000.0, 1500.0, size=shape)               # values on both sides of the clip window
    v = np.rint(v).astype(np.int16) if dtype == np.int16 else v.astype(np.float32)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def hessian_expected(name):
    _, sv, _, clip = HESSIAN_CASES[name]
    h = VR.hessian(hessian_input(name), sv, clip)
    h.setflags(write=False)
    return h


def hessian_bound(sv, max_abs):
    """The derived error bound of every output of dram_hessian against the fp64 restatement on the same fp32 taps, [6]:
        k * 2^-24 * prod over the axes of sum|taps| * max|I| * fl(sv[a] * sv[b])
    k counts the fp32 roundings on the output's path: per pass the tap count 2 r + 1 plus one (the kernel pairs the taps: one
    rounded sum or difference and one fused multiply-add per distance, one product for the centre: 2 r + 1, no more), plus one
    for the final scaling.  The last factor is the scaling itself: it multiplies the value and its error alike."""
    table = VR.tap_table(sv)
    out = []
    for name in VR.ORDER:
        k, amp = 1, 1.0
        for axis in range(3):
            t = table[axis, VR.ORDERS[name][axis]]
            k += len(t) + 1
            amp *= np.abs(t).sum()
        a, b = VR.AXES[name]
        out.append(k * 2.0 ** -24 * amp * max_abs * float(np.float32(sv[a] * sv[b])))
    return np.array(out)


def max_abs_input(name):
    _, _, _, clip = HESSIAN_CASES[name]
    return float(np.abs(VR.clamp(hessian_input(name), clip)).max())


# ---- hand-made Hessians for dram_vesselness ----

def _rot(axis, deg):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    r = np.eye(3)
    i, j = [(1, 2), (0, 2), (0, 1)][axis]
    r[i, i], r[i, j], r[j, i], r[j, j] = c, -s, s, c
    return r


def _h6(m):
    return [m[0, 0], m[1, 1], m[2, 2], m[0, 1], m[0, 2], m[1, 2]]


VESSELNESS_C = 20.0
VESSELNESS_COUNT = 2 * 256 + 37          # two blocks of 256 voxels and a ragged tail


@functools.lru_cache(maxsize=None)
def vesselness_h6():
    """[6, VESSELNESS_COUNT] float32.  Diagonal, two equal, all equal, zero, l2 / l3 positive, equal magnitudes of opposite sign,
    known rotations of diag(-1, -50, -60) and of a two-equal matrix, each also at 1e-3 and 1e4 times the size; the rest of the
    two blocks and the tail are seeded random rotations of random diagonals."""
    diags = [(-1, -50, -60), (-60, -1, -50), (3, -2, -2.5), (-5, -5, -1), (-2, -2, -2), (0, 0, 0), (1, 5, -7), (1, 5, 7),
             (-1, 5, -7), (2, -2, -3), (-3, 3, -3), (0, -4, -4), (0, 0, -1), (7, -50, -60)]
    mats = [np.diag(np.array(d, dtype=np.float64)) for d in diags]
    base = np.diag([-1.0, -50.0, -60.0])
    rots = [_rot(0, 30), _rot(1, 45), _rot(2, 60), _rot(0, 90), _rot(2, 20) @ _rot(1, 35), _rot(0, 10) @ _rot(1, 80) @ _rot(2, 55)]
    mats += [r @ base @ r.T for r in rots]
    mats += [r @ np.diag([-1.0, -50.0, -50.0]) @ r.T for r in rots[:3]]
    mats = mats + [m * 1e-3 for m in mats] + [m * 1e4 for m in mats]
    rng = np.random.default_rng(5)
    while len(mats) < VESSELNESS_COUNT:
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        d = rng.normal(size=3) * rng.choice([1.0, 30.0, 300.0])
        if rng.random() < 0.5:
            d = -np.abs(d)
        mats.append(q @ np.diag(d) @ q.T)
    h = np.array([_h6(m) for m in mats[:VESSELNESS_COUNT]], dtype=np.float64).T.astype(np.float32)
    h = np.ascontiguousarray(h)
    h[:, -1] = np.float32(3e4) * np.array(_h6(rots[4] @ base @ rots[4].T), dtype=np.float32)   # the largest norm: the last ragged element
    h.setflags(write=False)
    return h


NORM_MAX_CAP = 4096 * 256                # voxels of one lap of hessian_norm_max_kernel at its grid cap
NORM_MAX_S = NORM_MAX_CAP + 300
NORM_MAX_FIRST_LAP, NORM_MAX_SECOND_LAP = 777_777, NORM_MAX_CAP + 123


@functools.lru_cache(maxsize=None)
def norm_max_large():
    """(h6 [6, NORM_MAX_S] float32, {variant: lobe or None}): seeded Hessians of modest size, the largest norm of all planted in
    the second lap of the grid-stride loop and the second largest in the first.  Variants: no lobe map; a lobe map that holds
    the planted voxel of the second lap; one that leaves it out (and everything near it), so that the maximum is the first
    lap's."""
    rng = np.random.default_rng(8)
    h = rng.normal(size=(6, NORM_MAX_S)).astype(np.float32) * np.float32(3.0)
    h[:, NORM_MAX_SECOND_LAP] = np.array([100, -200, 150, 50, -75, 25], dtype=np.float32)
    h[:, NORM_MAX_FIRST_LAP] = np.array([-60, 90, 30, -45, 20, 10], dtype=np.float32)
    inside = (rng.random(NORM_MAX_S) < 0.5).astype(np.uint8) * rng.integers(1, 6, size=NORM_MAX_S).astype(np.uint8)
    inside[[NORM_MAX_FIRST_LAP, NORM_MAX_SECOND_LAP]] = 2
    outside = inside.copy()
    outside[NORM_MAX_SECOND_LAP - 40:NORM_MAX_SECOND_LAP + 40] = 0
    for a in (h, inside, outside):
        a.setflags(write=False)
    return h, {"no_lobe": None, "lobe_holds_the_maximum": inside, "lobe_leaves_it_out": outside}


def _jacobi_rotate(app, aqq, apq, arp, arq):
    """csrc/vessel_device.h: jacobi_rotate, operation for operation, on arrays."""
    with np.errstate(all="ignore"):
        act = apq != 0.0
        theta = (aqq - app) / (2.0 * np.where(act, apq, 1.0))
        t = np.copysign(1.0, theta) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
        c = 1.0 / np.sqrt(t * t + 1.0)
        s = t * c
        return (np.where(act, app - t * apq, app), np.where(act, aqq + t * apq, aqq), np.zeros_like(apq),
                np.where(act, c * arp - s * arq, arp), np.where(act, s * arp + c * arq, arq))


def jacobi_eigenvalues(h6, sweeps=JACOBI_SWEEPS):
    """The device's solver in numpy fp64: [3, n] by ascending magnitude, ties by value."""
    a00, a11, a22, a01, a02, a12 = (np.asarray(h6[k], dtype=np.float32).astype(np.float64) for k in range(6))
    for _ in range(sweeps):
        a00, a11, a01, a02, a12 = _jacobi_rotate(a00, a11, a01, a02, a12)
        a00, a22, a02, a01, a12 = _jacobi_rotate(a00, a22, a02, a01, a12)
        a11, a22, a12, a01, a02 = _jacobi_rotate(a11, a22, a12, a01, a02)
    ev = np.sort(np.stack([a00, a11, a22], axis=-1), axis=-1)
    return np.moveaxis(VR.sort_by_magnitude(ev), -1, 0)


def eig_scale(h6):
    """Per matrix the size its eigenvalue errors are measured against: the Frobenius norm (1 for the zero matrix)."""
    n = VR.frobenius32(h6).astype(np.float64)
    return np.where(n == 0, 1.0, n)


def measured_solver_error(h6):
    """max over the matrices of |jacobi - eigvalsh| / scale, eigenvalues compared in ascending order (a swap of two nearly
    equal magnitudes is no error of the solver)."""
    ours = np.sort(jacobi_eigenvalues(h6), axis=0)
    ref = np.sort(VR.eigenvalues(np.asarray(h6, dtype=np.float32).astype(np.float64)), axis=0)
    return float((np.abs(ours - ref).max(axis=0) / eig_scale(h6)).max())


# Measured on the CPU over vesselness_h6() by measured_solver_error: 9.7e-16 (test_vessel_cpu.py re-measures it); the device may
# differ from numpy by a few ulp per sqrt and division, hence the margin of 4.
EIG_TOLERANCE = 4 * 9.7e-16

# ---- end to end ----

E2E_SHAPE = (40, 48, 56)
E2E_SPACING = (1.0, 0.7, 0.7)
E2E_SIGMAS = (1.0, 1.5, 2.0, 3.0)
E2E_CLIP = (-1150.0, 350.0)
E2E_C_GIVEN = 60.0


@functools.lru_cache(maxsize=None)
def e2e_volume():
    """(scan int16, lobe uint8): lung-like background at -850 HU with noise of +-30 HU, two crossing bright tubes of different
    radii, a sheet, a blob; the lobe map is two boxes, the first touching the z = 0 face."""
    D, H, W = E2E_SHAPE
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    zm, ym, xm = z * E2E_SPACING[0], y * E2E_SPACING[1], x * E2E_SPACING[2]
    v = np.full(E2E_SHAPE, -850.0)
    # tube along x at (z, y) = (14, 15) mm, Gaussian profile of 1.2 mm; tube along (z, y) diagonal crossing it, 2 mm
    v += 800.0 * np.exp(-((zm - 14.0) ** 2 + (ym - 15.0) ** 2) / (2 * 1.2 ** 2))
    d2 = ((zm - 14.0) - (ym - 15.0)) ** 2 / 2.0 + (xm - 20.0) ** 2
    v += 700.0 * np.exp(-d2 / (2 * 2.0 ** 2))
    v += 600.0 * np.exp(-(zm - 30.0) ** 2 / (2 * 1.5 ** 2)) * (ym > 18.0)                      # a sheet
    v += 700.0 * np.exp(-((zm - 22.0) ** 2 + (ym - 27.0) ** 2 + (xm - 31.0) ** 2) / (2 * 2.5 ** 2))   # a blob
    v += np.random.default_rng(21).uniform(-30.0, 30.0, size=E2E_SHAPE)
    scan = np.rint(np.minimum(v, 200.0)).astype(np.int16)
    lobe = np.zeros(E2E_SHAPE, dtype=np.uint8)
    lobe[0:26, 6:40, 5:30] = 1
    lobe[8:36, 10:44, 30:52] = 2
    scan.setflags(write=False)
    lobe.setflags(write=False)
    return scan, lobe


def e2e_bound(sigma_mm):
    sv = [sigma_mm / s for s in E2E_SPACING]
    return hessian_bound(sv, max(abs(E2E_CLIP[0]), abs(E2E_CLIP[1])))


@functools.lru_cache(maxsize=None)
def e2e_hessians():
    scan, _ = e2e_volume()
    out = tuple(VR.hessian(scan, [s / sp for sp in E2E_SPACING], E2E_CLIP) for s in E2E_SIGMAS)
    for h in out:
        h.setflags(write=False)
    return out


def e2e_vesselness(c, lobe_for_c, perturb=None):
    """The restatement's vmax from the cached Hessians; perturb: a Generator -> every entry of H moves by its derived bound
    with a random sign (and Frangi's c with it)."""
    vmax = None
    for s, h in zip(E2E_SIGMAS, e2e_hessians()):
        if perturb is not None:
            h = h + perturb.choice([-1.0, 1.0], size=h.shape) * e2e_bound(s)[:, None, None, None]
        cs = VR.frangi_c(h.astype(np.float32), lobe_for_c) if c is None else np.float32(c)
        v = VR.tube_measure(VR.eigenvalues(h), 0.5, 0.5, cs)
        vmax = v if vmax is None else np.maximum(vmax, v)
    return vmax


def measured_e2e_tolerance(c, lobe_for_c, trials=4):
    """The largest change of V under `trials` random-sign perturbations of H by its bound, times 2 for the eigen-solver and the
    fp32 rounding of V."""
    ref = e2e_vesselness(c, lobe_for_c)
    rng = np.random.default_rng(3)
    return 2.0 * max(float(np.abs(e2e_vesselness(c, lobe_for_c, rng) - ref).max()) for _ in range(trials))


# Measured on the CPU by measured_e2e_tolerance(None, lobe): 0.05995 (test_vessel_cpu.py re-measures it).  It is this large
# because Frangi's V is not continuous: where l1 > 0 > l2 have nearly the same magnitude, a change of H far below the bound swaps
# them, l2 turns positive and V drops to exactly 0 -- from up to 0.03 here.  The largest change over the volume is such a voxel.
E2E_TOLERANCE = 0.0600
# the reference's V lies within E2E_TOLERANCE of it on 86 of the 43044 lobe voxels (0.2 %), 82 voxels are set
MASK_THRESHOLD = 0.5

# ---- bounding box: a lobe map whose box touches the z = 0, y = 0 and x = 0 faces and stays clear of the opposite ones by more
#      than the largest radius (z 12, y and x 17 at 3 mm) ----


def bbox_lobe():
    lobe = np.zeros(E2E_SHAPE, dtype=np.uint8)
    lobe[0:14, 0:12, 0:21] = 3
    lobe[5:10, 4:9, 10:19] = 1
    return lobe
