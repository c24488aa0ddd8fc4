"""fp64 restatement of the pseudo-vessel mask (csrc/vessel.hip, dram_amd/vessels.py) over scipy.ndimage and numpy.linalg: the
oracle of tests/test_gpu_vessel.py, itself held against scipy.ndimage.gaussian_filter and analytic anchors by
tests/test_vessel_cpu.py.  The definition is in include/dram_hip.h (dram_hessian ...)."""
import numpy as np
from scipy import ndimage

ORDER = ("zz", "yy", "xx", "zy", "zx", "yx")
# per output the filter order along (z, y, x)
ORDERS = {"zz": (2, 0, 0), "yy": (0, 2, 0), "xx": (0, 0, 2), "zy": (1, 1, 0), "zx": (1, 0, 1), "yx": (0, 1, 1)}
AXES = {"zz": (0, 0), "yy": (1, 1), "xx": (2, 2), "zy": (0, 1), "zx": (0, 2), "yx": (1, 2)}


def radius_of(sigma):
    return int(4.0 * float(sigma) + 0.5)


def scipy_taps(sigma, order):
    """The impulse response of scipy.ndimage.gaussian_filter1d(order=...) at truncate = 4.0: 2 r + 1 values, offsets -r .. r."""
    r = radius_of(sigma)
    delta = np.zeros(2 * r + 1)
    delta[r] = 1.0
    return ndimage.gaussian_filter1d(delta, sigma, order=order, mode="constant", cval=0.0, truncate=4.0)


def tap_table(sv, taps_of=scipy_taps, rounded=True):
    """{(axis, order): impulse response, as float64}; rounded: through fp32, as the device table is."""
    out = {}
    for a in range(3):
        for o in range(3):
            t = np.asarray(taps_of(sv[a], o), dtype=np.float64)
            out[a, o] = t.astype(np.float32).astype(np.float64) if rounded else t
    return out


def clamp(scan, clip):
    v = np.asarray(scan).astype(np.float32).astype(np.float64)
    return v if clip is None else np.clip(v, float(clip[0]), float(clip[1]))


def hessian(scan, sv, clip=None, table=None, scaled=True):
    """[6,D,H,W] float64: per output correlate1d along x, y, z with the REVERSED impulse response (gaussian_filter1d reverses its
    weights before it correlates; this matters for order 1), mode 'reflect', origin 0; times sv[a] * sv[b]."""
    table = tap_table(sv) if table is None else table
    v = clamp(scan, clip)
    out = np.empty((6,) + v.shape)
    for k, name in enumerate(ORDER):
        t = v
        for axis in (2, 1, 0):
            t = ndimage.correlate1d(t, table[axis, ORDERS[name][axis]][::-1], axis=axis, mode="reflect", origin=0)
        a, b = AXES[name]
        out[k] = t * np.float64(np.float32(sv[a] * sv[b])) if scaled else t
    return out


def matrices(h6):
    h6 = np.asarray(h6, dtype=np.float64)
    m = np.empty(h6.shape[1:] + (3, 3))
    m[..., 0, 0], m[..., 1, 1], m[..., 2, 2] = h6[0], h6[1], h6[2]
    m[..., 0, 1] = m[..., 1, 0] = h6[3]
    m[..., 0, 2] = m[..., 2, 0] = h6[4]
    m[..., 1, 2] = m[..., 2, 1] = h6[5]
    return m


def sort_by_magnitude(ev):
    """ev ascending along the last axis -> by ascending magnitude, ties by ascending value (a stable argsort)."""
    idx = np.argsort(np.abs(ev), axis=-1, kind="stable")
    return np.take_along_axis(ev, idx, axis=-1)


def eigenvalues(h6):
    """[3, ...]: l1, l2, l3."""
    return np.moveaxis(sort_by_magnitude(np.linalg.eigvalsh(matrices(h6))), -1, 0)


def tube_measure(l, alpha=0.5, beta=0.5, c=1.0):
    """V in fp64 from l = [3, ...]; exactly 0 when l2 >= 0, l3 >= 0 or the expression is not finite."""
    l1, l2, l3 = (np.asarray(x, dtype=np.float64) for x in l)
    c = np.float64(c)
    with np.errstate(all="ignore"):
        ra = np.abs(l2) / np.abs(l3)
        rb = np.abs(l1) / np.sqrt(np.abs(l2 * l3))
        s2 = l1 * l1 + l2 * l2 + l3 * l3
        v = -np.expm1(-(ra * ra) / (2.0 * alpha * alpha)) * np.exp(-(rb * rb) / (2.0 * beta * beta)) * -np.expm1(-s2 / (2.0 * c * c))
    return np.where((l2 >= 0.0) | (l3 >= 0.0) | ~np.isfinite(v), 0.0, v)


def frobenius32(h6):
    """The Frobenius norm per voxel: fp64 from the fp32 entries, rounded to fp32."""
    zz, yy, xx, zy, zx, yx = (np.asarray(h6[k], dtype=np.float32).astype(np.float64) for k in range(6))
    return np.sqrt(zz * zz + yy * yy + xx * xx + 2.0 * (zy * zy + zx * zx + yx * yx)).astype(np.float32)


def frangi_c(h6, lobe=None):
    """Half the largest norm over lobe > 0 (all voxels without a lobe map); 1 for a zero maximum.  float32."""
    n = frobenius32(h6)
    if lobe is not None:
        n = n[np.asarray(lobe) > 0]
    m = np.float32(n.max()) if n.size else np.float32(0.0)
    return np.float32(1.0) if m == 0 else np.float32(0.5) * m


def vesselness(scan, spacing, sigmas_mm=(1.0, 1.5, 2.0, 3.0), alpha=0.5, beta=0.5, c=None, clip=(-1150.0, 350.0), lobe=None):
    """float64 [D,H,W]: the maximum over scales of V.  c=None: per scale frangi_c of the Hessian rounded to fp32."""
    vmax = None
    for s in sigmas_mm:
        sv = [float(s) / float(sp) for sp in spacing]
        h6 = hessian(scan, sv, clip)
        cs = frangi_c(h6.astype(np.float32), lobe) if c is None else np.float32(c)
        v = tube_measure(eigenvalues(h6), alpha, beta, cs)
        vmax = v if vmax is None else np.maximum(vmax, v)
    return vmax


def mask(vmax, lobe, threshold):
    return ((vmax >= threshold) & (np.asarray(lobe) > 0)).astype(np.uint8)
