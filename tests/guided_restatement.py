"""An fp64 numpy restatement of the masked 3-D guided filter as include/dram_hip.h defines it ("heat-map refinement"): direct
window sums, the region applied with np.where (never as a product), steps 2 and 3 as written there.  Held against scipy's
uniform_filter and analytic anchors by tests/test_guided_cpu.py; the device is held against it by tests/test_gpu_guided.py."""
import numpy as np


def guide_values(guide, window):
    """g in fp64: an int16 scan is windowed, g = clip((hu - lo) / (hi - lo), 0, 1); anything else is taken as it is."""
    guide = np.asarray(guide)
    if guide.dtype == np.int16:
        lo, hi = float(window[0]), float(window[1])
        return np.clip((guide.astype(np.float64) - lo) / (hi - lo), 0.0, 1.0)
    return guide.astype(np.float64)


def window_sum(v, radius):
    """out[c] = the sum of v over the box c +- radius cut at the volume's edge: per axis x, then y, then z a direct sum over the
    offsets -r .. r in ascending order."""
    out = np.asarray(v, dtype=np.float64)
    for axis in (2, 1, 0):
        r, n = int(radius[axis]), out.shape[axis]
        acc = np.zeros_like(out)
        for j in range(-r, r + 1):
            if abs(j) >= n:
                continue
            dst = [slice(None)] * 3
            src = [slice(None)] * 3
            dst[axis] = slice(max(0, -j), n - max(0, j))          # c with 0 <= c + j < n
            src[axis] = slice(max(0, j), n - max(0, -j))          # c + j
            acc[tuple(dst)] += out[tuple(src)]
        out = acc
    return out


def guided_filter(guide, p, mask, radius, eps, window=None):
    """dict: q64 (the fp64 value of step 3 before its rounding, 0 outside M), q (float32), a, b (step 2, 0 outside M), n."""
    m = np.asarray(mask) != 0
    with np.errstate(invalid="ignore", over="ignore"):
        g_all = guide_values(guide, window)
        g = np.where(m, g_all, 0.0)
        pp = np.where(m, np.asarray(p).astype(np.float64), 0.0)
    n = window_sum(m.astype(np.float64), radius)
    sg, sp, sgg, sgp = (window_sum(f, radius) for f in (g, pp, g * g, g * pp))
    nn = np.where(m, n, 1.0)                                      # N >= 1 on M; elsewhere nothing below is read
    mg, mp = sg / nn, sp / nn
    a = (sgp / nn - mg * mp) / ((sgg / nn - mg * mg) + float(eps))
    b = mp - a * mg
    a, b = np.where(m, a, 0.0), np.where(m, b, 0.0)
    A, B = window_sum(a, radius) / nn, window_sum(b, radius) / nn
    q64 = np.where(m, A * g + B, 0.0)
    return {"q64": q64, "q": q64.astype(np.float32), "a": a, "b": b, "n": n}
