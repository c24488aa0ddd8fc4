"""The lesion density report restated in plain numpy, int64 throughout: the definition that csrc/density.hip and
dram_amd/density.py are held against bit for bit.  Itself held against scipy.ndimage and np.percentile by
tests/test_density_cpu.py."""
import numpy as np

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def _selected(scan, labels, n, mask):
    scan = np.asarray(scan).reshape(-1).astype(np.int64)
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    sel = (lab >= 1) & (lab <= n)
    if mask is not None:
        sel &= np.asarray(mask).reshape(-1) != 0
    return scan[sel], lab[sel] - 1


def moments(scan, labels, n, mask=None):
    """(count, sum, sumsq) int64 [n] and (min, max) int32 [n] over the voxels with 1 <= label <= n (and mask != 0); a label
    without voxels has 0, 0, 0, 32767, -32768."""
    v, k = _selected(scan, labels, n, mask)
    count = np.bincount(k, minlength=n).astype(np.int64)
    total, sumsq = np.zeros(n, np.int64), np.zeros(n, np.int64)
    np.add.at(total, k, v)
    np.add.at(sumsq, k, v * v)
    vmin, vmax = np.full(n, 32767, np.int64), np.full(n, -32768, np.int64)
    np.minimum.at(vmin, k, v)
    np.maximum.at(vmax, k, v)
    return count, total, sumsq, vmin.astype(np.int32), vmax.astype(np.int32)


def bin_of(v, lo, width, nbins):
    """Entry 0: v < lo; 1 + (v - lo) // width inside the range; nbins + 1 at or above lo + nbins * width."""
    v = np.asarray(v, dtype=np.int64)
    inside = 1 + (np.maximum(v - lo, 0) // max(width, 1))
    return np.where(v < lo, 0, np.where(v < lo + nbins * width, inside, nbins + 1)).astype(np.int64)


def histogram(scan, labels, n, lo, width, nbins, mask=None):
    """int64 [n, nbins + 2]."""
    v, k = _selected(scan, labels, n, mask)
    hist = np.zeros((n, nbins + 2), np.int64)
    np.add.at(hist, (k, bin_of(v, lo, width, nbins)), 1)
    return hist


def rank_of(q_permille, count):
    """The nearest rank, 1-based, in Python integers: max(1, ceil(q * count / 1000))."""
    return max(1, (int(q_permille) * int(count) + 999) // 1000)


def percentile_of_values(x, q_permille):
    """The nearest-rank percentile of a non-empty array: np.sort(x)[rank - 1]."""
    x = np.sort(np.asarray(x).reshape(-1))
    return int(x[rank_of(q_permille, x.size) - 1])


def summary(hist, lo, width, nbins, q_permille=(), edges=()):
    """(pct int32 [n, nq], bands int64 [n, ne + 1]) of histogram rows: the percentile is the lower edge of the first in-range bin
    at which the running count reaches the rank, INT32_MIN when that happens in the underflow entry, INT32_MAX when only in the
    overflow entry or for an empty row; band i sums the entries whose values lie in [edges[i-1], edges[i])."""
    hist = np.asarray(hist, dtype=np.int64)
    n = hist.shape[0]
    pct = np.zeros((n, len(q_permille)), np.int32)
    bands = np.zeros((n, len(edges) + 1), np.int64)
    lower = lo + width * np.arange(nbins, dtype=np.int64)                 # the lower edge of in-range bin b = 1 .. nbins
    band_of = np.zeros(nbins + 2, np.int64)
    band_of[1:nbins + 1] = np.searchsorted(np.asarray(edges, dtype=np.int64), lower, side="right")
    band_of[nbins + 1] = len(edges)
    for k in range(n):
        run = np.cumsum(hist[k])
        c = int(run[-1])
        for i, q in enumerate(q_permille):
            if c == 0:
                pct[k, i] = INT32_MAX
                continue
            e = int(np.searchsorted(run, rank_of(q, c), side="left"))      # the first entry with run >= rank
            pct[k, i] = INT32_MIN if e == 0 else (INT32_MAX if e == nbins + 1 else lo + (e - 1) * width)
        np.add.at(bands[k], band_of, hist[k])
    return pct, bands


def report_from_tables(count, total, sumsq, vmin, vmax, pct, bands):
    """mean = sum / count (fp64), std = sqrt((count * sumsq - sum^2) / count^2) with the numerator in Python integers, the band
    fractions; NaN for an empty label."""
    n = len(count)
    mean, std = np.full(n, np.nan), np.full(n, np.nan)
    fraction = np.full(np.shape(bands), np.nan)
    for k in range(n):
        c, s, q = int(count[k]), int(total[k]), int(sumsq[k])
        if c:
            mean[k] = s / c
            std[k] = float(np.sqrt(np.float64((c * q - s * s) / (c * c))))
            fraction[k] = np.asarray(bands[k], dtype=np.float64) / np.float64(c)
    return {"voxels": np.asarray(count, np.int64), "mean_hu": mean, "std_hu": std, "min_hu": np.asarray(vmin, np.int32),
            "max_hu": np.asarray(vmax, np.int32), "percentiles_hu": np.asarray(pct, np.int32),
            "band_voxels": np.asarray(bands, np.int64), "band_fraction": fraction}


def label_report(scan, labels, n, mask=None, percentiles_permille=(150, 500, 850), band_edges_hu=(-950, -750, -300),
                 hist_range=(-1024, 1, 4096)):
    lo, width, nbins = hist_range
    if n == 0:
        return report_from_tables(*(np.zeros(0, np.int64),) * 3, np.zeros(0, np.int32), np.zeros(0, np.int32),
                                  np.zeros((0, len(percentiles_permille)), np.int32), np.zeros((0, len(band_edges_hu) + 1), np.int64))
    pct, bands = summary(histogram(scan, labels, n, lo, width, nbins, mask), lo, width, nbins, percentiles_permille, band_edges_hu)
    return report_from_tables(*moments(scan, labels, n, mask), pct, bands)


def lesion_density(scan, kept_labels, n_kept, kept_mask, lobe, **kw):
    """The `density` entry of lesion_report: the kept components, and per lobe label present the whole lobe and its voxels
    inside the kept mask."""
    present = [int(v) for v in np.unique(lobe) if v != 0]
    lobes = {}
    if present:
        top = max(present)
        whole, inside = label_report(scan, lobe, top, **kw), label_report(scan, lobe, top, mask=kept_mask, **kw)
        row = lambda rep, k: {key: v[k] for key, v in rep.items()}
        lobes = {v: {"parenchyma": row(whole, v - 1), "lesion": row(inside, v - 1)} for v in present}
    return {"lesions": label_report(scan, kept_labels, n_kept, **kw), "lobes": lobes}
