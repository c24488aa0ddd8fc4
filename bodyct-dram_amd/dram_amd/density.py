"""Lesion density report on the device: the Hounsfield statistics of every lesion and every lobe -- voxel count, mean, standard
deviation, minimum, maximum, percentiles and the share of a few density bands -- without pulling the int16 scan and a label
volume back to the host for `scipy.ndimage.sum_labels / minimum / maximum / histogram`.

    rep = label_report(scan, lobe, 5)                       # the lobes' parenchyma: mean lung density, Perc15, share below -950 HU
    rep = lesion_report(mask, lobe, spacing, scan=scan)     # lesions.lesion_report with a `density` entry

Kernels: csrc/density.hip (one pass over scan and labels for the exact integer moments and a histogram per label; the
histograms' percentiles and band counts).  Only O(labels) numbers travel to the host, where mean and standard deviation are
formed from the exact integers.
"""
import numpy as np
import torch

from ._lib import call
from .surface import _device_u8, _stream

# The default bands: below -950 HU (low attenuation, "emphysema-like"), [-950, -750) (normally aerated), [-750, -300) (ground-glass
# range), at or above -300 (consolidation range).
BAND_NAMES = ("laa", "aerated", "ggo", "consolidation")
BAND_EDGES_HU = (-950, -750, -300)
PERCENTILES_PERMILLE = (150, 500, 850)
HIST_RANGE = (-1024, 1, 4096)


def _scan_and_labels(scan, labels, mask, who):
    scan = torch.as_tensor(scan)
    if scan.dtype != torch.int16:
        raise ValueError(f"{who}: the scan must be int16 (Hounsfield units)")
    labels = torch.as_tensor(labels)
    if labels.dtype not in (torch.uint8, torch.int32):
        raise ValueError(f"{who}: labels must be uint8 or int32")
    if scan.shape != labels.shape:
        raise ValueError(f"{who}: scan and labels must have the same shape")
    dev = labels.device if labels.is_cuda else (scan.device if scan.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    scan, labels = scan.to(dev).contiguous(), labels.to(dev).contiguous()
    if mask is not None:
        mask = _device_u8(mask, dev)
        if mask.shape != labels.shape:
            raise ValueError(f"{who}: mask and labels must have the same shape")
    return scan, labels, mask


def label_density(scan, labels, n, mask=None, bins=None):
    """Per label k = 1..n of a uint8 or int32 label volume (taken as it is: a lobe map is not widened), over the voxels with
    `mask` set when a mask is given: {"count", "sum", "sumsq": int64 [n], "min", "max": int32 [n]} as host numpy arrays, exact
    integers (a label without voxels: 0, 0, 0, 32767, -32768), and "hist": int64 [n, nbins + 2] on the DEVICE when
    `bins = (lo, width, nbins)` is given, else None -- entry 0 below lo, then nbins bins of `width` HU, then the rest."""
    n = int(n)
    scan, labels, mask = _scan_and_labels(scan, labels, mask, "label_density")
    lo, width, nbins = (0, 1, 0) if bins is None else (int(b) for b in bins)
    if bins is not None and nbins < 1:
        raise ValueError("label_density: bins = (lo, width, nbins) with nbins >= 1, or None")
    dev = labels.device
    if n <= 0 or labels.numel() == 0:
        hist = None if bins is None else torch.zeros((max(n, 0), nbins + 2), dtype=torch.int64, device=dev)
        z = np.zeros(max(n, 0), np.int64)
        return {"count": z, "sum": z.copy(), "sumsq": z.copy(), "min": np.full(max(n, 0), 32767, np.int32),
                "max": np.full(max(n, 0), -32768, np.int32), "hist": hist}
    # one buffer, one read-back: count [n] | sum [n] | sumsq [n] | min [n] int32, max [n] int32 in n int64 slots
    buf = torch.empty(4 * n, dtype=torch.int64, device=dev)
    mm = buf[3 * n:].view(torch.int32)
    hist = None if bins is None else torch.empty((n, nbins + 2), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        call("dram_label_density", scan.data_ptr(), labels.data_ptr(), 0 if labels.dtype == torch.uint8 else 1,
             None if mask is None else mask.data_ptr(), n, buf[:n].data_ptr(), buf[n:2 * n].data_ptr(), buf[2 * n:3 * n].data_ptr(),
             mm[:n].data_ptr(), mm[n:].data_ptr(), None if hist is None else hist.data_ptr(), lo, width, nbins, labels.numel(),
             _stream())
    host = buf.cpu().numpy()
    mm_h = host[3 * n:].view(np.int32)
    return {"count": host[:n].copy(), "sum": host[n:2 * n].copy(), "sumsq": host[2 * n:3 * n].copy(), "min": mm_h[:n].copy(),
            "max": mm_h[n:].copy(), "hist": hist}


def hist_summary(hist, bins, percentiles_permille=(), band_edges_hu=()):
    """Of the device histograms of `label_density(..., bins=bins)`: (percentiles int32 [n, nq], bands int64 [n, ne + 1]) on the
    host.  A percentile is the nearest-rank one (rank = max(1, ceil(q * count / 1000))), reported as the lower edge of its bin:
    exact for width 1; -2^31 when it lies below the range, 2^31 - 1 when above it or when the label is empty.  Band i counts the
    values in [edge[i-1], edge[i]); the edges must lie on bin edges."""
    lo, width, nbins = (int(b) for b in bins)
    q = np.asarray(percentiles_permille, dtype=np.int32).reshape(-1)
    edges = np.asarray(band_edges_hu, dtype=np.int32).reshape(-1)
    n, nq, ne = hist.shape[0], q.size, edges.size
    if n == 0:
        return np.zeros((0, nq), np.int32), np.zeros((0, ne + 1), np.int64)
    if hist.dtype != torch.int64 or not hist.is_cuda or tuple(hist.shape) != (n, nbins + 2):
        raise ValueError("hist_summary: an int64 [n, nbins + 2] histogram on the GPU")
    hist = hist.contiguous()
    pct = torch.empty((n, nq), dtype=torch.int32, device=hist.device)
    bands = torch.empty((n, ne + 1), dtype=torch.int64, device=hist.device)
    with torch.cuda.device(hist.device):
        call("dram_hist_summary", hist.data_ptr(), n, lo, width, nbins, q.ctypes.data if nq else None, nq,
             edges.ctypes.data if ne else None, ne, pct.data_ptr() if nq else None, bands.data_ptr(), _stream())
    return pct.cpu().numpy(), bands.cpu().numpy()


def report_from_tables(count, total, sumsq, vmin, vmax, percentiles, bands):
    """The per-label report from the exact integer tables (host arithmetic only): mean = sum / count in fp64; the variance is
    (count * sumsq - sum^2) / count^2 with the numerator formed in Python integers (it leaves int64), std its square root; an
    empty label has NaN for mean, std and the band fractions."""
    n = len(count)
    mean, std = np.full(n, np.nan), np.full(n, np.nan)
    for k in range(n):
        c, s, q = int(count[k]), int(total[k]), int(sumsq[k])
        if c:
            mean[k] = s / c
            std[k] = float(np.sqrt(np.float64((c * q - s * s) / (c * c))))
    bands = np.asarray(bands, dtype=np.int64)
    cnt = np.asarray(count, dtype=np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        fraction = np.where(cnt[:, None] > 0, bands.astype(np.float64) / cnt[:, None].astype(np.float64), np.nan)
    return {"voxels": cnt.copy(), "mean_hu": mean, "std_hu": std, "min_hu": np.asarray(vmin, dtype=np.int32).copy(),
            "max_hu": np.asarray(vmax, dtype=np.int32).copy(), "percentiles_hu": np.asarray(percentiles, dtype=np.int32),
            "band_voxels": bands, "band_fraction": fraction}


def label_report(scan, labels, n, mask=None, percentiles_permille=PERCENTILES_PERMILLE, band_edges_hu=BAND_EDGES_HU,
                 hist_range=HIST_RANGE):
    """The density report of the labels 1..n of a uint8 or int32 label volume over an int16 scan (with `mask`: over the masked
    voxels only), as host numpy arrays with one row per label:
        voxels (int64), mean_hu, std_hu (fp64), min_hu, max_hu (int32; 32767 / -32768 for an empty label),
        percentiles_hu (int32 [n, nq], nearest rank; see `hist_summary` for the out-of-range values),
        band_voxels (int64 [n, ne + 1]), band_fraction (fp64, band_voxels / voxels).
    An empty label has NaN for mean, std and the fractions.  `hist_range = (lo, width, nbins)` is the histogram behind the
    percentiles and bands; the default covers -1024 .. 3071 HU in bins of 1 HU, so the percentiles are exact there.

    The default band edges (-950, -750, -300 HU; BAND_NAMES = laa, aerated, ggo, consolidation) follow a common convention of
    CT densitometry.  They are a parameter, not something this project has validated clinically."""
    bins = tuple(int(b) for b in hist_range)
    d = label_density(scan, labels, n, mask, bins)
    pct, bands = hist_summary(d["hist"], bins, percentiles_permille, band_edges_hu)
    return report_from_tables(d["count"], d["sum"], d["sumsq"], d["min"], d["max"], pct, bands)


def row_of(report, k):
    """Row k (0-based) of a `label_report` as a dict of numpy scalars and 1-D arrays."""
    return {key: (v[k].copy() if v[k].ndim else v[k]) for key, v in report.items()}
