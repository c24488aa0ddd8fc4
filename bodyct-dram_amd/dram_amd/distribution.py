"""Lesion distribution report on the device: where in the lung the lesions lie -- peripheral (subpleural) against central, upper
against lower zone, a lesion's depth below the lung surface and its centre -- without a host-side
`scipy.ndimage.distance_transform_edt` over the whole lobe map followed by `sum_labels / minimum / center_of_mass` per label.

    depth = lung_depth(lobe, spacing)                                   # mm from every voxel to the nearest non-lung voxel
    rep = lesion_distribution(mask, lobe, spacing)                      # per lobe and for both lungs
    rep = lesion_report(mask, lobe, spacing, distribution=True)         # lesions.lesion_report with a `distribution` entry

Kernels: csrc/distance.hip (the exact distance transform), csrc/distribution.hip (one pass over depth and labels for the exact
integer tables per label: count, fixed-point depth sum, minimum and maximum depth, index sums, depth histogram, zone counts),
csrc/density.hip (dram_hist_summary: the histograms' percentiles and shell counts).  Only O(labels) numbers travel to the host,
where means, centroids and shares are formed from the exact integers.

Index 0 is the low-index end of each axis: which end is cranial, anterior or right depends on the scan's orientation, which this
module does not know.  The subpleural distance and the shell edges are conventions and parameters; nothing here has been
validated clinically.
"""
import numpy as np
import torch

from ._lib import call
from .surface import _device_u8, _spacing, _stream, _volume, distance_transform

Q_PER_MM = 1024                               # qsum counts depth in 1/1024 mm
BINS_PER_MM, NBINS = 4, 1024                  # the histogram behind percentiles, shells and the peripheral share: 0.25 mm bins up to 256 mm
SHELLS_MM = (5.0, 10.0, 20.0)
ZONES = (3, 2, 1)                             # thirds along z, halves along y
PERCENTILES_PERMILLE = (150, 500, 850)
SUBPLEURAL_MM = 3.0
INT32_MAX = 2 ** 31 - 1


def lung_depth(lobe, spacing):
    """The depth map of a [D,H,W] lobe map (0 = not lung): float32 on the device, the distance in mm under `spacing` (z, y, x) from
    every voxel to the centre of the nearest non-lung voxel -- `surface.distance_transform(lobe == 0, spacing)`, so 0 outside
    the lung, one voxel spacing on the lung's outermost layer, and +inf everywhere when the map has no zero.

    The faces of the volume are not a surface: a lung that the field of view cuts has no pleura there, and the depth of its
    voxels is measured to the surfaces that the volume does show.  Mediastinal and diaphragmatic surfaces count like costal
    ones (all of them border non-lung voxels); fissures do not, since the voxels on both sides of a fissure are lung."""
    sp = _spacing(spacing, "lung_depth")
    lobe = _volume(lobe, "lung_depth")
    if not lobe.is_cuda:
        lobe = lobe.to(torch.device("cuda", torch.cuda.current_device()))
    return distance_transform(lobe == 0, sp)


def _zones(zones, who):
    z = tuple(int(v) for v in zones)
    if len(z) != 3 or any(not 1 <= v <= 8 for v in z):
        raise ValueError(f"{who}: zones = (nz, ny, nx), each in 1..8")
    return z


def _box(box, who):
    if box is None:
        return None
    b = np.asarray(box, dtype=np.int64).reshape(-1)
    if b.shape != (6,) or np.any(b[0::2] >= b[1::2]) or np.any(np.abs(b) >= 2 ** 31):
        raise ValueError(f"{who}: box = (z0, z1, y0, y1, x0, x1) with a0 < a1 on every axis")
    return np.ascontiguousarray(b, dtype=np.int32)


def _tables_on_device(depth, labels, n, mask, bins_per_mm, nbins, zones, box):
    """One int64 device buffer count [n] | qsum [n] | possum [n,3] | dmin, dmax (uint32 [n] each in n slots) | hist [n, nbins + 2] |
    zones [n, nzt], filled by dram_label_depth; returns (buf, hist view or None)."""
    nzt = zones[0] * zones[1] * zones[2] if (zones != (1, 1, 1) or box is not None) else 0
    row = nbins + 2 if nbins else 0
    buf = torch.empty(n * (6 + row + nzt), dtype=torch.int64, device=labels.device)
    mm = buf[5 * n:6 * n].view(torch.int32)
    hist = buf[6 * n:6 * n + n * row].view(n, row) if nbins else None
    zone_t = buf[6 * n + n * row:] if nzt else None
    with torch.cuda.device(labels.device):
        call("dram_label_depth", depth.data_ptr(), labels.data_ptr(), 0 if labels.dtype == torch.uint8 else 1,
             None if mask is None else mask.data_ptr(), n, buf[:n].data_ptr(), buf[n:2 * n].data_ptr(), mm[:n].data_ptr(), mm[n:].data_ptr(),
             buf[2 * n:5 * n].data_ptr(), None if hist is None else hist.data_ptr(), bins_per_mm, nbins,
             None if zone_t is None else zone_t.data_ptr(), None if box is None else box.ctypes.data, *zones, *labels.shape, _stream())
    return buf, hist


def _split(host, n, nbins, nzt):
    """The host copy of `_tables_on_device`'s buffer as the dictionary of `label_depth`."""
    row = nbins + 2 if nbins else 0
    mm = host[5 * n:6 * n].view(np.uint32)
    return {"count": host[:n].copy(), "qsum": host[n:2 * n].copy(), "dmin": mm[:n].copy(), "dmax": mm[n:].copy(),
            "possum": host[2 * n:5 * n].reshape(n, 3).copy(), "hist": host[6 * n:6 * n + n * row].reshape(n, row).copy() if nbins else None,
            "zones": host[6 * n + n * row:].reshape(n, nzt).copy() if nzt else None}


def _empty_tables(n, nbins, nzt):
    return _split(np.zeros(n * (6 + (nbins + 2 if nbins else 0) + nzt), np.int64), n, nbins, nzt)


def _inputs(depth, labels, mask, who):
    depth, labels = torch.as_tensor(depth), torch.as_tensor(labels)
    if depth.dtype != torch.float32:
        raise ValueError(f"{who}: the depth map must be float32")
    if labels.dtype not in (torch.uint8, torch.int32):
        raise ValueError(f"{who}: labels must be uint8 or int32")
    if labels.dim() != 3 or depth.shape != labels.shape:
        raise ValueError(f"{who}: depth and labels must be [D,H,W] volumes of the same shape")
    dev = labels.device if labels.is_cuda else (depth.device if depth.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    depth, labels = depth.to(dev).contiguous(), labels.to(dev).contiguous()
    if mask is not None:
        mask = _device_u8(mask, dev)
        if mask.shape != labels.shape:
            raise ValueError(f"{who}: mask and labels must have the same shape")
    return depth, labels, mask


def label_depth(depth, labels, n, mask=None, bins_per_mm=4, nbins=1024, zones=(1, 1, 1), box=None):
    """The exact integer tables of dram_label_depth (include/dram_hip.h has the definition) per label k = 1..n of a uint8 or int32
    [D,H,W] label volume over a float32 depth map, over the voxels with `mask` set when a mask is given, as host numpy arrays
    from one read-back: {"count", "qsum": int64 [n], "dmin", "dmax": uint32 [n] (the depths' bit patterns), "possum": int64
    [n,3] (z, y, x), "hist": int64 [n, nbins + 2] or None for nbins = 0, "zones": int64 [n, nz*ny*nx] or None}.  `zones` =
    (nz, ny, nx) positional zones of `box` = (z0, z1, y0, y1, x0, x1), the whole volume without a box; with the default
    (1, 1, 1) and no box there is no zone table."""
    n, nbins, bins_per_mm = int(n), int(nbins), int(bins_per_mm)
    zones, box = _zones(zones, "label_depth"), _box(box, "label_depth")
    depth, labels, mask = _inputs(depth, labels, mask, "label_depth")
    nzt = zones[0] * zones[1] * zones[2] if (zones != (1, 1, 1) or box is not None) else 0
    if n <= 0 or labels.numel() == 0:
        t = _empty_tables(max(n, 0), max(nbins, 0), nzt)
        t["dmin"][:] = 0x7f800000
        return t
    buf, _ = _tables_on_device(depth, labels, n, mask, bins_per_mm, nbins, zones, box)
    return _split(buf.cpu().numpy(), n, nbins, nzt)


# ---- host arithmetic on the integer tables
def shell_bins(shells_mm, bins_per_mm=BINS_PER_MM, nbins=NBINS):
    """The shell edges as bin counts j = edge * bins_per_mm: every edge must be a multiple of 1 / bins_per_mm in
    0 .. nbins / bins_per_mm, and the edges must ascend strictly (at most 15), else ValueError."""
    out = []
    for e in shells_mm:
        j = float(e) * bins_per_mm
        if not (j == int(j) and 0 <= j <= nbins):
            raise ValueError(f"shell edge {e} mm is not a multiple of 1/{bins_per_mm} mm in 0 .. {nbins / bins_per_mm} mm")
        out.append(int(j))
    if len(out) > 15 or any(b <= a for a, b in zip(out, out[1:])):
        raise ValueError("shell edges must ascend strictly, 15 of them at most")
    return out


def peripheral_share(parenchyma_hist, lesion_hist):
    """Of two histogram rows of one lobe (its whole volume and its lesion voxels): the share of the lesion voxels that lie no
    deeper than the bin at which the running count of the lobe's own voxels first reaches a third of them (the smallest entry e
    with 3 * sum(parenchyma[:e + 1]) >= sum(parenchyma)) -- the outer third of the lobe's volume, to the bin width.  1/3 for a
    lesion load spread evenly over the lobe; exact integers up to the final fp64 quotient; NaN when either row is empty."""
    p = [int(v) for v in np.asarray(parenchyma_hist).reshape(-1)]
    les = [int(v) for v in np.asarray(lesion_hist).reshape(-1)]
    total, total_l = sum(p), sum(les)
    if total == 0 or total_l == 0:
        return float("nan")
    run = 0
    for e, c in enumerate(p):
        run += c
        if 3 * run >= total:
            break
    return sum(les[:e + 1]) / total_l


def sum_tables(t):
    """The tables of all labels together (both lungs from the lobes) as tables with one row: sums of the integer sums, minimum of
    the minima, maximum of the maxima."""
    one = lambda key: None if t[key] is None else t[key].sum(axis=0, dtype=np.int64, keepdims=True)
    dmin = np.array([t["dmin"].min() if len(t["dmin"]) else 0x7f800000], dtype=np.uint32)
    dmax = np.array([t["dmax"].max() if len(t["dmax"]) else 0], dtype=np.uint32)
    return {"count": one("count"), "qsum": one("qsum"), "dmin": dmin, "dmax": dmax, "possum": one("possum"), "hist": one("hist"),
            "zones": one("zones")}


def axis_zone(i, a0, a1, nzones):
    """((clamp(i, a0, a1 - 1) - a0) * nzones) // (a1 - a0) in Python integers."""
    return ((min(max(int(i), int(a0)), int(a1) - 1) - int(a0)) * int(nzones)) // (int(a1) - int(a0))


def centroid_zone(possum, count, box, zones):
    """The zone of a label's centroid: per axis the index nearest to possum / count (halves upwards, in integers), its zone as in
    the kernel.  None for an empty label."""
    c = int(count)
    if c == 0:
        return None
    zz, zy, zx = (axis_zone((2 * int(possum[a]) + c) // (2 * c), box[2 * a], box[2 * a + 1], zones[a]) for a in range(3))
    return (zz * zones[1] + zy) * zones[2] + zx


def rows_from_tables(t, spacing, bins_per_mm=BINS_PER_MM, percentile_bins=None, shell_voxels=None):
    """The report rows from the exact integer tables (host arithmetic only), one row per label as arrays:
        voxels (int64), depth_mean_mm = float64(qsum) / 1024 / float64(voxels), depth_min_mm, depth_max_mm (float32, the tables'
        bit patterns: +inf and 0 for an empty label), centroid (fp64 [n,3], possum / voxels in voxel indices z, y, x),
        centroid_mm (centroid * spacing),
        percentiles_mm (fp64 [n,nq], with `percentile_bins` of dram_hist_summary: the lower edge bin / bins_per_mm of the bin that
        holds the nearest-rank percentile, +inf past the histogram), shell_voxels (int64 [n,ns], voxels shallower than each
        edge) and shell_fraction, zone_voxels (int64 [n, nz*ny*nx]) and zone_fraction where the tables hold zones.
    An empty label has NaN for the mean, the centroid, the percentiles and the fractions."""
    cnt = np.asarray(t["count"], dtype=np.int64)
    n = len(cnt)
    sp = np.asarray(spacing, dtype=np.float64).reshape(3)
    some = cnt > 0
    safe = np.where(some, cnt, 1).astype(np.float64)
    mean = np.where(some, np.asarray(t["qsum"], dtype=np.int64).astype(np.float64) / float(Q_PER_MM) / safe, np.nan)
    centroid = np.where(some[:, None], np.asarray(t["possum"], dtype=np.int64).reshape(n, 3).astype(np.float64) / safe[:, None], np.nan)
    out = {"voxels": cnt.copy(), "depth_mean_mm": mean, "depth_min_mm": np.asarray(t["dmin"], dtype=np.uint32).view(np.float32).copy(),
           "depth_max_mm": np.asarray(t["dmax"], dtype=np.uint32).view(np.float32).copy(), "centroid": centroid,
           "centroid_mm": centroid * sp[None, :]}
    if percentile_bins is not None:
        p = np.asarray(percentile_bins, dtype=np.int64).reshape(n, -1)
        mm = np.where(p == INT32_MAX, np.inf, p.astype(np.float64) / float(bins_per_mm))
        out["percentiles_mm"] = np.where(some[:, None], mm, np.nan)
    if shell_voxels is not None:
        s = np.asarray(shell_voxels, dtype=np.int64).reshape(n, -1)
        out["shell_voxels"] = s
        out["shell_fraction"] = np.where(some[:, None], s.astype(np.float64) / safe[:, None], np.nan)
    if t.get("zones") is not None:
        z = np.asarray(t["zones"], dtype=np.int64)
        out["zone_voxels"] = z.copy()
        out["zone_fraction"] = np.where(some[:, None], z.astype(np.float64) / safe[:, None], np.nan)
    return out


def row_of(rows, k):
    """Row k (0-based) of `rows_from_tables` as a dict of numpy scalars and 1-D arrays."""
    return {key: (v[k].copy() if v[k].ndim else v[k]) for key, v in rows.items()}


def lobe_entry(parenchyma, lesion, par_hist, les_hist):
    """{"parenchyma", "lesion": the two rows, "peripheral_share": `peripheral_share` of their histograms, "depth_ratio": the
    lesion's mean depth over the parenchyma's (NaN when either is empty or the latter is 0)}."""
    a, b = float(lesion["depth_mean_mm"]), float(parenchyma["depth_mean_mm"])
    ratio = a / b if (a == a and b == b and b != 0.0) else float("nan")
    return {"parenchyma": parenchyma, "lesion": lesion, "peripheral_share": peripheral_share(par_hist, les_hist), "depth_ratio": ratio}


def _lobe_boxes(lobe):
    """(present labels, bounding box of lobe > 0 as z0, z1, y0, y1, x0, x1 or None) from dram_label_bboxes."""
    boxes = torch.empty(255 * 6, dtype=torch.int32, device=lobe.device)
    with torch.cuda.device(lobe.device):
        call("dram_label_bboxes", lobe.data_ptr(), boxes.data_ptr(), 255, *lobe.shape, _stream())
    boxes = boxes.cpu().numpy().reshape(255, 6)
    present = boxes[:, 3] >= boxes[:, 0]
    if not present.any():
        return [], None
    lo, hi = boxes[present, :3].min(axis=0), boxes[present, 3:].max(axis=0) + 1
    return [int(v) + 1 for v in np.nonzero(present)[0]], np.array([lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]], dtype=np.int32)


def lesion_distribution(mask, lobe, spacing, labels=None, n=0, depth=None, shells_mm=SHELLS_MM, zones=ZONES, box=None,
                        percentiles_permille=PERCENTILES_PERMILLE, subpleural_mm=SUBPLEURAL_MM):
    """Where the lesions of a [D,H,W] lesion mask lie in the lungs of its lobe map (uint8, 0 = not lung), under the voxel spacing
    (z, y, x) in mm.  `depth` is `lung_depth(lobe, spacing)` unless a float32 depth map is handed in.  Returns

        lobes: {label: {"parenchyma": row, "lesion": row, "peripheral_share", "depth_ratio"}} for every lobe label present; the
            first row is over the whole lobe, the second over its voxels inside `mask`.  peripheral_share (`peripheral_share`):
            the share of the lobe's lesion voxels that lie shallower than the depth holding the outer third of the lobe's own
            volume -- 1/3 for an evenly spread lesion load, above it for a peripheral one; depth_ratio: the lesion's mean depth
            over the parenchyma's.
        lungs: the same entry for all lobes together, from the sums of the lobes' integer tables.
        lesions (with `labels`, an int32 volume of components 1..`n`, e.g. `lesion_report`'s): rows of all components as arrays
            (no histogram, so without percentiles and shells), "subpleural": depth_min_mm <= subpleural_mm, "zone": the zone of
            each component's centroid (a list; None for a component without a voxel of valid depth).
        box, zones, shells_mm, percentiles_permille, subpleural_mm, bins_per_mm: the settings used.

    A row (`rows_from_tables`): voxels, depth_mean_mm, depth_min_mm, depth_max_mm, percentiles_mm, shell_voxels / shell_fraction
    (the voxels with depth below each edge of `shells_mm`; an edge must be a multiple of 1 / 4 mm, else ValueError), centroid
    (z, y, x in fp64 voxel indices) and centroid_mm, zone_voxels / zone_fraction over the `zones` = (nz, ny, nx) positional zones
    of `box` = (z0, z1, y0, y1, x0, x1), by default the bounding box of lobe > 0; zone index (zz * ny + zy) * nx + zx.

    Index 0 is the low-index end of each axis: which end is cranial or anterior depends on the scan's orientation.
    `subpleural_mm` and the shell edges are conventions and parameters, not clinically validated here."""
    who = "lesion_distribution"
    sp = _spacing(spacing, who)
    zones, box = _zones(zones, who), _box(box, who)
    edges = shell_bins(shells_mm)
    q = np.asarray(percentiles_permille, dtype=np.int32).reshape(-1)
    mask = _device_u8(_volume(mask, who))
    dev = mask.device
    lobe = torch.as_tensor(lobe).to(device=dev, dtype=torch.uint8).contiguous()
    if lobe.shape != mask.shape:
        raise ValueError(f"{who}: mask and lobe must be [D,H,W] volumes of the same shape")
    if depth is None:
        depth = lung_depth(lobe, sp) if lobe.numel() else torch.empty(lobe.shape, dtype=torch.float32, device=dev)
    depth, lobe, mask = _inputs(depth, lobe, mask, who)
    present, lobe_box = _lobe_boxes(lobe) if lobe.numel() else ([], None)
    if box is None:
        box = lobe_box if lobe_box is not None else np.array([0, max(lobe.shape[0], 1), 0, max(lobe.shape[1], 1), 0, max(lobe.shape[2], 1)], np.int32)
    nzt = zones[0] * zones[1] * zones[2]
    out = {"lobes": {}, "lungs": None, "box": tuple(int(v) for v in box), "zones": zones, "shells_mm": tuple(float(e) for e in shells_mm),
           "percentiles_permille": tuple(int(v) for v in q), "subpleural_mm": float(subpleural_mm), "bins_per_mm": BINS_PER_MM}
    if present:
        from .density import hist_summary
        top = max(present)
        whole_d, whole_hist = _tables_on_device(depth, lobe, top, None, BINS_PER_MM, NBINS, zones, box)
        inside_d, inside_hist = _tables_on_device(depth, lobe, top, mask, BINS_PER_MM, NBINS, zones, box)
        # rows 0 .. top-1: the lobes, top .. 2 top - 1: their lesion voxels, then both lungs and their lesion voxels
        hists = torch.cat((whole_hist, inside_hist, whole_hist.sum(dim=0, keepdim=True), inside_hist.sum(dim=0, keepdim=True)))
        pct, bands = hist_summary(hists, (0, 1, NBINS), q, np.asarray(edges, dtype=np.int32))
        shells = np.cumsum(bands[:, :len(edges)], axis=1)
        whole, inside = _split(whole_d.cpu().numpy(), top, NBINS, nzt), _split(inside_d.cpu().numpy(), top, NBINS, nzt)
        rows_w = rows_from_tables(whole, sp, BINS_PER_MM, pct[:top], shells[:top])
        rows_i = rows_from_tables(inside, sp, BINS_PER_MM, pct[top:2 * top], shells[top:2 * top])
        for v in present:
            out["lobes"][v] = lobe_entry(row_of(rows_w, v - 1), row_of(rows_i, v - 1), whole["hist"][v - 1], inside["hist"][v - 1])
        lw, li = sum_tables(whole), sum_tables(inside)
        out["lungs"] = lobe_entry(row_of(rows_from_tables(lw, sp, BINS_PER_MM, pct[2 * top:2 * top + 1], shells[2 * top:2 * top + 1]), 0),
                                  row_of(rows_from_tables(li, sp, BINS_PER_MM, pct[2 * top + 1:], shells[2 * top + 1:]), 0),
                                  lw["hist"][0], li["hist"][0])
    if labels is not None:
        n = int(n)
        labels = torch.as_tensor(labels)
        if labels.dtype != torch.int32 or labels.shape != lobe.shape:
            raise ValueError(f"{who}: labels must be an int32 [D,H,W] volume of the mask's shape")
        if n > 0 and labels.numel():
            buf, _ = _tables_on_device(depth, labels.to(dev).contiguous(), n, None, BINS_PER_MM, 0, zones, box)
            t = _split(buf.cpu().numpy(), n, 0, nzt)
        else:
            t = _empty_tables(0, 0, nzt)
        rows = rows_from_tables(t, sp)
        rows["subpleural"] = rows["depth_min_mm"].astype(np.float64) <= float(subpleural_mm)
        rows["zone"] = [centroid_zone(t["possum"][k], t["count"][k], box, zones) for k in range(len(t["count"]))]
        out["lesions"] = rows
    return out
