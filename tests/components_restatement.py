"""Plain numpy / Python restatement of the lesion-wise report (dram_amd/lesions.py, csrc/components.hip): connected-component
labelling by flood fill in raster order, the per-component statistics, the per-lobe burden table and the report arithmetic.
No scipy here: tests/test_components_cpu.py holds this restatement against scipy.ndimage where scipy imports, and the GPU tests
hold the kernels against this restatement."""
import itertools
import math

import numpy as np

# IntRegLoss.ctss_ratio_map (dram/metrics.py:76-83), written out again on purpose
CTSS_RATIO_MAP = {0: (0.0, 0.001), 1: (0.001, 0.01), 2: (0.01, 0.05), 3: (0.05, 0.35), 4: (0.35, 0.5), 5: (0.5, 1.00001)}


def ratio_to_label(ratio):
    return [k for k, (lo, hi) in CTSS_RATIO_MAP.items() if lo <= ratio < hi][0]


def neighbours(connectivity):
    """The offsets of generate_binary_structure(3, connectivity) without the centre: 6, 18 or 26."""
    return [d for d in itertools.product((-1, 0, 1), repeat=3) if 0 < sum(abs(v) for v in d) <= connectivity]


def label(mask, connectivity=1):
    """(labels int32, n): a raster scan that starts a flood fill at every set voxel not reached yet, so that component k is the
    one whose first voxel in raster order is the k-th such start."""
    mask = np.asarray(mask) != 0
    D, H, W = mask.shape
    nb = neighbours(connectivity)
    labels = np.zeros(mask.shape, dtype=np.int32)
    n = 0
    for z, y, x in zip(*np.nonzero(mask)):                   # np.nonzero walks in raster (C) order
        if labels[z, y, x]:
            continue
        n += 1
        labels[z, y, x] = n
        stack = [(int(z), int(y), int(x))]
        while stack:
            cz, cy, cx = stack.pop()
            for dz, dy, dx in nb:
                az, ay, ax = cz + dz, cy + dy, cx + dx
                if 0 <= az < D and 0 <= ay < H and 0 <= ax < W and mask[az, ay, ax] and not labels[az, ay, ax]:
                    labels[az, ay, ax] = n
                    stack.append((az, ay, ax))
    return labels, n


def stats(labels, n, other=None):
    """voxels [n] int64, bbox [n,6] int32 (z0, z1, y0, y1, x0, x1 half-open), hits [n] int64 or None; a voxel whose label is
    outside 1..n counts nowhere."""
    labels = np.asarray(labels)
    voxels = np.zeros(n, dtype=np.int64)
    hits = None if other is None else np.zeros(n, dtype=np.int64)
    bbox = np.tile(np.array([labels.shape[0], 0, labels.shape[1], 0, labels.shape[2], 0], dtype=np.int32), (n, 1))
    for z, y, x in zip(*np.nonzero(labels)):
        k = int(labels[z, y, x])
        if not 1 <= k <= n:
            continue
        voxels[k - 1] += 1
        b = bbox[k - 1]
        b[0], b[1] = min(b[0], z), max(b[1], z + 1)
        b[2], b[3] = min(b[2], y), max(b[3], y + 1)
        b[4], b[5] = min(b[4], x), max(b[5], x + 1)
        if other is not None and other[z, y, x]:
            hits[k - 1] += 1
    return voxels, bbox, hits


def relabel(labels, n, keep):
    """Kept components renumbered 1.. in their old order; (labels, n_kept, mask uint8)."""
    lut = np.zeros(n + 1, dtype=np.int32)
    new = 0
    for k in range(1, n + 1):
        if keep[k - 1]:
            new += 1
            lut[k] = new
    out = lut[np.asarray(labels)]
    return out.astype(np.int32), new, (out != 0).astype(np.uint8)


def burden(mask, lobe):
    """counts [256,2] int64: per lobe value {voxels, of which set in mask}."""
    counts = np.zeros((256, 2), dtype=np.int64)
    for v, m in zip(np.asarray(lobe).ravel().tolist(), (np.asarray(mask).ravel() != 0).tolist()):
        counts[v, 0] += 1
        counts[v, 1] += m
    return counts


def report_from_tables(voxels, bbox, hits, counts_of_kept_mask, spacing, min_volume_mm3, ref_found=None):
    """The report arithmetic on the tables alone (what the host side of lesion_report does after the kernels): keep rule,
    volumes, per-lobe ratio and score, and -- with hits (against the reference) and ref_found (per reference component: does
    the kept mask touch it) -- the detection figures.  counts_of_kept_mask is a function keep -> burden table of the kept mask."""
    voxel_volume = float(np.prod(np.asarray(spacing, dtype=np.float64)))
    keep = np.array([float(v) * voxel_volume >= float(min_volume_mm3) for v in voxels], dtype=bool)
    out = {"keep": keep, "n_lesions": int(keep.sum()),
           "volumes_ml": np.array([float(v) * voxel_volume / 1000.0 for v in np.asarray(voxels)[keep]], dtype=np.float64),
           "bboxes": np.asarray(bbox)[keep], "lobes": {}}
    counts = counts_of_kept_mask(keep)
    for v in range(1, 256):
        if counts[v, 0]:
            ratio = float(np.float64(int(counts[v, 1])) / np.float64(int(counts[v, 0])))
            out["lobes"][v] = {"voxels": int(counts[v, 0]), "lesion_voxels": int(counts[v, 1]), "ratio": ratio,
                               "ctss": ratio_to_label(ratio)}
    if ref_found is not None:
        found = ref_found(keep)
        n_ref, n_found = len(found), int(sum(bool(f) for f in found))
        out.update(n_reference=n_ref, n_found=n_found, sensitivity=n_found / n_ref if n_ref else math.nan,
                   n_false=int(sum(1 for h, k in zip(hits, keep) if k and h == 0)))
    return out


def report(mask, lobe, spacing, connectivity=1, min_volume_mm3=0.0, reference=None):
    """lesion_report, restated on host arrays: returns the same keys (mask / labels as numpy arrays)."""
    mask = np.asarray(mask) != 0
    labels, n = label(mask, connectivity)
    voxels, bbox, hits = stats(labels, n, None if reference is None else np.asarray(reference) != 0)
    kept = {}

    def kept_of(keep):
        if "v" not in kept:
            kept["v"] = relabel(labels, n, keep)
        return kept["v"]

    ref_found = None
    if reference is not None:
        ref_labels, n_ref = label(reference, connectivity)

        def ref_found(keep):
            return stats(ref_labels, n_ref, kept_of(keep)[2])[2] > 0

    out = report_from_tables(voxels, bbox, hits, lambda keep: burden(kept_of(keep)[2], lobe), spacing, min_volume_mm3, ref_found)
    new_labels, _, new_mask = kept_of(out.pop("keep"))
    out.update(labels=new_labels, mask=new_mask)
    return out
