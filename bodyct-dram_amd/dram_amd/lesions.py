"""Lesion-wise report on the device: what a consumer of `LobeInference`'s final mask otherwise does on the host with
`scipy.ndimage.label` over the whole volume -- split the mask into lesions, drop specks below a minimum volume, report count,
volumes and bounding boxes, match against a reference mask lesion by lesion -- and the CT severity score of
`IntRegLoss.ctss_ratio_map` (dram/metrics.py:76-83) per lobe from the final mask (the reference derives it for the whole scan
and from the heat map only).

    res = LobeInference(model).run(scan, lobe, spacing, vessel=vessel)
    rep = lesion_report(res["mask_post"], lobe, spacing, min_volume_mm3=10.0)

Kernels: csrc/components.hip (union-find labelling in a fixed number of launches, component statistics with integer atomics,
look-up-table relabelling, per-lobe burden); the boundary metrics against a reference come from `surface`.  Only small
per-component tables travel to the host.
"""
import numpy as np
import torch

from ._lib import call, lib
from .inference import ratio_to_label
from .surface import _device_u8, _stream, surface_distances


def label_components(mask, connectivity=1):
    """Connected components of a [D,H,W] mask (non-zero = set; a device tensor or anything `torch.as_tensor` accepts) under
    `scipy.ndimage.generate_binary_structure(3, connectivity)`: returns (labels, n) with labels int32 on the device, 0 on the
    background and 1..n numbered as `scipy.ndimage.label` numbers them, and n a Python int (reading it is the one
    synchronisation)."""
    mask = _device_u8(mask)
    if mask.dim() != 3:
        raise ValueError("label_components: a [D,H,W] mask")
    if connectivity not in (1, 2, 3):
        raise ValueError("label_components: connectivity must be 1, 2 or 3 (6, 18 or 26 neighbours)")
    D, H, W = mask.shape
    labels = torch.empty((D, H, W), dtype=torch.int32, device=mask.device)
    if mask.numel() == 0:
        return labels, 0
    with torch.cuda.device(mask.device):
        ws_bytes = lib.dram_cc_ws_bytes(D, H, W)
        ws = torch.empty(max(ws_bytes, 4) // 4, dtype=torch.int32, device=mask.device)
        count = torch.empty(1, dtype=torch.int32, device=mask.device)
        call("dram_cc_label", mask.data_ptr(), labels.data_ptr(), count.data_ptr(), int(connectivity), D, H, W, ws.data_ptr(),
             ws_bytes, _stream())
        return labels, int(count.item())


def component_stats(labels, n, other=None):
    """Per component k = 1..n of an int32 device label volume: {"voxels": int64 [n], "bbox": int32 [n,6] = (z0, z1, y0, y1, x0,
    x1) half-open like `scipy.ndimage.find_objects`, "hits": int64 [n] = voxels of k set in the mask `other`, or None} as host
    numpy arrays."""
    n = int(n)
    if labels.dim() != 3 or labels.dtype != torch.int32 or not labels.is_cuda:
        raise ValueError("component_stats: an int32 [D,H,W] label volume on the GPU")
    if n <= 0 or labels.numel() == 0:
        return {"voxels": np.zeros(0, np.int64), "bbox": np.zeros((0, 6), np.int32),
                "hits": None if other is None else np.zeros(0, np.int64)}
    labels = labels.contiguous()
    dev = labels.device
    if other is not None:
        other = _device_u8(other, dev)
        if other.shape != labels.shape:
            raise ValueError("component_stats: labels and other must have the same shape")
    # one buffer, one read-back: voxels [n] | hits [n] | bbox [n,6] int32 in 3n int64 slots
    buf = torch.empty(5 * n, dtype=torch.int64, device=dev)
    voxels, hits, bbox = buf[:n], buf[n:2 * n], buf[2 * n:]
    with torch.cuda.device(dev):
        call("dram_cc_stats", labels.data_ptr(), None if other is None else other.data_ptr(), n, voxels.data_ptr(), bbox.data_ptr(),
             None if other is None else hits.data_ptr(), *labels.shape, _stream())
    host = buf.cpu().numpy()
    return {"voxels": host[:n].copy(), "bbox": host[2 * n:].view(np.int32).reshape(n, 6).copy(),
            "hits": None if other is None else host[n:2 * n].copy()}


def _relabel(labels, n, keep):
    """Keep the components whose entry of the boolean host array `keep` is set, renumbered 1.. in their old order."""
    keep = np.asarray(keep, dtype=bool)
    lut = np.zeros(int(n) + 1, dtype=np.int32)
    lut[1:] = np.where(keep, np.cumsum(keep), 0)
    out = torch.empty_like(labels)
    mask = torch.empty(labels.shape, dtype=torch.uint8, device=labels.device)
    if labels.numel():
        lut_d = torch.from_numpy(lut).to(labels.device)
        with torch.cuda.device(labels.device):
            call("dram_cc_relabel", labels.data_ptr(), lut_d.data_ptr(), int(n), out.data_ptr(), mask.data_ptr(), labels.numel(),
                 _stream())
    return out, int(keep.sum()), mask


def remove_small(labels, n, voxels, min_voxels):
    """Drop the components with fewer than `min_voxels` voxels (`voxels`: their counts, `component_stats(...)["voxels"]`):
    returns (labels, n_kept, mask) with the kept components renumbered in their old order and mask = labels != 0 as uint8."""
    voxels = np.asarray(voxels)
    if voxels.shape != (int(n),):
        raise ValueError("remove_small: one voxel count per component")
    return _relabel(labels.contiguous(), n, voxels >= min_voxels)


def lobe_burden(mask, lobe):
    """counts [256,2] int64 (host): per lobe label value {voxels of that lobe, of which set in mask}."""
    mask = _device_u8(mask)
    lobe = torch.as_tensor(lobe).to(device=mask.device, dtype=torch.uint8).contiguous()
    if lobe.shape != mask.shape:
        raise ValueError("lobe_burden: mask and lobe must have the same shape")
    counts = torch.empty((256, 2), dtype=torch.int64, device=mask.device)
    if mask.numel() == 0:
        return np.zeros((256, 2), np.int64)
    with torch.cuda.device(mask.device):
        call("dram_lobe_burden", mask.data_ptr(), lobe.data_ptr(), counts.data_ptr(), mask.numel(), _stream())
    return counts.cpu().numpy()


def lesion_report(mask, lobe, spacing, connectivity=1, min_volume_mm3=0.0, reference=None, surface=False, tolerances_mm=(),
                  scan=None, percentiles_permille=(150, 500, 850), band_edges_hu=(-950, -750, -300), distribution=False, depth=None,
                  shells_mm=(5.0, 10.0, 20.0), zones=(3, 2, 1), box=None, subpleural_mm=3.0, shape=False, texture=False):
    """The lesion-wise report of a [D,H,W] lesion mask (e.g. `LobeInference.run(...)["mask_post"]`, or the "original" entries
    on the scan's own grid) with its lobe map and voxel spacing (z, y, x) in mm.

    A component (under `connectivity`) is kept iff voxels * voxel_volume >= min_volume_mm3, voxel_volume = float64(prod(spacing)),
    evaluated in fp64 on the host.  Returns
        mask (uint8, device, the kept components), labels (int32, device, renumbered 1..n_lesions), n_lesions,
        volumes_ml (voxels * voxel_volume / 1000), bboxes ([n,6] half-open z0, z1, y0, y1, x0, x1),
        lobes: {label: {voxels, lesion_voxels, ratio, ctss}} for every lobe label 1..255 present in `lobe`; ratio is the fp64
            quotient of the two integer counts of the filtered mask, ctss = inference.ratio_to_label(ratio);
    and with a `reference` mask: n_reference (its components under the same connectivity), n_found (those of them that the
    filtered mask touches), sensitivity (n_found / n_reference, NaN without reference lesions), n_false (kept components that do
    not touch the reference); and with `surface=True` on top of that: surface = `surface.surface_distances` of the filtered mask
    against the reference (Hausdorff distance, HD95, average symmetric surface distance, surface Dice at `tolerances_mm`);
    and with `scan` (int16 [D,H,W], Hounsfield units): density = {"lesions": `density.label_report` over the kept components,
    one row per lesion in the order of volumes_ml, "lobes": {label: {"parenchyma": the report row of the whole lobe, "lesion":
    that of the lobe's voxels inside the kept mask}}} at `percentiles_permille` and `band_edges_hu`.  Without `scan` nothing of
    that is computed and the result has no such key;
    and with `distribution=True`: distribution = `distribution.lesion_distribution` of the kept mask and its components (depth
    below the lung surface, peripheral share, centroids and positional zones per lobe, for both lungs and per lesion, "lesions"
    in the order of volumes_ml) at `depth`, `shells_mm`, `zones`, `box`, `percentiles_permille` and `subpleural_mm`.  Without
    the keyword nothing of that is computed and the result has no such key;
    and with `shape=True`: shape = `shape.lesion_shape` over the kept components (surface area, Euler number, sphericity,
    principal axes), one row per lesion in the order of volumes_ml.  Without the keyword nothing of that is computed and the
    result has no such key;
    and with `scan` and `texture=True` (the defaults of `texture.label_glcm`) or `texture=dict(levels=, lo=, width=, distance=)`:
    texture = {"lesions": `texture.lesion_texture` over the kept components (Haralick features of the grey-level co-occurrence
    tables), rows in the order of volumes_ml, "lobes": {label: {"parenchyma": the row of the whole lobe, "lesion": that of the
    lobe's voxels inside the kept mask}}}, the layout of `density`.  `texture` without `scan` is a ValueError.  Without the
    keyword nothing of that is computed and the result has no such key."""
    mask = _device_u8(mask)
    dev = mask.device
    if texture and scan is None:
        raise ValueError("lesion_report: texture needs the scan")
    if scan is not None:
        scan = torch.as_tensor(scan)
        if scan.dtype != torch.int16 or scan.shape != mask.shape:
            raise ValueError("lesion_report: scan must be an int16 [D,H,W] volume of the mask's shape")
    lobe = torch.as_tensor(lobe).to(device=dev, dtype=torch.uint8).contiguous()
    if mask.dim() != 3 or lobe.shape != mask.shape:
        raise ValueError("lesion_report: mask and lobe must be [D,H,W] volumes of the same shape")
    if reference is not None:
        reference = _device_u8(reference, dev)
        if reference.shape != mask.shape:
            raise ValueError("lesion_report: reference and mask must have the same shape")
    elif surface:
        raise ValueError("lesion_report: surface=True needs a reference mask")
    voxel_volume = float(np.prod(np.asarray(spacing, dtype=np.float64)))
    labels, n = label_components(mask, connectivity)
    stats = component_stats(labels, n, reference)
    keep = stats["voxels"].astype(np.float64) * voxel_volume >= float(min_volume_mm3)
    labels, n_kept, kept_mask = _relabel(labels, n, keep)
    voxels = stats["voxels"][keep]
    out = {"mask": kept_mask, "labels": labels, "n_lesions": n_kept, "volumes_ml": voxels.astype(np.float64) * voxel_volume / 1000.0,
           "bboxes": stats["bbox"][keep], "lobes": {}}
    counts = lobe_burden(kept_mask, lobe)
    for v in range(1, 256):
        total, set_ = int(counts[v, 0]), int(counts[v, 1])
        if total:
            ratio = float(np.float64(set_) / np.float64(total))
            out["lobes"][v] = {"voxels": total, "lesion_voxels": set_, "ratio": ratio, "ctss": ratio_to_label(ratio)}
    if reference is not None:
        ref_labels, n_ref = label_components(reference, connectivity)
        found = component_stats(ref_labels, n_ref, kept_mask)["hits"]
        n_found = int(np.count_nonzero(found))
        out.update(n_reference=n_ref, n_found=n_found, sensitivity=n_found / n_ref if n_ref else float("nan"),
                   n_false=int(np.count_nonzero(stats["hits"][keep] == 0)))
        if surface:
            out["surface"] = surface_distances(kept_mask, reference, spacing, tolerances_mm=tolerances_mm)
    if scan is not None:
        from .density import label_report, row_of
        scan = scan.to(dev).contiguous()
        kw = dict(percentiles_permille=percentiles_permille, band_edges_hu=band_edges_hu)
        lobes = {}
        if out["lobes"]:
            top = max(out["lobes"])
            whole, inside = label_report(scan, lobe, top, **kw), label_report(scan, lobe, top, mask=kept_mask, **kw)
            lobes = {v: {"parenchyma": row_of(whole, v - 1), "lesion": row_of(inside, v - 1)} for v in out["lobes"]}
        out["density"] = {"lesions": label_report(scan, labels, n_kept, **kw), "lobes": lobes}
    if distribution:
        from .distribution import lesion_distribution
        out["distribution"] = lesion_distribution(kept_mask, lobe, spacing, labels=labels, n=n_kept, depth=depth, shells_mm=shells_mm,
                                                  zones=zones, box=box, percentiles_permille=percentiles_permille,
                                                  subpleural_mm=subpleural_mm)
    if shape:
        from .shape import lesion_shape
        out["shape"] = lesion_shape(labels, n_kept, spacing)
    if texture:
        from .density import row_of
        from .texture import lesion_texture
        scan = scan.to(dev).contiguous()
        kw = {} if texture is True else dict(texture)
        if set(kw) - {"levels", "lo", "width", "distance"}:
            raise ValueError("lesion_report: texture takes levels, lo, width and distance")
        lobes = {}
        if out["lobes"]:
            top = max(out["lobes"])
            whole, inside = lesion_texture(scan, lobe, top, **kw), lesion_texture(scan, lobe, top, mask=kept_mask, **kw)
            lobes = {v: {"parenchyma": row_of(whole, v - 1), "lesion": row_of(inside, v - 1)} for v in out["lobes"]}
        out["texture"] = {"lesions": lesion_texture(scan, labels, n_kept, **kw), "lobes": lobes}
    return out
