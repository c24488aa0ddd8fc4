"""Surface-distance metrics on the device: what a consumer of a predicted lesion mask and its reference otherwise does on the
host with `scipy.ndimage.distance_transform_edt` over two whole volumes -- Hausdorff distance, its percentile (HD95), average
symmetric surface distance and surface Dice at a tolerance (NSD).

    m = surface_distances(res["mask_post"], reference, spacing, tolerances_mm=(1.0, 2.0))
    m["hd95"], m["assd"], m["nsd"][1.0]

Kernels: csrc/distance.hip (exact Euclidean distance transform with anisotropic spacing in three separable fp64 passes, the
6-neighbour surface of a mask, compaction of a distance map over a surface).  `torch.sort` / `torch.searchsorted` order the
compacted distances; only counts and a few order statistics travel to the host.
"""
import math

import numpy as np
import torch

from ._lib import call, lib


def _device_u8(v, device=None):
    v = torch.as_tensor(v)
    if device is None:
        device = v.device if v.is_cuda else torch.device("cuda", torch.cuda.current_device())
    if v.dtype != torch.uint8:
        v = v != 0
    return v.to(device=device, dtype=torch.uint8).contiguous()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _spacing(spacing, who):
    sp = np.asarray(spacing, dtype=np.float64).reshape(-1)
    if sp.shape != (3,) or not np.all(np.isfinite(sp)) or not np.all(sp > 0):
        raise ValueError(f"{who}: spacing must be three positive finite numbers (z, y, x) in mm")
    return [float(s) for s in sp]


def _volume(v, who):
    v = torch.as_tensor(v)
    if v.dim() != 3:
        raise ValueError(f"{who}: a [D,H,W] volume")
    return v


def distance_transform(feature, spacing):
    """The exact Euclidean distance transform of a [D,H,W] feature mask (non-zero = feature): float32 on the device, the distance
    in mm under `spacing` (z, y, x) from every voxel to the nearest feature -- 0 on a feature, +inf everywhere when there is
    none.  `scipy.ndimage.distance_transform_edt(feature == 0, sampling=spacing)` up to fp64 rounding; the bits are defined in
    include/dram_hip.h (dram_edt)."""
    sp = _spacing(spacing, "distance_transform")
    feature = _device_u8(_volume(feature, "distance_transform"))
    D, H, W = feature.shape
    dist = torch.empty((D, H, W), dtype=torch.float32, device=feature.device)
    if feature.numel() == 0:
        return dist
    with torch.cuda.device(feature.device):
        ws_bytes = lib.dram_edt_ws_bytes(D, H, W)
        ws = torch.empty(max(ws_bytes, 8) // 8, dtype=torch.float64, device=feature.device)
        call("dram_edt", feature.data_ptr(), dist.data_ptr(), *sp, D, H, W, ws.data_ptr(), ws_bytes, _stream())
    return dist


def mask_surface(mask):
    """(surf, n): the voxels of a [D,H,W] mask with a face neighbour that is unset or outside the volume, as a uint8 device
    volume, and their number (a Python int; reading it is the one synchronisation)."""
    mask = _device_u8(_volume(mask, "mask_surface"))
    surf = torch.empty_like(mask)
    if mask.numel() == 0:
        return surf, 0
    count = torch.empty(1, dtype=torch.int64, device=mask.device)
    with torch.cuda.device(mask.device):
        call("dram_mask_surface", mask.data_ptr(), surf.data_ptr(), count.data_ptr(), *mask.shape, _stream())
    return surf, int(count.item())


def gather_surface(surf, dist, n):
    """dist over the `n` set voxels of `surf` as a dense float32 device vector, in no particular order."""
    if surf.shape != dist.shape or surf.dtype != torch.uint8 or dist.dtype != torch.float32 or not (surf.is_cuda and dist.is_cuda):
        raise ValueError("gather_surface: a uint8 surface and a float32 distance map of the same shape on the GPU")
    out = torch.empty(int(n), dtype=torch.float32, device=surf.device)
    if surf.numel() == 0:
        return out
    surf, dist = surf.contiguous(), dist.contiguous()
    cursor = torch.empty(1, dtype=torch.int64, device=surf.device)
    with torch.cuda.device(surf.device):
        call("dram_surface_gather", surf.data_ptr(), dist.data_ptr(), out.data_ptr() if n else None, cursor.data_ptr(), int(n),
             surf.numel(), _stream())
    return out


def percentile_position(n, q):
    """numpy's default (linear) percentile of n sorted values: (lo, hi, t) with the result lerp(v[lo], v[hi], t)."""
    if n < 1 or not 0.0 <= q <= 100.0:
        raise ValueError("percentile: n >= 1 values and 0 <= q <= 100")
    pos = (q / 100.0) * (n - 1)
    lo = min(int(math.floor(pos)), n - 1)
    return lo, min(lo + 1, n - 1), pos - lo


def percentile_lerp(a, b, t):
    """numpy's _lerp in fp64: a + (b - a) * t below t = 0.5, b - (b - a) * (1 - t) from there."""
    a, b, t = float(a), float(b), float(t)
    if a == b:                           # also inf - inf
        return a
    return b - (b - a) * (1.0 - t) if t >= 0.5 else a + (b - a) * t


def _float32_at_most(v):
    """The largest float32 that does not exceed v: a float32 d has d <= v exactly when d <= that."""
    f = np.float32(v)
    return float(f if float(f) <= v else np.nextafter(f, np.float32(-np.inf)))


def _percentile_name(q):
    return "hd" + (str(int(q)) if float(q) == int(q) else str(float(q)))


def surface_distances(pred, ref, spacing, percentile=95.0, tolerances_mm=()):
    """Boundary metrics of a predicted [D,H,W] mask against a reference mask under the voxel spacing (z, y, x) in mm.  With A the
    distances from every surface voxel of `pred` to the nearest surface voxel of `ref` and B the other way round:
        hd: max(max A, max B);  hd<percentile> (e.g. "hd95"): numpy's default linear-interpolation percentile of A and B together,
        in fp64 from the two neighbouring order statistics;  assd: (sum A + sum B) / (|A| + |B|) with fp64 sums;
        nsd: {tol: (entries of A and B that are <= tol) / (|A| + |B|)} for every tolerance;  n_pred_surface = |A|, n_ref_surface = |B|.
    Both masks empty: NaN everywhere.  Exactly one empty: hd, the percentile and assd are inf, every nsd 0."""
    sp = _spacing(spacing, "surface_distances")
    if not 0.0 <= float(percentile) <= 100.0:
        raise ValueError("surface_distances: percentile must be in 0 .. 100")
    tols = [float(t) for t in tolerances_mm]
    if any(not t >= 0.0 for t in tols):
        raise ValueError("surface_distances: tolerances must be non-negative")
    pred, ref = _volume(pred, "surface_distances"), _volume(ref, "surface_distances")
    if ref.shape != pred.shape:
        raise ValueError("surface_distances: pred and ref must have the same shape")
    pred = _device_u8(pred)
    ref = _device_u8(ref, pred.device)
    name = _percentile_name(percentile)
    surf_p, n_p = mask_surface(pred)
    surf_r, n_r = mask_surface(ref)
    out = {"n_pred_surface": n_p, "n_ref_surface": n_r}
    if n_p == 0 or n_r == 0:
        both = n_p == 0 and n_r == 0
        bad = float("nan") if both else float("inf")
        out.update({"hd": bad, name: bad, "assd": bad, "nsd": {t: float("nan") if both else 0.0 for t in tols}})
        return out
    a = gather_surface(surf_p, distance_transform(surf_r, sp), n_p)
    b = gather_surface(surf_r, distance_transform(surf_p, sp), n_r)
    # every metric is symmetric in A and B, so one sort of both together serves all of them
    n = n_p + n_r
    both, _ = torch.sort(torch.cat((a, b)))
    lo, hi, t = percentile_position(n, float(percentile))
    parts = [torch.stack((both[-1], both[lo], both[hi])).double(), both.sum(dtype=torch.float64).reshape(1)]
    if tols:
        bounds = torch.tensor([_float32_at_most(tol) for tol in tols], dtype=torch.float32, device=both.device)
        parts.append(torch.searchsorted(both, bounds, right=True).double())
    host = torch.cat(parts).cpu().numpy()          # the one read-back
    out.update({"hd": float(host[0]), name: percentile_lerp(host[1], host[2], t), "assd": float(host[3] / n),
                "nsd": {tol: float(host[4 + k]) / n for k, tol in enumerate(tols)}})
    return out
