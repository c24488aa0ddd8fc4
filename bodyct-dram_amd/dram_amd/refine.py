"""Edge-aware refinement of the heat map on the device: the masked 3-D guided filter (He, Sun and Tang), guided by the scan
and restricted to the lung.  The reference has no such step: its heat map reaches the scan's grid by a trilinear resize of an
80^3 chunk, and the only place the CT informs the mask is the global brightness gate.

    q = refine_heatmap(res["htp"], scan, lobe, spacing)                     # float32 [D,H,W] on the device
    res = LobeInference(model, refine=True).run(scan, lobe, spacing, lesion=lesion, curves=256)
    res["curves"]["dice_best"], res["curves_refined"]["dice_best"]          # the effect, measured on the user's own labels

The bits are defined in include/dram_hip.h ("heat-map refinement"); kernels: csrc/guided.hip.

`radius_mm`, `eps` and the window are stated defaults that nobody has tuned, and whether the step improves any metric on real
scans has not been measured: there are no labelled scans here.  `refine=` together with `curves=` is how a user measures it.
"""
import ctypes
import math

import numpy as np
import torch

from ._lib import call, lib
from .surface import _spacing, _stream, _volume

DEFAULT_WINDOW = (-1150.0, 350.0)          # the reference's window (utils.py:189), as in `vessels`


def _radius(radius, who):
    try:
        r = [v for v in radius]
    except TypeError:
        raise ValueError(f"{who}: radius must be three integers (rz, ry, rx) in voxels") from None
    if len(r) != 3 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in r):
        raise ValueError(f"{who}: radius must be three integers (rz, ry, rx) in voxels")
    cap = lib.dram_guided_max_radius()
    if min(r) < 0 or max(r) > cap:
        raise ValueError(f"{who}: radius {tuple(int(v) for v in r)} is outside 0 .. {cap} voxels")
    return [int(v) for v in r]


def _eps(eps, who):
    eps = float(eps)
    if not (eps > 0.0 and math.isfinite(eps)):
        raise ValueError(f"{who}: eps must be positive and finite")
    return eps


def _window(window, who):
    try:
        lo, hi = float(window[0]), float(window[1])
    except (TypeError, IndexError):
        raise ValueError(f"{who}: window must be (lo, hi) in HU") from None
    if not (math.isfinite(lo) and math.isfinite(hi) and hi > lo):
        raise ValueError(f"{who}: window must be finite with hi > lo")
    return lo, hi


def _check(p, guide, mask, window, who):
    """The tensors as the C call takes them, and the window (None for a float32 guide); nothing is moved to the device."""
    p, guide, mask = _volume(p, who), _volume(guide, who), _volume(mask, who)
    if not (p.shape == guide.shape == mask.shape):
        raise ValueError(f"{who}: p, guide and mask must have the same shape")
    if p.numel() == 0 or p.numel() >= 1 << 31:
        raise ValueError(f"{who}: a volume of 1 .. 2^31 - 1 voxels")
    if p.dtype != torch.float32:
        raise ValueError(f"{who}: p must be float32")
    if mask.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f"{who}: mask must be uint8 (nonzero = inside) or bool")
    if guide.dtype == torch.int16:
        if window is None:
            raise ValueError(f"{who}: an int16 guide needs window=(lo, hi)")
        window = _window(window, who)
    elif guide.dtype == torch.float32:
        if window is not None:
            raise ValueError(f"{who}: a float32 guide is taken as it is; window must be None")
    else:
        raise ValueError(f"{who}: guide must be int16 (HU) or float32")
    return p, guide, mask, window


def _on_device(who, *tensors):
    dev = tensors[0].device
    if any(not t.is_cuda or t.device != dev for t in tensors):
        raise ValueError(f"{who}: p, guide and mask must be on one GPU")


def _filter_into(p, guide, mask, radius, eps, window, q, ab, ws):
    D, H, W = p.shape
    lo, hi = window if window is not None else (0.0, 1.0)
    call("dram_guided_filter", guide.data_ptr(), 0 if guide.dtype == torch.int16 else 1, lo, hi, p.data_ptr(), mask.data_ptr(),
         (ctypes.c_int * 3)(*radius), eps, D, H, W, q.data_ptr(), None if ab is None else ab.data_ptr(), ws.data_ptr(),
         ws.numel() * 8, _stream())


def _workspace(shape, dev):
    return torch.empty(lib.dram_guided_ws_bytes(*shape) // 8, dtype=torch.float64, device=dev)


def guided_filter(p, guide, mask, radius, eps, window=None, return_ab=False):
    """The masked 3-D guided filter of `p` (float32 [D,H,W]) under the guide (int16 HU, windowed on load to [0, 1] by `window` =
    (lo, hi); or float32, taken as it is, window=None) inside `mask` (uint8, nonzero = inside): float32 [D,H,W], 0 outside the
    mask.  radius: (rz, ry, rx) in voxels, each 0 .. dram_guided_max_radius(); eps > 0.  All three tensors on one GPU.
    return_ab: also the coefficients a, b of the filter's step 2 as float64 [2,D,H,W], 0 outside the mask.
    Raises ValueError for whatever `dram_guided_filter` would refuse."""
    who = "guided_filter"
    p, guide, mask, window = _check(p, guide, mask, window, who)
    radius = _radius(radius, who)
    eps = _eps(eps, who)
    _on_device(who, p, guide, mask)
    p, guide, mask = p.contiguous(), guide.contiguous(), mask.contiguous()
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    with torch.cuda.device(p.device):
        q = torch.empty(p.shape, dtype=torch.float32, device=p.device)
        ab = torch.empty((2, *p.shape), dtype=torch.float64, device=p.device) if return_ab else None
        _filter_into(p, guide, mask, radius, eps, window, q, ab, _workspace(p.shape, p.device))
    return (q, ab) if return_ab else q


def radius_voxels(radius_mm, spacing):
    """(rz, ry, rx) = max(1, round(radius_mm / spacing)) per axis, Python's round (halves to the even neighbour); raises
    ValueError when that exceeds dram_guided_max_radius()."""
    who = "refine_heatmap"
    sp = _spacing(spacing, who)
    radius_mm = float(radius_mm)
    if not (radius_mm > 0.0 and math.isfinite(radius_mm)):
        raise ValueError(f"{who}: radius_mm must be positive and finite")
    r = [max(1, round(radius_mm / s)) for s in sp]
    cap = lib.dram_guided_max_radius()
    if max(r) > cap:
        raise ValueError(f"{who}: {radius_mm} mm at spacing {tuple(sp)} is a radius of {max(r)} voxels; the kernels serve up to {cap}")
    return r


def refine_heatmap(htp, scan, lobe, spacing, radius_mm=3.0, eps=1e-3, window=DEFAULT_WINDOW, iterations=1):
    """The heat map refined by the guided filter inside the lung: float32 [D,H,W] on the device, 0 where lobe == 0.
    htp: float32 [D,H,W]; scan: int16 HU (windowed by `window` on load) or float32 (window=None); lobe: the uint8 label map, the
    region is lobe > 0; spacing (z, y, x) in mm.  The radius is `radius_voxels(radius_mm, spacing)`.  iterations=k feeds the
    result back in as the input k - 1 times.  Only the bounding box of lobe > 0 (x widened to multiples of 4) is filtered:
    nothing outside the region contributes, so the values are those of the whole-volume `guided_filter` bit for bit.
    `radius_mm`, `eps` and `window` are stated defaults that nobody has tuned, and whether refinement improves a metric on real
    scans has not been measured here."""
    who = "refine_heatmap"
    from .vessels import _lobe_box
    htp, scan, lobe, window = _check(htp, scan, lobe, window, who)
    if lobe.dtype != torch.uint8:
        raise ValueError(f"{who}: lobe must be the uint8 label map")
    radius = radius_voxels(radius_mm, spacing)
    eps = _eps(eps, who)
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or iterations < 1:
        raise ValueError(f"{who}: iterations must be a positive integer")
    _on_device(who, htp, scan, lobe)
    dev = htp.device
    with torch.cuda.device(dev):
        lobe = lobe.contiguous()
        out = torch.zeros(htp.shape, dtype=torch.float32, device=dev)
        box = _lobe_box(lobe, (0, 0, 0))
        if box is None:
            return out
        p, g, m = htp[box].contiguous(), scan[box].contiguous(), lobe[box].contiguous()
        ws = _workspace(p.shape, dev)
        for _ in range(int(iterations)):
            q = torch.empty(p.shape, dtype=torch.float32, device=dev)
            _filter_into(p, g, m, radius, eps, window, q, None, ws)
            p = q
        out[box] = p
    return out
