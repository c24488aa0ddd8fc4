"""Pseudo-vessel mask on the device: Frangi's multi-scale Hessian vesselness, the producer of the `vessel` input of
`LobeInference.run` -- the reference reads that mask from a file per scan and does not say how the files were made.

    vessel = pseudo_vessel_mask(scan, lobe, spacing)                               # uint8 [D,H,W] on the device
    res = LobeInference(model).run(scan, lobe, spacing, vessel=pseudo_vessel_mask)  # or a functools.partial of it

Per scale s (mm): the scale-normalised Hessian of Gaussian (three separable passes), its eigenvalues by magnitude, the tube
measure V; then the maximum over scales and a threshold inside the lobes.  The bits are defined in include/dram_hip.h
(dram_hessian ...); kernels: csrc/vessel.hip.  Only the taps are made on the host, in fp64 with numpy alone.

`sigmas_mm`, `c` and `threshold` are stated defaults that nobody has tuned: there is no vessel ground truth to tune them on.
"""
import ctypes
import math

import numpy as np
import torch

from ._lib import call, lib
from .surface import _spacing, _stream, _volume

DEFAULT_SIGMAS_MM = (1.0, 1.5, 2.0, 3.0)
DEFAULT_CLIP = (-1150.0, 350.0)            # the reference's window (utils.py:189)
TRUNCATE = 4.0                             # scipy.ndimage.gaussian_filter1d's default


def gaussian_radius(sigma):
    return int(TRUNCATE * float(sigma) + 0.5)


def gaussian_derivative_taps(sigma, order, radius=None):
    """The impulse response of `scipy.ndimage.gaussian_filter1d(sigma=sigma, order=order, truncate=4.0)`: fp64, 2 * radius + 1
    values for the offsets -radius .. radius (radius = int(4 sigma + 0.5) unless given).  The sampled Gaussian is normalised to
    sum 1 and multiplied by the polynomial q_order(x) with (q phi)' = (q' - q x / sigma^2) phi; the same numpy operations as
    scipy's, so the same bits.  Pure host, no scipy."""
    sigma = float(sigma)
    if not (sigma > 0.0 and math.isfinite(sigma)):
        raise ValueError("gaussian_derivative_taps: sigma must be positive and finite")
    if order not in (0, 1, 2):
        raise ValueError("gaussian_derivative_taps: order 0, 1 or 2")
    radius = gaussian_radius(sigma) if radius is None else int(radius)
    if radius < 0:
        raise ValueError("gaussian_derivative_taps: radius must not be negative")
    sigma2 = sigma * sigma
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / sigma2 * x ** 2)
    phi = phi / phi.sum()
    if order == 0:
        return phi
    exponents = np.arange(order + 1)
    q = np.zeros(order + 1)
    q[0] = 1
    step = np.diag(exponents[1:], 1) + np.diag(np.ones(order) / -sigma2, -1)      # coefficients of q -> those of q' - q x / sigma^2
    for _ in range(order):
        q = step.dot(q)
    return (x[:, None] ** exponents).dot(q) * phi


def _scale_tables(spacing, sigma_mm, who):
    """(taps fp32 [3][3][max_radius + 1], radius [3], sv [3]) of one scale: taps[a][o][j] multiplies the sample at distance +j."""
    cap = lib.dram_vessel_max_radius()
    sigma_mm = float(sigma_mm)
    if not (sigma_mm > 0.0 and math.isfinite(sigma_mm)):
        raise ValueError(f"{who}: every scale must be a positive finite number of mm")
    sv = [sigma_mm / s for s in spacing]
    radius = [gaussian_radius(s) for s in sv]
    if max(radius) > cap:
        raise ValueError(f"{who}: scale {sigma_mm} mm at spacing {tuple(spacing)} needs a filter radius of {max(radius)} voxels; "
                         f"the kernels serve up to {cap}")
    taps = np.zeros((3, 3, cap + 1), dtype=np.float32)
    for a in range(3):
        for o in range(3):
            t = gaussian_derivative_taps(sv[a], o, radius[a])
            # filtering is a convolution with the impulse response: the sample at +j meets the response at -j
            taps[a, o, :radius[a] + 1] = t[radius[a]::-1].astype(np.float32)
    return taps, radius, sv


def _scan(scan, who):
    scan = _volume(scan, who)
    if scan.numel() == 0:
        raise ValueError(f"{who}: an empty volume")
    if not scan.is_cuda:
        scan = scan.to(torch.device("cuda", torch.cuda.current_device()))
    if scan.dtype != torch.int16:
        scan = scan.to(torch.float32)
    return scan.contiguous()


def _clip(clip, who):
    if clip is None:
        return -math.inf, math.inf
    lo, hi = float(clip[0]), float(clip[1])
    if not lo <= hi:
        raise ValueError(f"{who}: clip must be (lo, hi) with lo <= hi, or None")
    return lo, hi


def _sigmas(sigmas_mm, who):
    sig = [float(s) for s in np.asarray(sigmas_mm, dtype=np.float64).reshape(-1)]
    if not sig:
        raise ValueError(f"{who}: at least one scale")
    return sig


def _hessian_into(scan, tables, clip, h6, ws):
    taps, radius, sv = tables
    D, H, W = scan.shape
    taps_dev = torch.from_numpy(taps).to(scan.device)
    call("dram_hessian", scan.data_ptr(), 0 if scan.dtype == torch.int16 else 1, clip[0], clip[1], taps_dev.data_ptr(),
         (ctypes.c_int * 3)(*radius), (ctypes.c_double * 3)(*sv), D, H, W, h6.data_ptr(), ws.data_ptr(), ws.numel() * 4, _stream())


def hessian(scan, spacing, sigma_mm, clip=DEFAULT_CLIP):
    """[6,D,H,W] float32 on the device: the scale-normalised Hessian of Gaussian of a [D,H,W] volume (int16 HU, or anything
    else as float32) at the scale `sigma_mm` under the voxel spacing (z, y, x) in mm, in the order zz, yy, xx, zy, zx, yx.
    Voxels are clamped to `clip` on load (None: not at all)."""
    sp = _spacing(spacing, "hessian")
    scan = _scan(scan, "hessian")
    clip = _clip(clip, "hessian")
    tables = _scale_tables(sp, sigma_mm, "hessian")
    D, H, W = scan.shape
    with torch.cuda.device(scan.device):
        h6 = torch.empty((6, D, H, W), dtype=torch.float32, device=scan.device)
        ws = torch.empty(lib.dram_hessian_ws_bytes(D, H, W) // 4, dtype=torch.float32, device=scan.device)
        _hessian_into(scan, tables, clip, h6, ws)
    return h6


def _lobe_box(lobe, margin):
    """The bounding box of lobe > 0 grown by `margin` per axis and cut at the volume's edge, as slices; None without a lobe
    voxel.  x is widened to multiples of 4 where the volume allows, which keeps the rows of the crop 16-byte aligned."""
    D, H, W = lobe.shape
    boxes = torch.empty(255 * 6, dtype=torch.int32, device=lobe.device)
    call("dram_label_bboxes", lobe.data_ptr(), boxes.data_ptr(), 255, D, H, W, _stream())
    boxes = boxes.cpu().numpy().reshape(255, 6)                  # the one synchronisation
    present = boxes[:, 3] >= boxes[:, 0]
    if not present.any():
        return None
    lo = boxes[present, :3].min(axis=0)
    hi = boxes[present, 3:].max(axis=0) + 1
    start = [max(0, int(l) - m) for l, m in zip(lo, margin)]
    stop = [min(n, int(h) + m) for h, m, n in zip(hi, margin, (D, H, W))]
    start[2] -= start[2] % 4
    stop[2] = min(W, (stop[2] + 3) // 4 * 4)
    return tuple(slice(a, b) for a, b in zip(start, stop))


def vesselness(scan, spacing, sigmas_mm=DEFAULT_SIGMAS_MM, alpha=0.5, beta=0.5, c=None, clip=DEFAULT_CLIP, lobe=None):
    """Frangi's multi-scale vesselness of a [D,H,W] volume (int16 HU or float32) under the voxel spacing (z, y, x) in mm: float32
    [D,H,W] on the device, the maximum over `sigmas_mm` of the bright-tube measure V in [0, 1) of the scale-normalised Hessian.
    `c`: the structureness scale, a float, or None for Frangi's own rule (skimage's default): per scale half the largest
    Frobenius norm of the Hessian over the voxels with lobe > 0 (all voxels without a lobe map); it stays on the device.
    With `lobe` only the bounding box of lobe > 0, grown per axis by the largest filter radius, is computed: the values on lobe
    voxels are the whole-volume values bit for bit (`c` given; with c=None the whole-volume call takes its maximum over every
    voxel, so pass the lobe map there too), the voxels outside the box are 0.
    The default scales, c and alpha / beta are stated defaults that nobody has tuned: there is no vessel ground truth here."""
    who = "vesselness"
    sp = _spacing(spacing, who)
    scan = _scan(scan, who)
    clip = _clip(clip, who)
    alpha, beta = float(alpha), float(beta)
    if not (alpha > 0.0 and beta > 0.0 and math.isfinite(alpha) and math.isfinite(beta)):
        raise ValueError(f"{who}: alpha and beta must be positive and finite")
    if c is not None and not (float(c) > 0.0 and math.isfinite(float(c))):
        raise ValueError(f"{who}: c must be a positive finite number, or None")
    tables = [_scale_tables(sp, s, who) for s in _sigmas(sigmas_mm, who)]
    dev = scan.device
    with torch.cuda.device(dev):
        out = None
        if lobe is not None:
            lobe = _volume(lobe, who)
            if lobe.shape != scan.shape:
                raise ValueError(f"{who}: scan and lobe must have the same shape")
            lobe = lobe.to(device=dev, dtype=torch.uint8).contiguous()
            box = _lobe_box(lobe, [max(t[1][a] for t in tables) for a in range(3)])
            out = torch.zeros(scan.shape, dtype=torch.float32, device=dev)
            if box is None:
                return out
            scan, lobe = scan[box].contiguous(), lobe[box].contiguous()
        D, H, W = scan.shape
        S = D * H * W
        vmax = torch.empty((D, H, W), dtype=torch.float32, device=dev)
        h6 = torch.empty((6, D, H, W), dtype=torch.float32, device=dev)
        ws = torch.empty(lib.dram_hessian_ws_bytes(D, H, W) // 4, dtype=torch.float32, device=dev)
        c_dev = torch.full((1,), 1.0 if c is None else float(c), dtype=torch.float32, device=dev)
        for k, t in enumerate(tables):
            _hessian_into(scan, t, clip, h6, ws)
            if c is None:
                call("dram_hessian_norm_max", h6.data_ptr(), None if lobe is None else lobe.data_ptr(), S, c_dev.data_ptr(), _stream())
            call("dram_vesselness", h6.data_ptr(), S, alpha, beta, c_dev.data_ptr(), vmax.data_ptr(), int(k > 0), None, _stream())
        if out is None:
            return vmax
        out[box] = vmax
    return out


def vessel_mask(vmax, lobe, threshold):
    """uint8 [D,H,W] on the device: (vmax >= threshold) & (lobe > 0); lobe=None: no gate."""
    vmax = _volume(vmax, "vessel_mask")
    if not vmax.is_cuda or vmax.dtype != torch.float32:
        raise ValueError("vessel_mask: a float32 vesselness volume on the GPU")
    vmax = vmax.contiguous()
    if lobe is not None:
        lobe = _volume(lobe, "vessel_mask")
        if lobe.shape != vmax.shape:
            raise ValueError("vessel_mask: vmax and lobe must have the same shape")
        lobe = lobe.to(device=vmax.device, dtype=torch.uint8).contiguous()
    mask = torch.empty(vmax.shape, dtype=torch.uint8, device=vmax.device)
    if vmax.numel():
        with torch.cuda.device(vmax.device):
            call("dram_vessel_mask", vmax.data_ptr(), None if lobe is None else lobe.data_ptr(), float(threshold), mask.data_ptr(),
                 vmax.numel(), _stream())
    return mask


def pseudo_vessel_mask(scan, lobe, spacing, threshold=0.5, **kw):
    """The pseudo-vessel mask of a scan: uint8 [D,H,W] on the device, (vesselness(scan, spacing, lobe=lobe, **kw) >= threshold)
    & (lobe > 0).  Fits `LobeInference.run(..., vessel=)` as it is, or as a functools.partial with its keywords bound.
    `threshold`, like the scales and c of `vesselness`, is a stated default that nobody has tuned: no vessel ground truth."""
    if not math.isfinite(float(threshold)):
        raise ValueError("pseudo_vessel_mask: threshold must be finite")
    lobe = _volume(lobe, "pseudo_vessel_mask")
    return vessel_mask(vesselness(scan, spacing, lobe=lobe, **kw), lobe, threshold)
