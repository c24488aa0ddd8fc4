"""The result contact sheet on the device: the screenshot that the reference's `archive_results` writes for every scan
(job_runner.py:897-904) through `draw_mask_tile_singleview_heatmap` (utils.py:542-620), and its contour twin
`draw_mask_tile_single_view` (utils.py:464-539).  Five slices through the findings: the windowed scan on top, below it one row
per list of layers, drawn over the scan through a colour map (or as filled masks / outlines).

    out = result_sheet(scan, [[pred], [post], [ref], [htp]], [pred, ref])
    out["sheet"]                       # uint8 [Hs, Ws, 3] on the device, RGB
    save_sheet(out["sheet"], "sheet.png")
    LobeInference(model).sheet(res, scan, lesion)

The reference zooms every whole volume with scipy to keep five planes of each.  Here one pass over the coordinate masks says
which planes the zoomed mask occupies (`dram_sheet_occupancy`), the host picks the slices from those flags (one small
read-back), and one launch renders the finished sheet from the planes it needs (`dram_sheet_render`).  Flip, zoom, pad, slice
choice, layout and the 8-bit sources are the reference's numpy / scipy arithmetic, reproduced exactly; the bits are defined in
include/dram_hip.h ("result contact sheet"), kernels: csrc/sheet.hip.

What is NOT the reference's, since OpenCV is not available to pin it against (the header marks it PARITY UNPINNED):
  * the colour maps are 256-entry tables from a closed form ("jet": clamp(1.5 - |4t - k|, 0, 1), "summer": (t, 0.5 + 0.5t, 0.4)),
    not OpenCV's tables, and the blend is defined in fp32 with round-half-even;
  * style="contour" paints filled masks (thickness -1) or, for thickness 1, the mask pixels that have a 4-neighbour outside the
    mask or outside the tile.  This is our own definition of an outline: it is NOT OpenCV's findContours / drawContours;
  * the sheet is in RGB order (the reference builds BGR for cv2.imwrite);
  * titles are not rasterised (cv2.putText's Hershey font is not reproduced): the titles and every tile's rectangle are
    returned so that a caller can annotate.
"""
import ctypes
import struct

import numpy as np
import torch

from ._lib import call

MAX_MASKS, MAX_ROWS, MAX_LAYERS, MAX_SLICES, MAX_W = 4, 8, 16, 16, 32768          # the DRAM_SHEET_MAX_* of include/dram_hip.h
_IMAGE_KINDS = {torch.int16: 0, torch.uint8: 1}
_LAYER_KINDS = {"mask": 2, "u8": 1, "unit": 3}
_STYLES = {"heatmap": 0, "contour": 1}
_COLORMAPS = {"jet": 0, "summer": 1}
_LAYER = struct.Struct("@Pii4B4x")                                                # dram_sheet_layer
DEFAULT_COLORS = ((255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0))


def _int(v, name, who, lo=None):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or (lo is not None and v < lo):
        raise ValueError(f"{who}: {name} must be an integer" + ("" if lo is None else f" >= {lo}"))
    return int(v)


def _axes(shape, zoom_size, coord_axis, flip_axis, who):
    try:
        shape = tuple(int(v) for v in shape)
    except TypeError:
        raise ValueError(f"{who}: shape must be (D, H, W)") from None
    if len(shape) != 3 or min(shape) < 1 or shape[0] * shape[1] * shape[2] >= 1 << 31:
        raise ValueError(f"{who}: a [D,H,W] volume of 1 .. 2^31 - 1 voxels")
    if coord_axis not in (0, 1, 2) or isinstance(coord_axis, bool):
        raise ValueError(f"{who}: coord_axis must be 0, 1 or 2")
    if flip_axis is not None and (flip_axis not in (0, 1, 2) or isinstance(flip_axis, bool)):
        raise ValueError(f"{who}: flip_axis must be None, 0, 1 or 2")
    if zoom_size is not None:
        zoom_size = _int(zoom_size, "zoom_size", who, 1)
    return shape, zoom_size


def zoomed_extents(shape, zoom_size, coord_axis):
    """(za, zb): the extents of a plane after the zoom, round(n * zoom_size / max(n_a, n_b)) with Python's round, as
    ndimage.zoom forms them; the raw extents for zoom_size=None.  ValueError for an extent of 0."""
    shape, zoom_size = _axes(shape, zoom_size, coord_axis, None, "zoomed_extents")
    a, b = [d for d in range(3) if d != coord_axis]
    if zoom_size is None:
        return shape[a], shape[b]
    ratio = zoom_size / max(shape[a], shape[b])
    z = int(round(shape[a] * ratio)), int(round(shape[b] * ratio))
    if min(z) < 1:
        raise ValueError(f"zoomed_extents: a plane of {shape[a]} x {shape[b]} zooms to {z[0]} x {z[1]} at zoom_size {zoom_size}")
    return z


def sheet_layout(shape, n_rows, num_slices=5, zoom_size=360, coord_axis=1, sheet_width=1920):
    """Where everything lies on the sheet of a [D,H,W] volume with `n_rows` rendered rows: a dict with
      "height", "width"   the sheet is uint8 [height, width, 3]
      "tile"              (th, tw): zoom_size x zoom_size, or the raw plane for zoom_size=None
      "zoomed", "pad"     the zoomed plane (za, zb) and the zeros in front of it inside a tile
      "left"              the zero columns on the left, (sheet_width - num_slices * tw) // 2 (0 for sheet_width=None)
      "tiles"             tiles[r][j] = (y0, x0, th, tw) of row r (0: the grey row) and slice j
    ValueError when the tiles are wider than `sheet_width` (the reference's np.pad refuses the negative width)."""
    who = "sheet_layout"
    shape, zoom_size = _axes(shape, zoom_size, coord_axis, None, who)
    n_rows, num_slices = _int(n_rows, "n_rows", who, 1), _int(num_slices, "num_slices", who, 1)
    za, zb = zoomed_extents(shape, zoom_size, coord_axis)
    th, tw = (za, zb) if zoom_size is None else (zoom_size, zoom_size)
    cur = num_slices * tw
    if sheet_width is None:
        width = cur
    else:
        width = _int(sheet_width, "sheet_width", who, 1)
        if cur > width:
            raise ValueError(f"{who}: {num_slices} tiles of width {tw} do not fit a sheet of width {width}")
    left = (width - cur) // 2
    return {"height": (1 + n_rows) * th, "width": width, "tile": (th, tw), "zoomed": (za, zb), "pad": ((th - za) // 2, (tw - zb) // 2),
            "left": left, "tiles": [[(r * th, left + j * tw, th, tw) for j in range(num_slices)] for r in range(1 + n_rows)]}


def pick_slices(flags, num_slices=5):
    """The reference's slice choice (utils.py:579-592) from the per-plane flags of the zoomed coordinate mask: None when no plane is
    occupied ("no object found!"); else with s, e the first and one-past-last occupied plane and stride = (e - s) // num_slices
    -- or, when that is 0, s, e = 0, extent - 1 -- the first num_slices of range(s, e, stride).  ValueError when the stride is
    still 0 (the reference dies in range())."""
    num_slices = _int(num_slices, "num_slices", "pick_slices", 1)
    flags = np.asarray(flags.cpu() if isinstance(flags, torch.Tensor) else flags).reshape(-1)
    occupied = np.flatnonzero(flags)
    if occupied.size == 0:
        return None
    s, e = int(occupied[0]), int(occupied[-1]) + 1
    stride = (e - s) // num_slices
    if stride == 0:
        s, e = 0, int(flags.size) - 1
        stride = (e - s) // num_slices
    if stride == 0:
        raise ValueError(f"pick_slices: {flags.size} planes are too few for {num_slices} slices")
    return list(range(s, e, stride))[:num_slices]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _volume(v, who, what):
    if not isinstance(v, torch.Tensor):
        raise ValueError(f"{who}: {what} must be a torch tensor on the GPU")
    if v.dim() != 3:
        raise ValueError(f"{who}: {what} must be a [D,H,W] volume")
    return v


def _on_device(who, tensors):
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError(f"{who}: tensor is on {t.device}; the sheet kernels only run on a ROCm device (there is no CPU "
                               f"fallback)")
    if any(t.device != tensors[0].device for t in tensors):
        raise RuntimeError(f"{who}: all tensors must be on one device")


def _mask_u8(m, who, what):
    if m.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f"{who}: {what} must be uint8 (non-zero = set) or bool")
    m = m.contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else m


def sheet_occupancy(coord_mask, flip_axis=0, zoom_size=360, coord_axis=1):
    """int32 [extent along coord_axis] on the device: 1 where that plane of the flipped, order-0 zoomed coordinate mask holds a
    non-zero voxel.  coord_mask: a uint8 / bool [D,H,W] device tensor or a list of up to 4, ORed on load."""
    who = "sheet_occupancy"
    masks = list(coord_mask) if isinstance(coord_mask, (list, tuple)) else [coord_mask]
    if not 1 <= len(masks) <= MAX_MASKS:
        raise ValueError(f"{who}: 1 .. {MAX_MASKS} coordinate masks")
    masks = [_volume(m, who, "coord_mask") for m in masks]
    shape, zoom_size = _axes(masks[0].shape, zoom_size, coord_axis, flip_axis, who)
    if any(tuple(m.shape) != shape for m in masks):
        raise ValueError(f"{who}: the coordinate masks must have one shape")
    if shape[2] > MAX_W:
        raise ValueError(f"{who}: W must not exceed {MAX_W}")
    zoomed_extents(shape, zoom_size, coord_axis)
    masks = [_mask_u8(m, who, "coord_mask") for m in masks]
    _on_device(who, masks)
    dev = masks[0].device
    with torch.cuda.device(dev):
        flags = torch.empty(shape[coord_axis], dtype=torch.int32, device=dev)
        ptrs = (ctypes.c_void_p * len(masks))(*[m.data_ptr() for m in masks])
        call("dram_sheet_occupancy", ptrs, len(masks), *shape, coord_axis, -1 if flip_axis is None else flip_axis, zoom_size or 0,
             flags.data_ptr(), _stream())
    return flags


def _layer(entry, who):
    """(tensor, kind name): a layer is a tensor or (tensor, "mask" | "u8" | "unit"); by default float32 is "unit", else "mask"."""
    if isinstance(entry, (tuple, list)):
        if len(entry) != 2:
            raise ValueError(f"{who}: a layer is a tensor or (tensor, kind)")
        t, kind = entry
    else:
        t, kind = entry, None
    t = _volume(t, who, "a layer")
    if kind is None:
        kind = "unit" if t.dtype == torch.float32 else "mask"
    if kind not in _LAYER_KINDS:
        raise ValueError(f"{who}: a layer's kind is one of {tuple(_LAYER_KINDS)}")
    if kind == "unit":
        if t.dtype != torch.float32:
            raise ValueError(f"{who}: a 'unit' layer must be float32")
        return t.contiguous(), kind
    if kind == "u8" and t.dtype != torch.uint8:
        raise ValueError(f"{who}: a 'u8' layer must be uint8")
    return _mask_u8(t, who, f"a '{kind}' layer"), kind


def result_sheet(image, rows, coord_mask, num_slices=5, style="heatmap", alpha=0.5, flip_axis=0, zoom_size=360, coord_axis=1,
                 colormap="jet", colors=None, thickness=None, window=(-1150, 350), sheet_width=1920, titles=None):
    """The contact sheet of `image` (int16 HU, windowed by `window` to 8 bits on load as `windowing(scan).astype(uint8)` does; or
    uint8, taken as it is) with one rendered row per entry of `rows`, at `num_slices` slices through `coord_mask`.  All tensors are
    [D,H,W] on one GPU.

    rows: a list of rows; a row is a list of layers (a single layer may stand for its list); a layer is a tensor or (tensor, kind):
      "mask"  uint8 / bool, 255 where non-zero (the default for every dtype but float32)
      "u8"    uint8, used as it is
      "unit"  float32 through windowing(h, (0, 1)) to 8 bits, NaN -> 0 (the default for float32)
    coord_mask: a uint8 / bool tensor or a list of up to 4 to be ORed; the slices are chosen as the reference chooses them, from the
      planes that the ZOOMED mask occupies (`pick_slices`).
    style "heatmap" (draw_2d_heatmap): every layer of a row is blended over the scan through `colormap` ("jet" | "summer";
      anything else raises NotImplementedError, like the reference) with weight `alpha`.
    style "contour" (draw_2d): layer i of a row is painted with colors[i] (RGB) -- filled for thickness[i] == -1, its outline for
      1 -- and the painted tile blended with the scan.  See the module docstring: this outline is NOT OpenCV's contour.
    flip_axis None | 0 | 1 | 2, zoom_size None | int, coord_axis 0 | 1 | 2, sheet_width None | int as in the reference (its 1920).

    Returns None when coord_mask is empty (the reference prints "no object found!"), else a dict: "sheet" (uint8 [Hs, Ws, 3] on
    the device, RGB), "slice_ids" (planes of the flipped volume, as the reference counts them), "tiles" (tiles[r][j] = (y0, x0, h,
    w); row 0 is the scan) and "titles" (one per rendered row, not drawn).
    RuntimeError for tensors that are not on the GPU; ValueError for every other refusal."""
    who = "result_sheet"
    image = _volume(image, who, "image")
    if image.dtype not in _IMAGE_KINDS:
        raise ValueError(f"{who}: image must be int16 (HU) or uint8")
    shape, zoom_size = _axes(image.shape, zoom_size, coord_axis, flip_axis, who)
    num_slices = _int(num_slices, "num_slices", who, 1)
    if num_slices > MAX_SLICES:
        raise ValueError(f"{who}: up to {MAX_SLICES} slices")
    if style not in _STYLES:
        raise ValueError(f"{who}: style must be 'heatmap' or 'contour'")
    if style == "heatmap" and colormap not in _COLORMAPS:
        raise NotImplementedError(f"{who}: colormap {colormap!r}; 'jet' and 'summer' are served")
    alpha = float(alpha)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"{who}: alpha must lie in [0, 1]")
    try:
        wmin, wmax = window
        wmin, wmax = _int(wmin, "window", who), _int(wmax, "window", who)
    except TypeError:
        raise ValueError(f"{who}: window must be two integers (lo, hi) in HU") from None
    if not (-32768 <= wmin < wmax <= 32767 and wmax - wmin <= 32767):
        raise ValueError(f"{who}: window must satisfy -32768 <= lo < hi <= 32767 with hi - lo <= 32767 (the reference's int16 "
                         f"arithmetic)")
    if not isinstance(rows, (list, tuple)) or not 1 <= len(rows) <= MAX_ROWS:
        raise ValueError(f"{who}: rows must be a list of 1 .. {MAX_ROWS} rows")
    rows = [[_layer(e, who) for e in (row if isinstance(row, list) else [row])] for row in rows]
    flat = [l for row in rows for l in row]
    if any(not row for row in rows) or len(flat) > MAX_LAYERS:
        raise ValueError(f"{who}: every row needs a layer, and all rows together hold up to {MAX_LAYERS}")
    if any(tuple(t.shape) != shape for t, _ in flat):
        raise ValueError(f"{who}: every layer must have the image's shape {shape}")
    width = max(len(row) for row in rows)
    if style == "contour":
        colors = DEFAULT_COLORS if colors is None else colors
        thickness = [-1] * width if thickness is None else thickness
        try:
            colors = [tuple(_int(c, "a colour channel", who) for c in col) for col in colors]
            thickness = [_int(t, "thickness", who) for t in thickness]
        except TypeError:
            raise ValueError(f"{who}: colors is a list of (r, g, b), thickness a list of integers") from None
        if len(colors) < width or len(thickness) < width:
            raise ValueError(f"{who}: a row has {width} layers; colors and thickness must be at least that long")
        if any(len(c) != 3 or min(c) < 0 or max(c) > 255 for c in colors):
            raise ValueError(f"{who}: a colour is (r, g, b) in 0 .. 255")
        if any(t not in (-1, 1) for t in thickness):
            raise ValueError(f"{who}: thickness must be -1 (filled) or 1 (outline)")
    if titles is not None:
        titles = [str(t) for t in titles]
        if len(titles) != len(rows):
            raise ValueError(f"{who}: one title per row")
    layout = sheet_layout(shape, len(rows), num_slices, zoom_size, coord_axis, sheet_width)
    if layout["height"] > 65535 or layout["height"] * layout["width"] * 3 >= 1 << 31:
        raise ValueError(f"{who}: a sheet of {layout['height']} x {layout['width']} is too large")
    masks = list(coord_mask) if isinstance(coord_mask, (list, tuple)) else [coord_mask]
    if any(isinstance(m, torch.Tensor) and m.dim() == 3 and tuple(m.shape) != shape for m in masks):
        raise ValueError(f"{who}: coord_mask must have the image's shape {shape}")
    image = image.contiguous()
    _on_device(who, [image] + [t for t, _ in flat] + [m for m in masks if isinstance(m, torch.Tensor)])
    flags = sheet_occupancy(masks, flip_axis, zoom_size, coord_axis)
    ids = pick_slices(flags, num_slices)                         # the one read-back: an int per plane
    if ids is None:
        return None
    dev = image.device
    table = bytearray()
    for row in rows:
        for i, (t, kind) in enumerate(row):
            color, thick = (colors[i], thickness[i]) if style == "contour" else ((0, 0, 0), -1)
            table += _LAYER.pack(t.data_ptr(), _LAYER_KINDS[kind], thick, *color, 0)
    table = (ctypes.c_char * len(table)).from_buffer(table)
    with torch.cuda.device(dev):
        sheet = torch.empty((layout["height"], layout["width"], 3), dtype=torch.uint8, device=dev)
        call("dram_sheet_render", image.data_ptr(), _IMAGE_KINDS[image.dtype], wmin, wmax, ctypes.addressof(table),
             (ctypes.c_int * len(rows))(*[len(row) for row in rows]), len(rows), (ctypes.c_int * num_slices)(*ids), num_slices, *shape,
             coord_axis, -1 if flip_axis is None else flip_axis, zoom_size or 0, layout["width"] if sheet_width is not None else 0,
             _STYLES[style], _COLORMAPS.get(colormap, 0), alpha, sheet.data_ptr(), _stream())
    return {"sheet": sheet, "slice_ids": ids, "tiles": layout["tiles"], "titles": titles}


def save_sheet(sheet, path):
    """Write a uint8 [H, W, 3] RGB sheet (a tensor on any device, or an array) to `path`: through PIL when it imports (the format
    follows the extension), else as a binary PPM (P6) with the standard library alone, whatever the extension says.  Returns the
    format written: "pil" or "ppm"."""
    arr = sheet.detach().cpu().numpy() if isinstance(sheet, torch.Tensor) else np.asarray(sheet)
    if arr.ndim != 3 or arr.shape[2] != 3 or arr.dtype != np.uint8:
        raise ValueError("save_sheet: a uint8 [H, W, 3] sheet")
    arr = np.ascontiguousarray(arr)
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        Image.fromarray(arr, "RGB").save(path)
        return "pil"
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (arr.shape[1], arr.shape[0]))
        f.write(arr.tobytes())
    return "ppm"
