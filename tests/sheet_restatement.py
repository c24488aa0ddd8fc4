"""The result contact sheet in plain numpy, written from the text of include/dram_hip.h ("result contact sheet"), not from the
kernels: flip, zoom (order 0 and order 1), pad, slice choice, layout, the 8-bit sources and the two drawing styles.  Host code
only.  tests/test_sheet_cpu.py holds the zoom against scipy.ndimage.zoom and the slice choice against the reference's lines;
the GPU tests demand equality with `sheet` here."""
import numpy as np

MASK, U8, UNIT = "mask", "u8", "unit"


# ------------------------------------------------------------------------------------------------ step 2: zoom
def other_axes(coord_axis):
    return [d for d in range(3) if d != coord_axis]


def zoomed_shape(shape, zoom_size, coord_axis):
    """The extents after the zoom: round-half-even(n * ratio) along the two tile axes, n along coord_axis."""
    if zoom_size is None:
        return tuple(shape)
    ratio = zoom_size / max(shape[d] for d in other_axes(coord_axis))
    return tuple(shape[d] if d == coord_axis else int(round(shape[d] * ratio)) for d in range(3))


def coordinates(n, zn):
    """c[o] = o * step, step = (n - 1) / (zn - 1) rounded before the product; 0 when zn == 1."""
    if zn == 1:
        return np.zeros(1, dtype=np.float64)
    step = np.float64(n - 1) / np.float64(zn - 1)
    return np.arange(zn, dtype=np.float64) * step


def outside(n, zn):
    """ndimage.zoom's mode is "constant": an output index whose coordinate exceeds n - 1 (by the rounding of o * step; only the
    last index can) reads the constant 0."""
    return coordinates(n, zn) > n - 1


def nearest_index(n, zn):
    return np.minimum(np.floor(coordinates(n, zn) + 0.5).astype(np.int64), n - 1)


def _blank(w, d, out):
    if out.any():
        index = [slice(None)] * w.ndim
        index[d] = out
        w[tuple(index)] = 0
    return w


def zoom_nearest(v, out_shape):
    """Order 0 over every axis (the identity where out_shape equals the extent)."""
    for d in range(v.ndim):
        if out_shape[d] != v.shape[d]:
            v = _blank(np.take(v, nearest_index(v.shape[d], out_shape[d]), axis=d), d, outside(v.shape[d], out_shape[d]))
    return v


def zoom_linear_u8(v, out_shape):
    """Order 1 on uint8: a separable fp64 lerp, axis 0 first, v0 * (1 - t) + v1 * t, cast as floor(v + 0.5)."""
    w = v.astype(np.float64)
    for d in range(v.ndim):
        n, zn = v.shape[d], out_shape[d]
        if zn == n:
            continue                                             # t = 0: v0 * 1 + v1 * 0 = v0
        c = coordinates(n, zn)
        i0 = np.minimum(np.floor(c).astype(np.int64), n - 1)
        i1 = np.minimum(i0 + 1, n - 1)
        t = c - i0
        bshape = [1] * v.ndim
        bshape[d] = zn
        t = t.reshape(bshape)
        w = _blank(np.take(w, i0, axis=d) * (1.0 - t) + np.take(w, i1, axis=d) * t, d, outside(n, zn))
    return np.floor(w + 0.5).astype(np.uint8)


def pad_tile_axes(v, zoom_size, coord_axis):
    """Step 3: zeros to zoom_size along the two tile axes, (t - z) // 2 in front."""
    pad = [(0, 0) if d == coord_axis else ((zoom_size - z) // 2, zoom_size - z - (zoom_size - z) // 2) for d, z in enumerate(v.shape)]
    return np.pad(v, pad, mode="constant")


def prepare(v, order, flip_axis, zoom_size, coord_axis):
    """Steps 1-3 on one uint8 / bool volume."""
    if flip_axis is not None:
        v = np.flip(v, axis=flip_axis)
    if zoom_size is None:
        return v
    zs = zoomed_shape(v.shape, zoom_size, coord_axis)
    if min(zs) == 0:
        raise ValueError("a zoomed extent of 0")
    z = zoom_linear_u8(v, zs) if order == 1 else zoom_nearest(v, zs)
    return pad_tile_axes(z, zoom_size, coord_axis)


# ------------------------------------------------------------------------------------------------ step 4: slice choice
def occupancy(coord_mask, flip_axis, zoom_size, coord_axis):
    """flag[k]: plane k of the flipped, zoomed coordinate mask holds a non-zero voxel."""
    m = prepare(np.asarray(coord_mask) != 0, 0, flip_axis, zoom_size, coord_axis)
    return m.any(axis=tuple(other_axes(coord_axis))).astype(np.int32)


def pick_slices(flags, num_slices):
    flags = np.asarray(flags)
    nz = np.flatnonzero(flags)
    if nz.size == 0:
        return None
    s, e = int(nz[0]), int(nz[-1]) + 1
    stride = (e - s) // num_slices
    if stride == 0:
        s, e = 0, flags.size - 1
        stride = (e - s) // num_slices
    if stride == 0:
        raise ValueError("too few planes")
    return list(range(s, e, stride))[:num_slices]


# ------------------------------------------------------------------------------------------------ step 6: 8-bit sources
def windowing(image, from_span, to_span=(0, 255)):
    """The reference's windowing (utils.py:189-198) for a given span: clip, subtract, divide by the span as a Python float, scale
    to to_span -- in numpy's own types, which is the point: int16 and float32 inputs keep theirs up to the division."""
    lo, hi = from_span
    unit = (np.clip(image, lo, hi) - lo) / float(hi - lo)
    return unit * (to_span[1] - to_span[0]) + to_span[0]


def image_u8(image, window):
    image = np.asarray(image)
    if image.dtype == np.uint8:
        return image
    assert image.dtype == np.int16
    return windowing(image, window).astype(np.uint8)


def layer_u8(layer, kind):
    layer = np.asarray(layer)
    if kind == MASK:
        return ((layer != 0) * 255).astype(np.uint8)
    if kind == U8:
        assert layer.dtype == np.uint8
        return layer
    assert kind == UNIT and layer.dtype == np.float32
    w = windowing(np.where(np.isnan(layer), np.float32(0), layer), (0, 1))
    assert w.dtype == np.float32                                 # numpy stays in fp32 here
    return w.astype(np.uint8)


# ------------------------------------------------------------------------------------------------ step 7: drawing
def colormap_table(name):
    t = np.arange(256, dtype=np.float64) / 255.0
    if name == "jet":
        c = np.stack([np.clip(1.5 - np.abs(4.0 * t - k), 0.0, 1.0) for k in (3.0, 2.0, 1.0)], axis=1)
    elif name == "summer":
        c = np.stack([t, 0.5 + 0.5 * t, np.full(256, 0.4)], axis=1)
    else:
        raise NotImplementedError(name)
    return np.rint(255.0 * c).astype(np.uint8)


def blend(x, y, alpha):
    """sat(rne(x * a + y * b)) in fp32 with a = (float)alpha, b = (float)(1.0 - alpha)."""
    a, b = np.float32(alpha), np.float32(1.0 - float(alpha))
    p, q = np.asarray(x).astype(np.float32) * a, np.asarray(y).astype(np.float32) * b
    s = p + q
    assert s.dtype == np.float32
    return np.clip(np.rint(s), 0, 255).astype(np.uint8)


def draw_heatmap(grey, layers, alpha, colormap):
    table = colormap_table(colormap)
    value = np.dstack((grey, grey, grey))
    for layer in layers:
        value = blend(table[layer], value, alpha)
    return value


def outline(mask):
    """Mask pixels with a 4-neighbour that is zero or outside the tile."""
    m = np.pad(mask != 0, 1, mode="constant")
    inner = m[:-2, 1:-1] & m[2:, 1:-1] & m[1:-1, :-2] & m[1:-1, 2:]
    return (mask != 0) & ~inner


def draw_contour(grey, layers, alpha, colors, thickness):
    original = np.dstack((grey, grey, grey))
    painted = original.copy()
    for layer, color, thick in zip(layers, colors, thickness):
        if thick not in (-1, 1):
            raise ValueError("thickness")
        where = (layer != 0) if thick == -1 else outline(layer)
        painted[where] = np.asarray(color, dtype=np.uint8)
    return blend(painted, original, alpha)


# ------------------------------------------------------------------------------------------------ the sheet
def default_kind(layer):
    return UNIT if np.asarray(layer).dtype == np.float32 else MASK


def sheet(image, rows, slice_ids, style="heatmap", alpha=0.5, flip_axis=0, zoom_size=360, coord_axis=1, colormap="jet", colors=None,
          thickness=None, window=(-1150, 350), sheet_width=1920):
    """uint8 [Hs, Ws, 3] in RGB order for the given slice ids.  rows: lists of (array, kind)."""
    img = prepare(image_u8(image, window), 1, flip_axis, zoom_size, coord_axis)
    prepared = [[prepare(layer_u8(v, kind), 0, flip_axis, zoom_size, coord_axis) for v, kind in row] for row in rows]
    columns = []
    for sid in slice_ids:
        grey = np.take(img, sid, axis=coord_axis)
        tiles = [np.dstack((grey, grey, grey))]
        for row in prepared:
            planes = [np.take(v, sid, axis=coord_axis) for v in row]
            if style == "heatmap":
                tiles.append(draw_heatmap(grey, planes, alpha, colormap))
            else:
                tiles.append(draw_contour(grey, planes, alpha, colors, thickness))
        columns.append(np.vstack(tiles))
    out = np.hstack(columns)
    if sheet_width is not None:
        room = sheet_width - out.shape[1]
        out = np.pad(out, ((0, 0), (room // 2, room - room // 2), (0, 0)), mode="constant")
    return out
