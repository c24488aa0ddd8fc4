"""dram_sheet_occupancy and dram_sheet_render through the C ABI on guard-banded buffers against the numpy restatement
(tests/sheet_restatement.py).  Every output is an integer: equality is demanded everywhere.

Shapes.  (37, 21, 53) at zoom_size 64 and (21, 37, 19) zoom up on every coord axis (W odd: the byte path of the occupancy pass);
(36, 22, 52) at zoom_size 24 zooms down (rows, planes and bytes that the zoom skips) with W % 4 == 0 (the word path); zoom_size
None is the raw plane; (70, 9, 530) at the defaults' 360 / 1920 puts eight blocks on a sheet row."""
import ctypes
import functools
import struct

import numpy as np
import pytest
import torch

import sheet_restatement as S
from gpu_buffers import DEV, Placed, stream

pytestmark = pytest.mark.gpu

KIND = {S.MASK: 2, S.U8: 1, S.UNIT: 3}
LAYER = struct.Struct("@Pii4B4x")
WINDOW = (-1150, 350)


def placed(arr, shift=0):
    t = torch.from_numpy(np.array(arr))                         # a writable, contiguous copy
    return Placed(tuple(arr.shape), shift, dtype=t.dtype, src=t)


def occupancy_c(masks, ca, flip, zoom, shift=0):
    from dram_amd import _lib
    shape = masks[0].shape
    bufs = [placed(m, shift) for m in masks]
    flags = placed(np.full(shape[ca], -7, dtype=np.int32))
    ptrs = (ctypes.c_void_p * len(bufs))(*[b.t.data_ptr() for b in bufs])
    _lib.call("dram_sheet_occupancy", ptrs, len(bufs), *shape, ca, -1 if flip is None else flip, zoom or 0, flags.t.data_ptr(), stream())
    torch.cuda.synchronize()
    assert flags.intact() and all(b.intact() for b in bufs)
    return flags.t.cpu().numpy()


def render_c(image, rows, ids, style="heatmap", alpha=0.5, flip=0, zoom=360, ca=1, colormap="jet", colors=None, thickness=None,
             width=1920):
    from dram_amd import _lib
    from dram_amd.sheet import sheet_layout
    shape = image.shape
    lay = sheet_layout(shape, len(rows), len(ids), zoom, ca, width)
    img = placed(image, 2 if image.dtype == np.int16 else 1)
    bufs, table = [], bytearray()
    for row in rows:
        for i, (v, kind) in enumerate(row):
            b = placed(v, 4 if kind == S.UNIT else 3)
            bufs.append(b)
            color, thick = (colors[i], thickness[i]) if style == "contour" else ((9, 9, 9), 5)     # read by the contour style only
            table += LAYER.pack(b.t.data_ptr(), KIND[kind], thick, *color, 0)
    table = (ctypes.c_char * len(table)).from_buffer(table)
    out = Placed((lay["height"], lay["width"], 3), 1, dtype=torch.uint8)
    _lib.call("dram_sheet_render", img.t.data_ptr(), 0 if image.dtype == np.int16 else 1, *WINDOW, ctypes.addressof(table),
              (ctypes.c_int * len(rows))(*[len(r) for r in rows]), len(rows), (ctypes.c_int * len(ids))(*ids), len(ids), *shape, ca,
              -1 if flip is None else flip, zoom or 0, 0 if width is None else width, {"heatmap": 0, "contour": 1}[style],
              {"jet": 0, "summer": 1}[colormap], alpha, out.t.data_ptr(), stream())
    torch.cuda.synchronize()
    assert out.intact() and img.intact() and all(b.intact() for b in bufs)
    return out.t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def volumes(shape):
    """Shared, never modified: an int16 scan beyond the window on both sides, a sparse mask with values 0 / 1 / 3, a uint8 layer,
    a float32 layer with NaN, values below 0 and above 1, and two coordinate masks that leave the first and last planes empty."""
    g = np.random.default_rng(sum(shape))
    scan = g.integers(-1500, 700, size=shape).astype(np.int16)
    mask = (g.integers(0, 6, size=shape) == 0).astype(np.uint8) * g.choice(np.array([1, 3], dtype=np.uint8), size=shape)
    u8 = g.integers(0, 256, size=shape).astype(np.uint8)
    unit = g.uniform(-0.2, 1.2, size=shape).astype(np.float32)
    unit.reshape(-1)[g.choice(unit.size, size=unit.size // 20, replace=False)] = np.nan
    unit.reshape(-1)[:4] = (np.inf, -np.inf, 1.0, -0.0)
    assert np.isnan(unit).any() and (unit < 0).any() and (unit > 1).any()
    c1 = np.zeros(shape, dtype=np.uint8)
    c2 = np.zeros(shape, dtype=np.uint8)
    inner = tuple(slice(2, n - 1) for n in shape)
    c1[inner] = g.integers(0, 40, size=c1[inner].shape) == 0
    c2[inner] = (g.integers(0, 40, size=c2[inner].shape) == 0) * 200
    for v in (scan, mask, u8, unit, c1, c2):
        v.setflags(write=False)
    return scan, mask, u8, unit, c1, c2


CONFIGS = [((37, 21, 53), 64), ((21, 37, 19), 64), ((36, 22, 52), 24), ((37, 21, 53), None), ((21, 37, 19), None)]


@pytest.mark.parametrize("flip", [None, 0, 1, 2])
@pytest.mark.parametrize("ca", [0, 1, 2])
@pytest.mark.parametrize("shape,zoom", CONFIGS)
def test_occupancy_and_heatmap_sheet(shape, zoom, ca, flip):
    scan, mask, u8, unit, c1, c2 = volumes(shape)
    want = S.occupancy(c1 | c2, flip, zoom, ca)
    flags = occupancy_c([c1, c2], ca, flip, zoom)
    assert np.array_equal(flags, want)
    assert want.any() and not want.all()
    ids = S.pick_slices(want, 5)
    rows = [[(mask, S.MASK)], [(u8, S.U8), (unit, S.UNIT)]]
    tw = zoom or shape[[d for d in range(3) if d != ca][1]]
    width = 5 * tw + 7                                           # an odd room: 3 columns on the left, 4 on the right
    got = render_c(scan, rows, ids, flip=flip, zoom=zoom, ca=ca, width=width)
    ref = S.sheet(scan, rows, ids, flip_axis=flip, zoom_size=zoom, coord_axis=ca, window=WINDOW, sheet_width=width)
    assert got.shape == ref.shape and np.array_equal(got, ref)
    assert ref[ref.shape[0] // 3:].any() and len(np.unique(ref)) > 50


def test_occupancy_word_path_and_misaligned_masks_agree():
    shape = (36, 22, 52)
    _, _, _, _, c1, c2 = volumes(shape)
    for ca in range(3):
        want = S.occupancy(c1 | c2, 0, 24, ca)
        for shift in (0, 1):                                     # 0: words; 1: the masks are not 4-byte aligned, bytes
            assert np.array_equal(occupancy_c([c1, c2], ca, 0, 24, shift), want)
    four = [np.where(np.arange(36)[:, None, None] % 4 == k, c1, 0).astype(np.uint8) for k in range(4)]
    assert np.array_equal(occupancy_c(four, 1, None, 24), S.occupancy(c1, None, 24, 1))


@pytest.mark.parametrize("ca", [0, 1, 2])
def test_occupancy_follows_the_zoomed_mask(ca):
    """Single-voxel planes: one voxel at a source index that the nearest down-zoom reads, one at an index it skips, along each of
    the two tile axes.  The indices come from the restated map."""
    shape, zoom = (36, 22, 52), 24
    a, b = S.other_axes(ca)
    zs = S.zoomed_shape(shape, zoom, ca)
    read = {d: set(S.nearest_index(shape[d], zs[d])[~S.outside(shape[d], zs[d])].tolist()) for d in (a, b)}
    skip = {d: sorted(set(range(shape[d])) - read[d]) for d in (a, b)}
    assert skip[a] and skip[b]
    hit = {d: sorted(read[d])[len(read[d]) // 2] for d in (a, b)}
    cases = {3: (hit[a], hit[b]), 7: (hit[a], skip[b][1]), 11: (skip[a][1], hit[b]), 15: (skip[a][0], skip[b][0])}
    m = np.zeros(shape, dtype=np.uint8)
    for plane, (ia, ib) in cases.items():
        at = [0, 0, 0]
        at[ca], at[a], at[b] = plane, ia, ib
        m[tuple(at)] = 1
    want = S.occupancy(m, None, zoom, ca)
    assert want[3] == 1 and want[7] == 0 and want[11] == 0 and want[15] == 0 and want.sum() == 1     # the two cases differ
    assert np.array_equal(occupancy_c([m], ca, None, zoom), want)
    for flip in range(3):
        assert np.array_equal(occupancy_c([m], ca, flip, zoom), S.occupancy(m, flip, zoom, ca))
    # a mask confined to one plane: stride 0, the fallback to the whole extent
    from dram_amd.sheet import pick_slices
    ids = pick_slices(occupancy_c([m], ca, None, zoom), 5)
    n = shape[ca]
    assert ids == list(range(0, n - 1, (n - 1) // 5))[:5] == S.pick_slices(want, 5)
    assert pick_slices(occupancy_c([np.zeros(shape, dtype=np.uint8)], ca, None, zoom), 5) is None


@pytest.mark.parametrize("colormap", ["jet", "summer"])
@pytest.mark.parametrize("alpha", [0.5, 0.3])
def test_heatmap_styles(colormap, alpha):
    shape = (37, 21, 53)
    scan, mask, u8, unit, _, _ = volumes(shape)
    ids = [3, 9, 10, 15, 20]
    for rows in ([[(unit, S.UNIT)], [(u8, S.U8)], [(mask, S.MASK)]], [[(mask, S.MASK), (unit, S.UNIT)]]):
        got = render_c(scan, rows, ids, alpha=alpha, zoom=64, colormap=colormap, width=None)
        ref = S.sheet(scan, rows, ids, alpha=alpha, zoom_size=64, colormap=colormap, window=WINDOW, sheet_width=None)
        assert np.array_equal(got, ref)
    u8_image = render_c(u8, [[(mask, S.MASK)]], ids, alpha=alpha, zoom=64, colormap=colormap, width=None)
    assert np.array_equal(u8_image, S.sheet(u8, [[(mask, S.MASK)]], ids, alpha=alpha, zoom_size=64, colormap=colormap, sheet_width=None))


@functools.lru_cache(maxsize=None)
def contour_masks(shape):
    """A slab that reaches the volume's faces along axes 0 and 2 (the tile's edge wherever the zoomed extent fills the tile) with
    one-voxel holes, and a second, smaller box inside it."""
    m1 = np.zeros(shape, dtype=np.uint8)
    m1[:, 4:15, :] = 1
    m1[::5, 5:14:3, 3::7] = 0
    m1[3, 9, 10] = 0
    m2 = np.zeros(shape, dtype=np.uint8)
    m2[6:20, 7:12, 10:30] = 2
    m1.setflags(write=False)
    m2.setflags(write=False)
    return m1, m2


@pytest.mark.parametrize("zoom,ca", [(64, 1), (None, 1), (64, 0), (24, 2)])
@pytest.mark.parametrize("thickness", [(-1, -1), (1, 1), (-1, 1)])
def test_contour_style(zoom, ca, thickness):
    shape = (37, 21, 53)
    scan = volumes(shape)[0]
    m1, m2 = contour_masks(shape)
    ids = [5, 6, 9, 10, 13] if ca == 1 else [3, 4, 10, 15, 20]
    colors = [(255, 10, 0), (0, 200, 255)]
    rows = [[(m1, S.MASK), (m2, S.MASK)], [(m2, S.U8)]]
    for alpha in (0.5, 0.3):
        got = render_c(scan, rows, ids, style="contour", alpha=alpha, flip=0, zoom=zoom, ca=ca, colors=colors, thickness=thickness,
                       width=None)
        ref = S.sheet(scan, rows, ids, style="contour", alpha=alpha, flip_axis=0, zoom_size=zoom, coord_axis=ca, colors=colors,
                      thickness=thickness, window=WINDOW, sheet_width=None)
        assert np.array_equal(got, ref)
    if ca == 1:                                                  # the restated outline on these planes: edge pixels and hole rims
        plane = S.prepare(m1, 0, 0, zoom, ca)[:, 5]
        edge = S.outline(plane)
        assert edge[:, 0].any() or edge[0].any()                 # the mask touches the tile's edge and is outlined there
        assert (edge & (plane != 0)).sum() < (plane != 0).sum()  # and has an interior that an outline leaves unpainted


def test_more_than_one_block_per_sheet_row():
    shape = (70, 9, 530)
    g = np.random.default_rng(5)
    scan = g.integers(-1300, 500, size=shape).astype(np.int16)
    htp = g.random(size=shape, dtype=np.float32)
    pred = (htp > 0.8).astype(np.uint8)
    pred[:, 0] = 0
    want = S.occupancy(pred, 0, 360, 1)
    assert np.array_equal(occupancy_c([pred], 1, 0, 360), want)
    ids = S.pick_slices(want, 5)
    assert ids == [1, 2, 3, 4, 5]
    rows = [[(pred, S.MASK)], [(htp, S.UNIT)]]
    got = render_c(scan, rows, ids)
    ref = S.sheet(scan, rows, ids, window=WINDOW)
    assert got.shape == (3 * 360, 1920, 3) and np.array_equal(got, ref)
    assert not ref[:, :60].any() and not ref[:, 1860:].any() and ref[:, 60:1860].any()


def test_result_sheet_wrapper():
    """dram_amd.sheet.result_sheet on device tensors: the same sheet, the slice ids, the rectangles and the titles."""
    from dram_amd import result_sheet, sheet_layout
    shape = (37, 21, 53)
    scan, mask, u8, unit, c1, c2 = volumes(shape)
    d = lambda v: torch.from_numpy(np.array(v)).to(DEV)
    out = result_sheet(d(scan), [d(mask) != 0, [(d(u8), "u8"), d(unit)]], [d(c1), d(c2)], zoom_size=64, sheet_width=400, titles=["a", "b"])
    ids = S.pick_slices(S.occupancy(c1 | c2, 0, 64, 1), 5)
    assert out["slice_ids"] == ids and out["titles"] == ["a", "b"]
    ref = S.sheet(scan, [[(mask, S.MASK)], [(u8, S.U8), (unit, S.UNIT)]], ids, zoom_size=64, sheet_width=400)
    assert out["sheet"].is_cuda and np.array_equal(out["sheet"].cpu().numpy(), ref)
    assert out["tiles"] == sheet_layout(shape, 2, 5, 64, 1, 400)["tiles"]
    y0, x0, h, w = out["tiles"][0][2]
    grey = np.take(S.prepare(S.image_u8(scan, WINDOW), 1, 0, 64, 1), ids[2], axis=1)
    assert np.array_equal(ref[y0:y0 + h, x0:x0 + w, 1], grey)
    assert result_sheet(d(scan), [d(mask)], torch.zeros(shape, dtype=torch.uint8, device=DEV), zoom_size=64) is None
    with pytest.raises(ValueError):                              # one occupied plane of 4: no stride
        result_sheet(d(scan)[:4], [d(mask)[:4]], d(c1)[:4] * 0 + 1, coord_axis=0, zoom_size=64)
