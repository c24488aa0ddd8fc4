"""The numpy restatement of the contact sheet (tests/sheet_restatement.py) against scipy.ndimage -- the reference's own geometry
-- and the reference's lines, and everything of dram_amd/sheet.py and the C ABI that answers without a GPU."""
import ctypes
import os
import struct
import sys

import numpy as np
import pytest
import torch

import sheet_restatement as S

SHAPES = [(37, 5, 53), (61, 4, 29), (7, 40, 33), (23, 31, 6)]
ZOOMS = [16, 24, 64, 100]                                        # below and above every extent


def _ratio(shape, zoom, ca):
    r = zoom / max(shape[d] for d in S.other_axes(ca))
    return [1.0 if d == ca else r for d in range(3)]


@pytest.mark.parametrize("ca", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_zoom_is_ndimage_zoom(shape, ca):
    """Order 0 (bool and uint8): equal.  Order 1: within one grey level (scipy sums the eight weighted corners, the header lerps
    axis by axis).  Zoom up and zoom down; the blanked last index of scipy's "constant" mode occurs among the cases."""
    from scipy import ndimage
    g = np.random.default_rng(shape[0])
    v = g.integers(0, 256, size=shape).astype(np.uint8)
    m = g.integers(0, 5, size=shape) == 0
    seen = 0
    for zoom in ZOOMS:
        zs = S.zoomed_shape(shape, zoom, ca)
        if min(zs) == 0:
            continue
        seen += 1
        ratio = _ratio(shape, zoom, ca)
        for vol in (m, v):
            ref = ndimage.zoom(vol, ratio, order=0)
            assert ref.shape == zs and np.array_equal(ref, S.zoom_nearest(vol, zs)), (zoom, vol.dtype)
        ref = ndimage.zoom(v, ratio, order=1)
        err = np.abs(ref.astype(np.int64) - S.zoom_linear_u8(v, zs)).max()
        print(f"{shape} coord_axis {ca} zoom {zoom}: order 1 differs by at most {err} grey level(s)")
        assert err <= 1
    assert seen >= 3


def test_constant_mode_blanks_the_last_index_in_scipy_too():
    from scipy import ndimage
    assert S.outside(53, 100)[-1] and not S.outside(53, 100)[:-1].any() and not S.outside(512, 360).any()
    v = np.full((3, 53), 200, dtype=np.uint8)
    for order in (0, 1):
        out = ndimage.zoom(v, [1.0, 100 / 53], order=order)
        assert out.shape == (3, 100) and not out[:, -1].any() and out[:, :-1].all()
    assert not S.zoom_nearest(v, (3, 100))[:, -1].any() and not S.zoom_linear_u8(v, (3, 100))[:, -1].any()


def _scipy_prepare(v, order, flip_axis, zoom_size, coord_axis):
    """Flip, ndimage.zoom and the centred zero pad of utils.py:547-577, through scipy itself."""
    from scipy import ndimage
    if flip_axis is not None:
        v = v[tuple(slice(None, None, -1) if d == flip_axis else slice(None) for d in range(3))]
    if zoom_size is None:
        return v
    longest = max(n for d, n in enumerate(v.shape) if d != coord_axis)
    z = ndimage.zoom(v, [1.0 if d == coord_axis else zoom_size / longest for d in range(3)], order=order)
    assert all(n <= zoom_size for d, n in enumerate(z.shape) if d != coord_axis)          # the reference's crop never cuts
    out = np.zeros([n if d == coord_axis else zoom_size for d, n in enumerate(z.shape)], dtype=z.dtype)
    out[tuple(slice(None) if d == coord_axis else slice((zoom_size - n) // 2, (zoom_size - n) // 2 + n) for d, n in enumerate(z.shape))] = z
    return out


@pytest.mark.parametrize("flip", [None, 0, 1, 2])
def test_prepare_and_occupancy_are_the_reference_lines(flip):
    from scipy import ndimage
    g = np.random.default_rng(11)
    shape = (23, 31, 6)
    m = np.zeros(shape, dtype=bool)
    m[4:17, 6:20, 1:5] = g.integers(0, 9, size=(13, 14, 4)) == 0
    for ca in range(3):
        for zoom in (16, 64, None):
            ref = _scipy_prepare(m, 0, flip, zoom, ca)
            assert np.array_equal(ref, S.prepare(m, 0, flip, zoom, ca))
            flags = S.occupancy(m, flip, zoom, ca)
            sl = ndimage.find_objects(ref.astype(np.uint8))[0][ca]
            occupied = np.flatnonzero(flags)
            assert (occupied[0], occupied[-1] + 1) == (sl.start, sl.stop)


def _scipy_slices(mask, axis, k):
    """The slice choice of utils.py:579-592 through scipy's find_objects; range() raises ValueError for a step of 0."""
    from scipy import ndimage
    if not mask.any():
        return None
    box = ndimage.find_objects(mask)[0][axis]
    first, stop = box.start, box.stop
    step = (stop - first) // k
    if step == 0:
        first, stop = 0, mask.shape[axis] - 1
        step = stop // k
    return list(range(first, stop, step))[:k]


def _mask_from_flags(flags):
    m = np.zeros((3, len(flags), 2), dtype=np.uint8)
    m[1, :, 1] = np.asarray(flags) != 0
    return m


@pytest.mark.parametrize("flags", [
    [0, 0, 1, 0, 1, 1, 0, 0, 1, 1, 1, 0, 1, 1, 0, 1, 1, 1, 1, 0, 0],           # wide, with gaps: stride 3
    [0, 1] + [1] * 27 + [0],                                                     # wide: stride 5, more than five candidates
    [0] * 9 + [1, 0, 1, 1] + [0] * 20,                                           # e - s = 4 < 5: the fallback, stride 6
    [0, 0, 0, 1, 0, 0, 0, 0],                                                    # one plane: the fallback, stride 1
    [1, 1, 1, 1, 1, 1],                                                          # e - s = 6: stride 1, no fallback
])
def test_pick_slices_is_the_reference_lines(flags):
    from dram_amd import pick_slices
    want = _scipy_slices(_mask_from_flags(flags), 1, 5)
    assert pick_slices(flags, 5) == want == S.pick_slices(flags, 5) and len(want) == 5
    assert pick_slices(torch.tensor(flags, dtype=torch.int32), 5) == want
    assert pick_slices(np.asarray(flags), 3) == _scipy_slices(_mask_from_flags(flags), 1, 3)


def test_pick_slices_refusals_and_empty():
    from dram_amd import pick_slices
    assert pick_slices([0] * 12, 5) is None and S.pick_slices([0] * 12, 5) is None
    assert _scipy_slices(_mask_from_flags([0] * 12), 1, 5) is None
    for flags in ([1, 1, 1, 1, 0], [0, 1, 0], [1], [0, 0, 1, 1, 0]):  # extent below num_slices + 1: stride 0 twice
        with pytest.raises(ValueError):
            _scipy_slices(_mask_from_flags(flags), 1, 5)           # the reference dies in range()
        with pytest.raises(ValueError):
            pick_slices(flags, 5)
        with pytest.raises(ValueError):
            S.pick_slices(flags, 5)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError):
            pick_slices([1, 1, 1], bad)


@pytest.mark.parametrize("shape,zoom,ca,width", [((30, 51, 40), 36, 1, 200), ((30, 51, 40), None, 0, 301), ((9, 8, 7), 12, 2, None),
                                                 ((300, 512, 512), 360, 1, 1920)])
def test_sheet_layout_is_vstack_hstack_pad(shape, zoom, ca, width):
    from dram_amd import sheet_layout
    n_rows, num = 3, 5
    lay = sheet_layout(shape, n_rows, num, zoom, ca, width)
    a, b = S.other_axes(ca)
    zs = S.zoomed_shape(shape, zoom, ca)
    assert lay["zoomed"] == (zs[a], zs[b])
    th, tw = lay["tile"]
    assert (th, tw) == ((zoom, zoom) if zoom else (shape[a], shape[b]))
    columns = []
    for j in range(num):
        tiles = [np.full((th, tw), 1 + r * num + j, dtype=np.int32) for r in range(1 + n_rows)]
        columns.append(np.vstack(tiles))
    draw = np.hstack(columns)
    if width is not None:
        room = width - draw.shape[1]
        draw = np.pad(draw, ((0, 0), (room // 2, room - room // 2)), mode="constant")
    assert draw.shape == (lay["height"], lay["width"])
    want = np.zeros_like(draw)
    for r, row in enumerate(lay["tiles"]):
        for j, (y0, x0, h, w) in enumerate(row):
            want[y0:y0 + h, x0:x0 + w] = 1 + r * num + j
    assert np.array_equal(want, draw)
    assert lay["left"] == lay["tiles"][0][0][1] and lay["pad"] == ((th - zs[a]) // 2, (tw - zs[b]) // 2)


def test_sheet_layout_refusals():
    from dram_amd import sheet_layout
    with pytest.raises(ValueError, match="do not fit"):
        sheet_layout((300, 512, 512), 4, 6, 360, 1, 1920)        # np.pad would be asked for a negative width
    for kw in (dict(shape=(3, 4)), dict(shape=(0, 4, 5)), dict(n_rows=0), dict(num_slices=0), dict(zoom_size=0), dict(zoom_size=2.5),
               dict(coord_axis=3), dict(sheet_width=0), dict(shape=(1, 1000, 1000), zoom_size=300, coord_axis=1)):
        a = {**dict(shape=(8, 9, 10), n_rows=2, num_slices=5, zoom_size=16, coord_axis=1, sheet_width=400), **kw}
        with pytest.raises(ValueError):
            sheet_layout(**a)


def test_colour_tables_follow_their_formulas():
    jet, summer = S.colormap_table("jet"), S.colormap_table("summer")
    assert jet.shape == summer.shape == (256, 3) and jet.dtype == np.uint8
    for i in range(256):
        t = i / 255.0
        for ch, k in enumerate((3, 2, 1)):
            assert jet[i, ch] == round(255 * min(max(1.5 - abs(4 * t - k), 0.0), 1.0))
        assert tuple(summer[i]) == (i, round(255 * (0.5 + 0.5 * t)), 102)
    assert tuple(jet[0]) == (0, 0, 128) and tuple(jet[255]) == (128, 0, 0) and tuple(jet[128])[1] == 255
    # on a ramp 255 c = 382.5 - |4 i - 255 k| is a tie in exact arithmetic: the entry is whatever the fp64 roundings of the stated
    # operations leave, which is why the header fixes their order
    assert {int(jet[64][1]), int(jet[191][1])} <= {128, 129}
    with pytest.raises(NotImplementedError):
        S.colormap_table("hot")


def test_blend_and_sources():
    assert S.blend(np.array([255, 0, 1, 3]), np.array([0, 255, 0, 0]), 0.5).tolist() == [128, 128, 0, 2]      # halves go to even
    assert S.blend(np.array([200]), np.array([100]), 0.3).tolist() == [130]
    scan = np.array([-2000, -1150, -1149, -400, 349, 350, 3000], dtype=np.int16)
    assert S.image_u8(scan, (-1150, 350)).tolist() == [0, 0, 0, 127, 254, 255, 255]
    unit = np.array([np.nan, -0.5, 0.0, 0.5, 1.0, 7.0, np.inf, 0.999], dtype=np.float32)
    assert S.layer_u8(unit, S.UNIT).tolist() == [0, 0, 0, 127, 255, 255, 255, 254]
    assert S.layer_u8(np.array([0, 1, 200], dtype=np.uint8), S.MASK).tolist() == [0, 255, 255]
    hole = np.ones((5, 6), dtype=np.uint8)
    hole[2, 3] = 0
    edge = S.outline(hole)
    assert edge[0].all() and edge[:, 0].all() and edge[-1].all() and edge[:, -1].all()       # outside the tile counts as outside
    assert edge[1, 3] and edge[3, 3] and edge[2, 2] and edge[2, 4] and not edge[2, 3] and not edge[1, 1] and not edge[1, 2]


def test_exports_and_abi():
    import dram_amd
    from dram_amd import _lib
    for name in ("sheet_layout", "pick_slices", "sheet_occupancy", "result_sheet", "save_sheet"):
        assert name in dram_amd.__all__ and callable(getattr(dram_amd, name))
    for name in ("dram_sheet_occupancy", "dram_sheet_render"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert _lib.lib.dram_abi_version() == 2
    from dram_amd.inference import LobeInference
    assert callable(LobeInference.sheet)
    from dram_amd import sheet
    assert sheet._LAYER.size == 24                               # sizeof(dram_sheet_layer)


def test_c_refusals_come_before_any_launch():
    from dram_amd._lib import lib
    q = 64                                                       # a dummy aligned pointer: nothing is launched
    masks = (ctypes.c_void_p * 1)(q)
    ok = dict(masks=masks, n=1, D=8, H=9, W=10, ca=1, flip=0, zoom=16, flags=q)
    for change in (dict(masks=None), dict(flags=None), dict(n=0), dict(n=5), dict(D=0), dict(D=2048, H=1024, W=1024), dict(W=32772, D=1, H=1),
                   dict(ca=3), dict(ca=-1), dict(flip=3), dict(flip=-2), dict(zoom=-1), dict(masks=(ctypes.c_void_p * 1)(None)),
                   dict(D=1, H=1000, W=1000, zoom=300)):
        a = {**ok, **change}
        assert lib.dram_sheet_occupancy(a["masks"], a["n"], a["D"], a["H"], a["W"], a["ca"], a["flip"], a["zoom"], a["flags"], None) != 0, change
    layer = struct.Struct("@Pii4B4x")
    one = lambda data=q, kind=2, thick=-1: ctypes.create_string_buffer(layer.pack(data, kind, thick, 1, 2, 3, 0), 24)
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    ok = dict(image=q, ikind=0, wmin=-1150, wmax=350, layers=one(), rl=ints(1), n_rows=1, ids=ints(0, 1, 2), ns=3, D=8, H=9, W=10, ca=1,
              flip=0, zoom=16, width=100, style=0, cmap=0, alpha=0.5, sheet=q)
    for change in (dict(image=None), dict(layers=None), dict(sheet=None), dict(ids=None), dict(rl=None), dict(ikind=2), dict(wmax=-1150),
                   dict(image=q + 1), dict(layers=one(data=0)), dict(layers=one(kind=0)), dict(layers=one(kind=3, data=q + 2)),
                   dict(style=2), dict(cmap=2), dict(style=1, layers=one(thick=2)), dict(style=1, layers=one(thick=0)),
                   dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float("nan")), dict(n_rows=0), dict(n_rows=9), dict(rl=ints(0)),
                   dict(rl=ints(17)), dict(ns=0), dict(ns=17), dict(ids=ints(0, 9, 2)), dict(ids=ints(-1, 1, 2)), dict(width=47),
                   dict(width=-1), dict(zoom=-2), dict(ca=3), dict(flip=5), dict(D=0)):
        a = {**ok, **change}
        rc = lib.dram_sheet_render(a["image"], a["ikind"], a["wmin"], a["wmax"], a["layers"], a["rl"], a["n_rows"], a["ids"], a["ns"],
                                   a["D"], a["H"], a["W"], a["ca"], a["flip"], a["zoom"], a["width"], a["style"], a["cmap"], a["alpha"],
                                   a["sheet"], None)
        assert rc != 0, change


def test_wrapper_refusals():
    from dram_amd import result_sheet, sheet_occupancy
    shape = (8, 9, 10)
    scan, m, h = torch.zeros(shape, dtype=torch.int16), torch.ones(shape, dtype=torch.uint8), torch.zeros(shape)
    ok = dict(image=scan, rows=[[m], [h]], coord_mask=m)
    bad = [
        dict(image=scan.float()), dict(image=scan[0]), dict(image=scan.numpy()), dict(rows=[]), dict(rows=[[]]), dict(rows=[[m]] * 9),
        dict(rows=[[m] * 17]), dict(rows=[[m[:4]]]), dict(rows=[[(m, "unit")]]), dict(rows=[[(h, "u8")]]), dict(rows=[[(h, "mask")]]),
        dict(rows=[[(m, "heat")]]), dict(rows=[[(m, "mask", 1)]]), dict(rows=[[m.numpy()]]), dict(rows=m),
        dict(num_slices=0), dict(num_slices=17), dict(num_slices=2.0), dict(style="filled"), dict(alpha=-0.1), dict(alpha=1.01),
        dict(alpha=float("nan")), dict(flip_axis=3), dict(flip_axis=-1), dict(coord_axis=None), dict(coord_axis=3), dict(zoom_size=0),
        dict(zoom_size=16.0), dict(window=(350, -1150)), dict(window=(0, 0)), dict(window=(-40000, 0)), dict(window=(-20000, 20000)),
        dict(window=(0.0, 1.0)), dict(window=5), dict(sheet_width=79), dict(sheet_width=0), dict(titles=["one"]),
        dict(coord_mask=m[:4]), dict(style="contour", thickness=[2, 1]), dict(style="contour", thickness=[0, 1]),
        dict(style="contour", rows=[[m, m]], thickness=[1]), dict(style="contour", rows=[[m, m]], colors=[(1, 2, 3)]),
        dict(style="contour", colors=[(1, 2), (1, 2, 3)]), dict(style="contour", colors=[(1, 2, 256), (1, 2, 3)]), dict(style="contour", colors=3),
    ]
    for change in bad:
        a = {**dict(zoom_size=16, sheet_width=80), **ok, **change}
        with pytest.raises(ValueError):
            result_sheet(**a)
    with pytest.raises(NotImplementedError):                     # like the reference's draw_2d_heatmap
        result_sheet(**ok, zoom_size=16, sheet_width=80, colormap="hot")
    with pytest.raises(RuntimeError, match="cpu"):               # valid arguments, tensors on the host
        result_sheet(**ok, zoom_size=16, sheet_width=80)
    with pytest.raises(RuntimeError, match="cpu"):
        result_sheet(**ok, zoom_size=16, sheet_width=80, style="contour", thickness=[1], colors=[(255, 0, 0)])
    for masks in ([], [m] * 5, [m, m[:4]], m.float(), m.numpy(), [m[0]]):
        with pytest.raises(ValueError):
            sheet_occupancy(masks, 0, 16, 1)
    with pytest.raises(ValueError):
        sheet_occupancy(torch.ones((1, 1000, 1000), dtype=torch.uint8), 0, 300, 1)        # a zoomed extent of 0
    with pytest.raises(RuntimeError, match="cpu"):
        sheet_occupancy([m, m != 0], 0, 16, 1)


def test_inference_sheet_needs_the_original_grid_for_original():
    from dram_amd.inference import LobeInference
    with pytest.raises(ValueError, match="original"):
        LobeInference(None).sheet({"htp": torch.zeros(2, 2, 2), "mask": torch.zeros(2, 2, 2, dtype=torch.uint8)}, None, original=True)


def test_save_sheet_ppm_fallback(tmp_path, monkeypatch):
    from dram_amd import save_sheet
    g = np.random.default_rng(2)
    arr = g.integers(0, 256, size=(7, 11, 3)).astype(np.uint8)
    monkeypatch.setitem(sys.modules, "PIL", None)                # `from PIL import Image` now raises ImportError
    path = os.path.join(tmp_path, "sheet.ppm")
    assert save_sheet(torch.from_numpy(arr), path) == "ppm"
    raw = open(path, "rb").read()
    head = b"P6\n11 7\n255\n"
    assert raw[:len(head)] == head and raw[len(head):] == arr.tobytes()
    monkeypatch.undo()
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:                                        # with PIL: the format follows the extension, and reads back equal
        path = os.path.join(tmp_path, "sheet.png")
        assert save_sheet(arr, path) == "pil"
        assert np.array_equal(np.asarray(Image.open(path).convert("RGB")), arr)
    for bad in (arr[:, :, :2], arr.astype(np.float32), arr[0]):
        with pytest.raises(ValueError):
            save_sheet(bad, os.path.join(tmp_path, "bad.ppm"))
