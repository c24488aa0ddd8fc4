"""The named cases of the lesion distribution tests, each at the smallest shape at which its failure can still show, and the
restatement's tables for each, computed once and shared between the CPU and GPU tests.

A case is {depth float32 [D,H,W], labels uint8 | int32, n, mask uint8 | None, bins_per_mm, nbins (0: no histogram), zones
(nz, ny, nx) | None, box 6 ints | None, offsets}: offsets = the elements by which depth, labels and mask are moved off a
16-byte boundary on the device.  The depth map of a structural case is surface_restatement.edt_passes of a sparse random
feature mask under an anisotropic spacing (zeros on the features, irrational distances elsewhere); the depth-value cases set
the values they are about by hand.

Which kernel a case takes is decided by dram_label_depth_plan(label_kind, n, nbins, nzones) alone (0: table in LDS, 1: runs
reduced within a wave), so a structural case is run once with its own small n (regime 0) and once as `<name>/wave` with n raised
to the first n that the LDS regime does not take at 4096 bins and the case's zones (labels above the case's own stay empty).
The boundaries are found by asking the library, never copied."""
import functools

import numpy as np

import distribution_restatement as XR
import surface_restatement as SR

SPACING = (2.5, 0.7, 0.8)
BPMS = (1, 2, 4, 8, 16)

# The launch walks 16 voxels per thread and aims at four laps: a block of 256 threads covers 4096 voxels per lap, one of 1024
# threads (tables above 16 KiB) 16384.  31 x 102 x 62 = 196,044 voxels = 12,252 groups of 16 + 12 voxels are 12 blocks x 4 laps
# at 256 threads and 3 blocks x 4 laps at 1024 threads (the last lap partial in both); the 12 odd voxels go element by element,
# and a row of 62 voxels never starts a group where the one before did.  Off the 16-byte alignment every voxel goes element by
# element: 192 blocks of 256 threads x 4 laps.
MULTI_LAP_SHAPE = (31, 102, 62)


def plan(label_kind, n, nbins, nzones):
    from dram_amd import _lib
    return _lib.lib.dram_label_depth_plan(label_kind, n, nbins, nzones)


@functools.lru_cache(maxsize=None)
def last_n_in_lds(label_kind, nbins, nzones):
    """The largest n that regime 0 takes at these settings (plan is monotone in n); None if n = 1 is past it."""
    top = 255 if label_kind == 0 else 1 << 20
    if plan(label_kind, 1, nbins, nzones) != 0:
        return None
    lo, hi = 1, top + 1                                   # plan(lo) == 0; hi is past the regime or past the range
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if plan(label_kind, mid, nbins, nzones) == 0 else (lo, mid)
    return lo


def nzones_of(c):
    return 0 if c["zones"] is None else c["zones"][0] * c["zones"][1] * c["zones"][2]


def kind_of(c):
    return 0 if c["labels"].dtype == np.uint8 else 1


@functools.lru_cache(maxsize=None)
def _edt(shape, seed):
    f = (np.random.default_rng(seed).random(shape) < 0.03).astype(np.uint8)
    f.reshape(-1)[0] = 1                                   # never without a feature
    d = SR.edt_passes(f, SPACING)
    d.setflags(write=False)
    return d


def _runs(rng, shape, n, dtype, zero_share=0.3, lengths=(3, 90)):
    """Labels in runs along the flat index, as a label volume has them, 0 among them."""
    size = int(np.prod(shape))
    out = np.zeros(0, dtype=np.int64)
    while out.size < size:
        k = 0 if rng.random() < zero_share else int(rng.integers(1, n + 1))
        out = np.concatenate([out, np.full(int(rng.integers(*lengths)), k)])
    return out[:size].astype(dtype).reshape(shape)


def _case(depth, labels, n, mask=None, bins_per_mm=4, nbins=0, zones=None, box=None, offsets=(0, 0, 0)):
    depth = np.ascontiguousarray(depth, dtype=np.float32)
    labels = np.ascontiguousarray(labels).reshape(depth.shape)
    return {"depth": depth, "labels": labels, "n": int(n), "mask": None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8).reshape(depth.shape),
            "bins_per_mm": int(bins_per_mm), "nbins": int(nbins), "zones": zones, "box": box, "offsets": tuple(offsets)}


def _small(seed, shape, n, dtype, **kw):
    rng = np.random.default_rng(seed)
    return _case(_edt(shape, seed), rng.integers(0, n + 1, size=shape).astype(dtype), n, **kw)


def _row_runs(every_voxel):
    labels = np.zeros((1, 1, 300), dtype=np.int32)
    if every_voxel:                                        # no two neighbours alike: there are no runs at all
        labels[0, 0, :] = 1 + np.arange(300) % 6
    else:                                                  # runs across the 64- and 256-voxel seams, one label in two runs
        for k, (a, b) in enumerate(((0, 1), (3, 70), (71, 72), (128, 193), (255, 257), (299, 300), (200, 230))):
            labels[0, 0, a:b] = min(k + 1, 6)
    return _case(_edt((1, 1, 300), 21), labels, 6, nbins=64, zones=(1, 1, 5))


def _skipped():
    c = _small(5, (3, 5, 7), 4, np.int32, nbins=128, zones=(2, 2, 2))
    c["labels"][0, 0, :6] = (-3, 0, 5, 2 ** 31 - 1, -2 ** 31, 4)        # below, zero and above the range: skipped
    return c


def _masked(value):
    c = _small(9, (4, 6, 10), 3, np.uint8, nbins=40, bins_per_mm=2, zones=(2, 1, 3))
    c["mask"] = (np.random.default_rng(10).random((4, 6, 10)) < 0.5).astype(np.uint8) * np.uint8(value)
    return c


def _offset(offsets, dtype):
    c = _small(13, (2, 9, 31), 5, dtype, nbins=4096, bins_per_mm=16, zones=(2, 3, 4), box=(0, 2, 1, 8, 3, 29), offsets=offsets)   # 558 voxels
    c["mask"] = (np.random.default_rng(14).random((2, 9, 31)) < 0.7).astype(np.uint8)
    return c


def _multi_lap(dtype, n, nbins, with_mask, seed, **kw):
    rng = np.random.default_rng(seed)
    labels = _runs(rng, MULTI_LAP_SHAPE, n, dtype, lengths=(5, 400))
    mask = (rng.random(MULTI_LAP_SHAPE) < 0.6).astype(np.uint8) * np.uint8(200) if with_mask else None
    return _case(_edt(MULTI_LAP_SHAPE, 30), labels, n, mask, nbins=nbins, **kw)


def _values(bins_per_mm, nbins=64):
    """Exactly k / bins_per_mm and the float just below it; nbins / bins_per_mm and just below; +inf, NaN, -1, -0.0; a value above
    the qsum clamp; equal minima on two voxels."""
    one = np.float32(1.0)
    edges = np.array([k / bins_per_mm for k in (0, 1, 2, 3, 7, nbins - 1, nbins)], dtype=np.float32)
    below = np.nextafter(edges[1:], np.float32(0.0))
    special = np.array([np.inf, np.nan, -1.0, -0.0, 3.0e6, 2097152.0, np.nextafter(np.float32(2097152.0), one * 0), 0.3, 0.3, 0.7],
                       dtype=np.float32)
    d = np.concatenate([edges, below, special])
    labels = np.ones(d.size, dtype=np.uint8)
    labels[-3:] = 2                                        # label 2: equal minima 0.3, 0.3
    labels[edges.size + below.size:edges.size + below.size + 4] = 3       # label 3: +inf, NaN, -1.0, -0.0
    return _case(d.reshape(1, 1, -1), labels, 4, bins_per_mm=bins_per_mm, nbins=nbins)


def _zones(zones, box, shape=(5, 7, 9), seed=50):
    return _small(seed, shape, 3, np.uint8, zones=zones, box=box)


def _wave_extremes():
    """The two extremes of the keyed wave reduction in one block: int32 labels, n = 64 and 4096 bins (past the LDS regime as it
    stands), 2 x 1024 + 5 voxels.  The 64 lanes of the first wave each hold another label for their 16 voxels (64 rounds, each a
    group of one lane), those of the second all hold label 7 (one round, the full butterfly), and the last 5 voxels go element
    by element."""
    labels = np.concatenate([1 + np.arange(1024) // 16, np.full(1024, 7), [3, 0, 64, 3, 1]]).astype(np.int32)
    return _case(_edt((1, 1, labels.size), 61), labels, 64, nbins=4096, zones=(1, 1, 5))


# regime 1 by their own n and bins
WAVE_ONLY = {"wave_64_groups_and_one": _wave_extremes}


def _seam(label_kind, n, nbins, zones, seed, size):
    """Every label 1..n occurs where n allows it, the last one for certain."""
    rng = np.random.default_rng(seed)
    shape = (1, 3, size // 3)
    labels = _runs(rng, shape, n, np.uint8 if label_kind == 0 else np.int32, lengths=(1, 9))
    labels.reshape(-1)[-3:] = n
    labels.reshape(-1)[:2] = 1
    return _case(_edt((1, 3, 200), 40)[:, :, np.arange(size // 3) % 200], labels, n, nbins=nbins, zones=zones)


BASE = {
    "one_voxel": lambda: _case(np.full((1, 1, 1), 1.25), np.array([[[1]]], dtype=np.uint8), 1, nbins=1024),
    "one_voxel_unlabelled": lambda: _case(np.full((1, 1, 1), 1.25), np.array([[[0]]], dtype=np.int32), 2, zones=(2, 1, 1)),
    "absent_label": lambda: _case(_edt((1, 4, 10), 1), np.repeat(np.array([1, 3, 0, 3], dtype=np.uint8), 10), 3, nbins=16, zones=(1, 2, 2)),
    "n1_u8": lambda: _small(2, (3, 4, 5), 1, np.uint8),
    "n255_u8": lambda: _small(3, (5, 20, 33), 255, np.uint8, zones=(2, 2, 2)),
    "skipped_i32": _skipped,
    "row_runs": lambda: _row_runs(False),
    "row_no_runs": lambda: _row_runs(True),
    "odd_size_105": lambda: _small(4, (3, 5, 7), 5, np.uint8, nbins=4096, bins_per_mm=16, zones=(3, 2, 2), box=(1, 2, 1, 4, 2, 6)),
    "odd_size_105_i32": lambda: _small(4, (3, 5, 7), 5, np.int32),
    "offset_all": lambda: _offset((1, 1, 1), np.uint8),
    "offset_depth": lambda: _offset((1, 0, 0), np.int32),
    "offset_labels": lambda: _offset((0, 1, 0), np.int32),
    "offset_mask": lambda: _offset((0, 0, 1), np.uint8),
    "mask_absent": lambda: {**_masked(1), "mask": None},
    "mask_200": lambda: _masked(200),
    **{f"values_bpm{b}": functools.partial(_values, b) for b in BPMS},
    "values_one_bin": lambda: _values(4, 1),
    "values_4096_bins": lambda: _values(8, 4096),
    "values_no_hist": lambda: _values(4, 0),
    "zones_box_inside": lambda: _zones((3, 2, 2), (1, 4, 2, 6, 1, 7)),           # smaller than the volume on both sides of every axis
    "zones_box_one_voxel": lambda: _zones((2, 2, 2), (2, 3, 3, 4, 4, 5)),
    "zones_more_than_voxels": lambda: _zones((8, 5, 7), (1, 4, 2, 5, 3, 7)),      # 8 zones over 3 voxels: empty zones
    "zones_not_divisible": lambda: _zones((3, 3, 4), (0, 5, 0, 7, 0, 9)),
    "zones_8x8x1": lambda: _zones((8, 8, 1), (0, 9, 1, 20, 0, 11), shape=(9, 21, 11), seed=51),
    "zones_no_box": lambda: _zones((2, 3, 2), None),
    "zones_one_with_box": lambda: _zones((1, 1, 1), (1, 4, 2, 6, 1, 7)),
    "zones_box_past_the_volume": lambda: _zones((4, 4, 4), (-3, 9, -2, 11, 2, 40)),
    "multi_lap_u8": lambda: _multi_lap(np.uint8, 5, 0, False, 31),
    "multi_lap_u8_hist": lambda: _multi_lap(np.uint8, 5, 4096, True, 32, bins_per_mm=16, zones=(3, 2, 1), box=(2, 29, 5, 95, 0, 62)),
    "multi_lap_i32": lambda: _multi_lap(np.int32, 40, 512, True, 33, zones=(2, 2, 2)),
    "multi_lap_offset": lambda: {**_multi_lap(np.uint8, 5, 64, True, 34, zones=(3, 2, 1)), "offsets": (1, 1, 1)},
}

# the same data with n past the LDS regime at 4096 bins
WAVE_OF = ("one_voxel", "absent_label", "skipped_i32", "row_runs", "row_no_runs", "odd_size_105", "offset_all", "offset_labels",
           "mask_200", "values_bpm4", "values_4096_bins", "zones_box_inside", "zones_more_than_voxels", "zones_8x8x1",
           "multi_lap_u8_hist", "multi_lap_i32", "multi_lap_offset")


def _wave(name):
    c = dict(BASE[name]())
    c["nbins"] = 4096
    c["n"] = max(c["n"], last_n_in_lds(kind_of(c), 4096, nzones_of(c)) + 1)
    return c


def _seam_cases():
    """For each setting the largest n that the LDS regime takes and the first one past it."""
    out = {}
    for tag, kind, nbins, zones in (("i32_nohist", 1, 0, None), ("i32_nohist_zones", 1, 0, (3, 2, 1)), ("i32_4096", 1, 4096, None),
                                    ("u8_4096_zones", 0, 4096, (3, 2, 1))):
        n0 = last_n_in_lds(kind, nbins, 0 if zones is None else zones[0] * zones[1] * zones[2])
        size = 3 * n0 if nbins == 0 else 6000
        out[f"seam_{tag}_last"] = functools.partial(_seam, kind, n0, nbins, zones, 41, size)
        out[f"seam_{tag}_past"] = functools.partial(_seam, kind, n0 + 1, nbins, zones, 42, size)
    return out


SEAM_REGIMES = {f"seam_{tag}_{end}": r for tag in ("i32_nohist", "i32_nohist_zones", "i32_4096", "u8_4096_zones")
                for end, r in (("last", 0), ("past", 1))}
NAMES_WITHOUT_LIBRARY = tuple(BASE)


@functools.lru_cache(maxsize=None)
def names():
    return tuple(BASE) + tuple(k + "/wave" for k in WAVE_OF) + tuple(WAVE_ONLY) + tuple(SEAM_REGIMES)


@functools.lru_cache(maxsize=None)
def case(name):
    if name.endswith("/wave"):
        c = _wave(name[:-5])
    elif name in WAVE_ONLY:
        c = WAVE_ONLY[name]()
    else:
        c = BASE[name]() if name in BASE else _seam_cases()[name]()
    for key in ("depth", "labels", "mask"):
        if c[key] is not None:
            c[key].setflags(write=False)
    return c


def regime(name):
    c = case(name)
    return plan(kind_of(c), c["n"], c["nbins"], nzones_of(c))


@functools.lru_cache(maxsize=None)
def expected(name):
    """The restatement's tables; read-only, computed once."""
    c = case(name)
    t = XR.tables(c["depth"], c["labels"], c["n"], c["mask"], c["bins_per_mm"], c["nbins"], c["zones"], c["box"])
    for a in t.values():
        if a is not None:
            a.setflags(write=False)
    return t
