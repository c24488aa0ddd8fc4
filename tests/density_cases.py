"""The named cases of the lesion density tests, each at the smallest shape at which its failure can still show, and the
restatement's result for each, computed once and shared between the CPU and GPU tests.

A case is {scan int16, labels uint8 | int32, n, mask uint8 | None, bins (lo, width, nbins) | None, offsets}: offsets = the
elements by which scan, labels and mask are moved off a 16-byte boundary on the device.

Which kernel a case takes is decided by dram_label_density_plan(label_kind, n, nbins) alone (0: table in LDS, 1: runs reduced
within a wave), so a structural case is run once with its own small n (regime 0) and once as `<name>/wave` with n raised to the
first n that the LDS regime does not take at 4096 bins (labels above the case's own stay empty).  The boundaries are found by
asking the library, never copied."""
import functools

import numpy as np

import density_restatement as DR

FULL_BINS = (-1024, 1, 4096)

# The launch walks 16 voxels per thread and aims at four laps: a block of 256 threads covers 4096 voxels per lap, one of 1024
# threads (tables above 16 KiB) 16384.  196,629 voxels = 12,289 groups of 16 + 5 voxels are 13 blocks x 4 laps at 256 threads
# and 4 blocks x 4 laps at 1024 threads (the last lap partial in both), and the 5 odd voxels go element by element.  Off the
# 16-byte alignment every voxel goes element by element: 769 blocks of 256 threads x 4 laps.
MULTI_LAP_VOXELS = 16 * 12289 + 5


def plan(label_kind, n, nbins):
    from dram_amd import _lib
    return _lib.lib.dram_label_density_plan(label_kind, n, nbins)


@functools.lru_cache(maxsize=None)
def last_n_in_lds(label_kind, nbins):
    """The largest n that regime 0 takes at this label kind and nbins (plan is monotone in n); None if n = 1 is past it."""
    top = 255 if label_kind == 0 else 1 << 20
    if plan(label_kind, 1, nbins) != 0:
        return None
    lo, hi = 1, top + 1                                   # plan(lo) == 0; hi is past the regime or past the range
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if plan(label_kind, mid, nbins) == 0 else (lo, mid)
    return lo


@functools.lru_cache(maxsize=None)
def last_nbins_in_lds(label_kind, n):
    """The largest nbins that regime 0 takes at this n (None if even nbins = 0 is past it)."""
    if plan(label_kind, n, 0) != 0:
        return None
    lo, hi = 0, 4097
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if plan(label_kind, n, mid) == 0 else (lo, mid)
    return lo


def _hu(rng, size):
    """Plausible Hounsfield units with a few values at and past the ends of the default range."""
    v = rng.integers(-1100, 400, size=size).astype(np.int16)
    flat = v.reshape(-1)
    flat[::53] = rng.choice(np.array([-32768, -1025, -1024, 3071, 3072, 32767], dtype=np.int16), size=flat[::53].size)
    return v


def _runs(rng, size, n, dtype, zero_share=0.3, lengths=(3, 90)):
    """Labels in runs, as a label volume has them, 0 among them."""
    out = np.zeros(0, dtype=np.int64)
    while out.size < size:
        k = 0 if rng.random() < zero_share else int(rng.integers(1, n + 1))
        out = np.concatenate([out, np.full(int(rng.integers(*lengths)), k)])
    return out[:size].astype(dtype)


def _case(scan, labels, n, mask=None, bins=None, offsets=(0, 0, 0)):
    return {"scan": np.ascontiguousarray(scan, dtype=np.int16), "labels": np.ascontiguousarray(labels), "n": int(n),
            "mask": None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8), "bins": bins, "offsets": tuple(offsets)}


def _row_runs(every_voxel):
    rng = np.random.default_rng(21)
    labels = np.zeros((1, 1, 300), dtype=np.int32)
    if every_voxel:                                        # no two neighbours alike: there are no runs at all
        labels[0, 0, :] = 1 + np.arange(300) % 6
    else:                                                  # runs across the 64- and 256-voxel seams, one label in two runs
        for k, (a, b) in enumerate(((0, 1), (3, 70), (71, 72), (128, 193), (255, 257), (299, 300), (200, 230))):
            labels[0, 0, a:b] = min(k + 1, 6)
    return _case(_hu(rng, (1, 1, 300)), labels, 6, bins=(-1024, 1, 64))


def _extremes():
    labels = np.repeat(np.array([1, 2, 0], dtype=np.uint8), (71680, 71680, 16))
    scan = np.repeat(np.array([32767, -32768, 5], dtype=np.int16), (71680, 71680, 16))
    return _case(scan, labels, 2, bins=(-1024, 7, 16))


def _hist_edges(lo, width, nbins, dtype=np.uint8):
    v = np.array([lo - 1, lo, lo + width - 1, lo + width, lo + nbins * width - 1, lo + nbins * width, lo, lo - 1], dtype=np.int64)
    labels = np.array([1, 1, 1, 1, 1, 1, 2, 2], dtype=dtype)
    return _case(v.astype(np.int16), labels, 3, bins=(lo, width, nbins))


def _multi_lap(dtype, n, bins, with_mask, seed):
    rng = np.random.default_rng(seed)
    labels = _runs(rng, MULTI_LAP_VOXELS, n, dtype, lengths=(5, 400))
    mask = (rng.random(MULTI_LAP_VOXELS) < 0.6).astype(np.uint8) * np.uint8(200) if with_mask else None
    return _case(_hu(rng, MULTI_LAP_VOXELS), labels, n, mask, bins)


def _seam(label_kind, n, nbins, seed, size=6000):
    """Every label 1..n occurs where n allows it, the last one for certain."""
    rng = np.random.default_rng(seed)
    dtype = np.uint8 if label_kind == 0 else np.int32
    labels = _runs(rng, size, n, dtype, lengths=(1, 9))
    labels[-3:] = n
    labels[:2] = 1
    return _case(_hu(rng, size), labels, n, bins=None if nbins == 0 else (-1024 + 5, 3, nbins))


def _small(seed, shape, n, dtype, **kw):
    rng = np.random.default_rng(seed)
    return _case(_hu(rng, shape), rng.integers(0, n + 1, size=shape).astype(dtype), n, **kw)


def _skipped():
    c = _small(5, (3, 5, 7), 4, np.int32, bins=(-1024, 16, 128))
    c["labels"][0, 0, :6] = (-3, 0, 5, 2 ** 31 - 1, -2 ** 31, 4)        # below, zero and above the range: skipped
    return c


def _masked(value):
    rng = np.random.default_rng(9)
    c = _small(9, (4, 6, 10), 3, np.uint8, bins=(-1000, 7, 40))
    c["mask"] = (rng.random((4, 6, 10)) < 0.5).astype(np.uint8) * np.uint8(value)
    return c


def _offset(offsets, dtype):
    c = _small(13, (2, 9, 31), 5, dtype, bins=(-1024, 1, 4096), offsets=offsets)   # 558 voxels: 34 groups of 16 + 14
    c["mask"] = (np.random.default_rng(14).random((2, 9, 31)) < 0.7).astype(np.uint8)
    return c


BASE = {
    "one_voxel": lambda: _case(np.array([[[-700]]]), np.array([[[1]]], dtype=np.uint8), 1, bins=(-1024, 1, 4096)),
    "one_voxel_unlabelled": lambda: _case(np.array([[[-700]]]), np.array([[[0]]], dtype=np.int32), 2),
    "absent_label": lambda: _case(_hu(np.random.default_rng(1), 40), np.repeat(np.array([1, 3, 0, 3], dtype=np.uint8), 10), 3,
                                  bins=(-1024, 1, 16)),
    "n1_u8": lambda: _small(2, (3, 4, 5), 1, np.uint8),
    "n255_u8": lambda: _small(3, (5, 20, 33), 255, np.uint8),
    "skipped_i32": _skipped,
    "row_runs": lambda: _row_runs(False),
    "row_no_runs": lambda: _row_runs(True),
    "odd_size_105": lambda: _small(4, (3, 5, 7), 5, np.uint8, bins=(-1024, 1, 4096)),
    "odd_size_105_i32": lambda: _small(4, (3, 5, 7), 5, np.int32),
    "offset_all": lambda: _offset((1, 1, 1), np.uint8),
    "offset_scan": lambda: _offset((1, 0, 0), np.int32),
    "offset_labels": lambda: _offset((0, 1, 0), np.int32),
    "offset_mask": lambda: _offset((0, 0, 1), np.uint8),
    "extremes": _extremes,
    "mask_absent": lambda: {**_masked(1), "mask": None},
    "mask_200": lambda: _masked(200),
    "hist_w1_negative_lo": lambda: _hist_edges(-50, 1, 10),
    "hist_w7_negative_lo": lambda: _hist_edges(-1000, 7, 100, np.int32),
    "hist_one_bin": lambda: _hist_edges(-5, 7, 1),
    "hist_4096_w1": lambda: _hist_edges(-1024, 1, 4096),
    "hist_4096_w7": lambda: _hist_edges(-1024, 7, 4096, np.int32),
    "hist_none": lambda: {**_hist_edges(-50, 1, 10), "bins": None},
    "multi_lap_u8": lambda: _multi_lap(np.uint8, 5, None, False, 31),
    "multi_lap_u8_hist": lambda: _multi_lap(np.uint8, 5, FULL_BINS, True, 32),
    "multi_lap_i32": lambda: _multi_lap(np.int32, 40, (-1024, 8, 512), True, 33),
    "multi_lap_offset": lambda: {**_multi_lap(np.uint8, 5, (-1024, 1, 64), True, 34), "offsets": (1, 1, 1)},
}

# the same data with n past the LDS regime at 4096 bins
WAVE_OF = ("one_voxel", "absent_label", "skipped_i32", "row_runs", "row_no_runs", "odd_size_105", "offset_all", "offset_labels",
           "extremes", "mask_200", "hist_4096_w7", "multi_lap_u8_hist", "multi_lap_i32", "multi_lap_offset")


def _wave(name):
    c = dict(BASE[name]())
    kind = 0 if c["labels"].dtype == np.uint8 else 1
    c["n"] = max(c["n"], last_n_in_lds(kind, FULL_BINS[2]) + 1)
    c["bins"] = FULL_BINS if c["bins"] is None or c["bins"][2] != 4096 else c["bins"]
    return c


def _wave_extremes():
    """The two extremes of the keyed wave reduction in one block: int32 labels, n = 64 and 4096 bins (n * (7 + 4098) words: past
    the LDS regime as it stands), 2 x 1024 + 5 voxels.  The 64 lanes of the first wave each hold another label for their 16
    voxels (64 rounds, each a group of one lane), those of the second all hold label 7 (one round, the full butterfly), and the
    last 5 voxels go element by element."""
    labels = np.concatenate([1 + np.arange(1024) // 16, np.full(1024, 7), [3, 0, 64, 3, 1]]).astype(np.int32)
    return _case(_hu(np.random.default_rng(61), labels.size), labels, 64, bins=FULL_BINS)


# regime 1 by their own n and bins
WAVE_ONLY = {"wave_64_groups_and_one": _wave_extremes}


def _seam_cases():
    """For each regime the largest n or nbins it takes and the first one past it."""
    out = {}
    n0 = last_n_in_lds(1, 0)                               # int32 labels without a histogram
    out["seam_i32_nohist_last"], out["seam_i32_nohist_past"] = (lambda: _seam(1, n0, 0, 41, 3 * n0)), (lambda: _seam(1, n0 + 1, 0, 42, 3 * n0))
    b0 = last_nbins_in_lds(0, 255)                         # uint8 labels, all 255 of them
    out["seam_u8_255_last"], out["seam_u8_255_past"] = (lambda: _seam(0, 255, b0, 43)), (lambda: _seam(0, 255, b0 + 1, 44))
    n4 = last_n_in_lds(1, 4096)                            # the full histogram
    out["seam_i32_4096_last"], out["seam_i32_4096_past"] = (lambda: _seam(1, n4, 4096, 45)), (lambda: _seam(1, n4 + 1, 4096, 46))
    return out


@functools.lru_cache(maxsize=None)
def names():
    return tuple(BASE) + tuple(k + "/wave" for k in WAVE_OF) + tuple(WAVE_ONLY) + tuple(_seam_cases())


# what each seam case must report as its regime
SEAM_REGIMES = {"seam_i32_nohist_last": 0, "seam_i32_nohist_past": 1, "seam_u8_255_last": 0, "seam_u8_255_past": 1,
                "seam_i32_4096_last": 0, "seam_i32_4096_past": 1}
NAMES_WITHOUT_LIBRARY = tuple(BASE)


@functools.lru_cache(maxsize=None)
def case(name):
    if name.endswith("/wave"):
        c = _wave(name[:-5])
    elif name in WAVE_ONLY:
        c = WAVE_ONLY[name]()
    else:
        c = BASE[name]() if name in BASE else _seam_cases()[name]()
    for key in ("scan", "labels", "mask"):
        if c[key] is not None:
            c[key].setflags(write=False)
    return c


def regime(name):
    c = case(name)
    return plan(0 if c["labels"].dtype == np.uint8 else 1, c["n"], 0 if c["bins"] is None else c["bins"][2])


@functools.lru_cache(maxsize=None)
def expected(name):
    """(count, sum, sumsq, min, max, hist | None) of the restatement; read-only, computed once."""
    c = case(name)
    out = DR.moments(c["scan"], c["labels"], c["n"], c["mask"])
    hist = None if c["bins"] is None else DR.histogram(c["scan"], c["labels"], c["n"], *c["bins"], c["mask"])
    for a in out + ((hist,) if hist is not None else ()):
        a.setflags(write=False)
    return out + (hist,)


# ---- histogram rows for dram_hist_summary: {hist [n, nbins + 2], lo, width, nbins, q, edges}
def _rows(*rows):
    return np.array(rows, dtype=np.int64)


def _random_rows(seed, n, nbins, empty_row=None):
    h = np.random.default_rng(seed).integers(0, 50, size=(n, nbins + 2)).astype(np.int64)
    h[:, ::3] = 0
    if empty_row is not None:
        h[empty_row] = 0
    return h


SUMMARY_CASES = {
    # ten values in four bins: q = 0 and a rank inside the first entry, the median of an even count, q = 1000
    "even_count_median": dict(hist=_rows([0, 1, 4, 0, 5, 0], [0, 5, 0, 0, 5, 0], [0, 2, 2, 2, 4, 0]), lo=-10, width=5, nbins=4,
                              q=(0, 500, 1000, 501, 1), edges=(-5, 5)),
    "rank_in_underflow": dict(hist=_rows([7, 1, 1, 1], [1, 0, 0, 9]), lo=-3, width=7, nbins=2, q=(0, 100, 500, 700, 1000), edges=(4,)),
    "rank_only_in_overflow": dict(hist=_rows([0, 1, 0, 9], [0, 0, 0, 4]), lo=-3, width=1, nbins=2, q=(0, 100, 101, 1000), edges=(-2,)),
    "empty_row": dict(hist=_rows([0, 0, 0, 0, 0], [1, 2, 3, 4, 5], [0, 0, 0, 0, 0]), lo=0, width=2, nbins=3, q=(0, 500, 1000), edges=(2, 4)),
    "edges_on_both_ends": dict(hist=_rows([3, 1, 2, 3, 4], [0, 0, 5, 0, 6]), lo=-6, width=3, nbins=3, q=(150, 850), edges=(-6, 0, 3)),
    "no_percentiles": dict(hist=_random_rows(3, 4, 12), lo=-100, width=10, nbins=12, q=(), edges=(-50, 0)),
    "no_edges": dict(hist=_random_rows(4, 4, 12), lo=-100, width=10, nbins=12, q=(0, 150, 500, 850, 1000), edges=()),
    "one_bin": dict(hist=_rows([2, 3, 4], [0, 3, 0]), lo=-5, width=7, nbins=1, q=(0, 300, 1000), edges=(-5, 2)),
    # rows longer than the block: 4098 entries in pieces of 17, the default report's settings; 16 percentiles and 15 edges
    "full_row": dict(hist=_random_rows(5, 6, 4096, empty_row=2), lo=-1024, width=1, nbins=4096,
                     q=tuple(range(0, 1001, 67))[:15] + (1000,), edges=tuple(range(-1024, 3073, 292))[:15]),
    "full_row_w7": dict(hist=_random_rows(6, 3, 4096), lo=-1024, width=7, nbins=4096, q=(150, 500, 850), edges=(-1024 + 7 * 4096,)),
}


@functools.lru_cache(maxsize=None)
def summary_expected(name):
    c = SUMMARY_CASES[name]
    return DR.summary(c["hist"], c["lo"], c["width"], c["nbins"], c["q"], c["edges"])
