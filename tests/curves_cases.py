"""The named cases of the heat-map curve tests, each at the smallest shape at which its failure can still show, and the
restatement's tables for each, computed once and shared between the CPU and GPU tests.

A case is {score float32, ref uint8, region uint8 | None, nregions, gate uint8 | None, nbins, conf bool, offsets}: offsets = the
elements by which score, ref, region and gate are moved off a 16-byte boundary on the device.

Which path a case takes is decided by dram_score_hist_plan(nregions, nbins, conf) alone (0: the table in LDS, 1: updates to global
memory).  The launch walks 16 voxels per thread with 16-byte loads and aims at four laps: a block of 256 threads (tables up to
16 KiB, and path 1) covers 4096 voxels per lap, one of 1024 threads (larger tables in LDS) 16384.  Off the 16-byte alignment, and
for the last nvox % 16 voxels, every voxel goes element by element, one voxel per lane."""
import functools

import numpy as np

import curves_restatement as CR

SMALL = dict(nregions=1, nbins=256)          # 6 KiB with conf: 256 threads
BIG = dict(nregions=5, nbins=1024)           # 120 KiB with conf: 1024 threads
MULTI_LAP_VOXELS = 16 * 12289 + 5            # 13 blocks x 4 laps at 256 threads, 4 blocks x 4 laps at 1024 (last lap partial) + 5


def plan(nregions, nbins, conf):
    from dram_amd import _lib
    return _lib.lib.dram_score_hist_plan(nregions, nbins, int(bool(conf)))


def special_scores(nbins):
    """Bin edges j / nbins and their fp32 neighbours, the ends of the range and everything outside it."""
    f = np.float32
    edges = np.array([j / nbins for j in sorted({0, 1, 2, nbins // 2, nbins - 1})], dtype=np.float32)
    below, above = np.nextafter(edges, f(-1)), np.nextafter(edges, f(2))
    rest = np.array([0.0, -0.0, np.float32(1e-45), 1.0, np.nextafter(f(1), f(0)), 1.5, np.inf, -1e-30, -np.inf, np.nan, 0.5, 0.999],
                    dtype=np.float32)
    return np.concatenate([edges, below, above, rest])


def _skewed(rng, n):
    """A heat map as a sigmoid head gives it inside the lungs: nearly everything within a few low bins, a thin tail up to 1."""
    s = rng.normal(0.02, 0.002, size=n)
    tail = rng.random(n) < 0.03
    s[tail] = rng.random(int(tail.sum()))
    return s.astype(np.float32)


def _case(score, ref, region=None, nregions=1, gate=None, nbins=256, conf=True, offsets=(0, 0, 0, 0)):
    u8 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.uint8)
    return {"score": np.ascontiguousarray(score, dtype=np.float32), "ref": u8(ref), "region": u8(region), "nregions": int(nregions),
            "gate": u8(gate), "nbins": int(nbins), "conf": bool(conf), "offsets": tuple(offsets)}


def _random(seed, n, nregions=1, nbins=256, conf=True, region="labels", gate="random", offsets=(0, 0, 0, 0), skew=True, specials=True):
    """n voxels: a skewed or uniform map with the special scores sprinkled in, a reference that follows the score loosely, region
    labels in runs (0 and labels above nregions among them), a gate."""
    rng = np.random.default_rng(seed)
    score = _skewed(rng, n) if skew else rng.random(n).astype(np.float32)
    if specials:
        sp = special_scores(nbins)
        where = rng.choice(n, size=min(n, sp.size), replace=False)
        score[where] = sp[:where.size]
    with np.errstate(invalid="ignore"):
        ref = ((rng.random(n) < np.clip(np.nan_to_num(score), 0.05, 0.9)) * rng.integers(1, 256, size=n)).astype(np.uint8)
    reg = None
    if region == "labels":
        top = min(nregions + 2, 255)                       # labels above nregions are skipped
        reg = np.zeros(0, dtype=np.int64)
        while reg.size < n:
            k = 0 if rng.random() < 0.3 else int(rng.integers(1, top + 1))
            reg = np.concatenate([reg, np.full(int(rng.integers(1, 70)), k)])
        reg = reg[:n]
    elif region == "every":                                # every voxel its own label: no runs
        reg = rng.integers(0, min(nregions + 2, 256), size=n)
    g = {None: None, "on": np.full(n, 7), "off": np.zeros(n), "random": (rng.random(n) < 0.8) * rng.integers(1, 256, size=n)}[gate]
    return _case(score, ref, reg, nregions, g, nbins, conf, offsets)


def _one_voxel(score, ref, region, gate):
    return _case(np.array([score]), np.array([ref]), None if region is None else np.array([region]), 1,
                 None if gate is None else np.array([gate]), 256)


def _specials(nbins, conf=True):
    sp = special_scores(nbins)
    score = np.concatenate([sp, sp, sp])                   # both classes gate on, and once gate off
    ref = np.concatenate([np.zeros(sp.size), np.ones(sp.size), np.ones(sp.size)])
    gate = np.concatenate([np.ones(2 * sp.size), np.zeros(sp.size)])
    return _case(score, ref, None, 1, gate, nbins, conf)


def _one_bin():
    n = 65536
    return _case(np.full(n, 0.0201, dtype=np.float32), np.ones(n), np.full(n, 2), 3, None, 1024)


def _two_bins(offset):
    """Voxel by voxel two bins in turn.  Aligned, all lanes of a wave send the same key at each of a thread's 16 positions; moved off
    the alignment the voxels go one per lane, so neighbouring lanes alternate."""
    n = 65536
    score = np.where(np.arange(n) % 2 == 0, np.float32(0.0201), np.float32(0.73)).astype(np.float32)
    return _case(score, np.zeros(n), None, 1, None, 1024, True, (offset,) * 4)


def _empty_class(positive):
    c = _random(61, 3000, 5, 256)
    c["ref"] = np.full(3000, 1 if positive else 0, dtype=np.uint8)
    return c


def _empty_region():
    c = _random(62, 3000, 5, 256)
    c["region"] = np.where(c["region"] == 3, 0, c["region"]).astype(np.uint8)
    return c


def _sized(n, table):
    return lambda: _random(100 + n, n, **table)


BASE = {
    "one_voxel": lambda: _one_voxel(0.5, 1, None, None),
    "one_voxel_skipped": lambda: _one_voxel(0.5, 1, 0, 1),
    "one_voxel_gate_off": lambda: _one_voxel(0.5, 0, 1, 0),
    **{f"size_{n}": _sized(n, SMALL) for n in (15, 16, 17, 63, 64, 65, 4095, 4096, 4097)},
    **{f"size_big_{n}": _sized(n, BIG) for n in (16383, 16384, 16385)},
    "multi_lap_small": lambda: _random(31, MULTI_LAP_VOXELS, **SMALL),
    "multi_lap_big": lambda: _random(32, MULTI_LAP_VOXELS, **BIG),
    "multi_lap_big_uniform": lambda: _random(33, MULTI_LAP_VOXELS, skew=False, region="every", **BIG),
    "multi_lap_global": lambda: _random(34, MULTI_LAP_VOXELS, 5, 4096),
    "multi_lap_global_noconf": lambda: _random(35, MULTI_LAP_VOXELS, 5, 4096, conf=False, skew=False),
    "multi_lap_offset": lambda: _random(36, MULTI_LAP_VOXELS, offsets=(1, 1, 1, 1), **BIG),
    "offset_none": lambda: _random(40, 5003, 5, 256, offsets=(0, 0, 0, 0)),
    "offset_score_1": lambda: _random(41, 5003, 5, 256, offsets=(1, 0, 0, 0)),
    "offset_score_3": lambda: _random(42, 5003, 5, 256, offsets=(3, 0, 0, 0)),
    "offset_ref_1": lambda: _random(43, 5003, 5, 256, offsets=(0, 1, 0, 0)),
    "offset_ref_3": lambda: _random(44, 5003, 5, 256, offsets=(0, 3, 0, 0)),
    "offset_region_1": lambda: _random(45, 5003, 5, 256, offsets=(0, 0, 1, 0)),
    "offset_region_3": lambda: _random(46, 5003, 5, 256, offsets=(0, 0, 3, 0)),
    "offset_gate_1": lambda: _random(47, 5003, 5, 256, offsets=(0, 0, 0, 1)),
    "offset_gate_3": lambda: _random(48, 5003, 5, 256, offsets=(0, 0, 0, 3)),
    "offset_all_3_global": lambda: _random(49, 5003, 5, 4096, offsets=(3, 3, 3, 3)),
    "specials_2": lambda: _specials(2),
    "specials_256": lambda: _specials(256),
    "specials_1024": lambda: _specials(1024, conf=False),
    "specials_4096": lambda: _specials(4096),
    "region_null": lambda: _random(50, 3000, 1, 256, region=None),
    "region_null_4096_noconf": lambda: _random(51, 3000, 1, 4096, region=None, conf=False),
    "regions_1": lambda: _random(52, 3000, 1, 256),
    "regions_5": lambda: _random(53, 3000, 5, 1024),
    "regions_255_lds": lambda: _random(54, 6000, 255, 2, region="every"),
    "regions_255_global": lambda: _random(55, 6000, 255, 256, region="every"),
    "regions_255_global_noconf": lambda: _random(56, 6000, 255, 256, conf=False),
    "no_positive": lambda: _empty_class(False),
    "no_negative": lambda: _empty_class(True),
    "empty_region": _empty_region,
    "one_bin_64k": _one_bin,
    "two_bins_per_voxel": lambda: _two_bins(0),
    "two_bins_per_lane": lambda: _two_bins(1),
    "gate_null": lambda: _random(70, 3000, 5, 256, gate=None),
    "gate_on": lambda: _random(71, 3000, 5, 256, gate="on"),
    "gate_off": lambda: _random(72, 3000, 5, 256, gate="off"),
    "gate_random_noconf": lambda: _random(73, 3000, 5, 256, conf=False),
    "gate_null_noconf_global": lambda: _random(74, 3000, 5, 4096, gate=None, conf=False),
}

# what the structural cases must report as their path
REGIMES = {"multi_lap_small": 0, "multi_lap_big": 0, "multi_lap_global": 1, "multi_lap_global_noconf": 1, "regions_255_lds": 0,
           "regions_255_global": 1, "regions_255_global_noconf": 1, "specials_4096": 0, "offset_all_3_global": 1}


def names():
    return tuple(BASE)


@functools.lru_cache(maxsize=None)
def case(name):
    c = dict(BASE[name]())
    for key in ("score", "ref", "region", "gate"):
        if c[key] is not None:
            c[key].setflags(write=False)
    return c


def regime(name):
    c = case(name)
    return plan(c["nregions"], c["nbins"], c["conf"])


@functools.lru_cache(maxsize=None)
def expected(name):
    """(hist, conf | None) of the restatement; read-only, computed once."""
    c = case(name)
    out = CR.tables(c["score"], c["ref"], c["region"], c["nregions"], c["gate"], c["nbins"], c["conf"])
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


INT_KEYS = ("tp", "fp", "fn", "tn", "cal_count", "cal_positive")
FP_KEYS = ("thresholds", "tpr", "fpr", "precision", "dice", "iou", "best_dice", "best_dice_threshold", "auc_roc", "average_precision",
           "cal_confidence", "cal_frequency", "ece")


def n_cal(c):
    return min(16, c["nbins"]) if c["conf"] else None


def assert_curves_equal(got, ref):
    """Integers exactly; fp64 to 1e-12 relative: the same operations up to the order of sums of at most 4097 terms."""
    assert sorted(got) == sorted(ref)
    for key in ref:
        g, r = np.asarray(got[key]), np.asarray(ref[key])
        assert g.shape == r.shape and g.dtype == r.dtype, key
        if key in INT_KEYS:
            assert np.array_equal(g, r), key
        else:
            assert key in FP_KEYS
            assert np.array_equal(np.isnan(g), np.isnan(r)), key
            ok = ~np.isnan(r)
            assert np.all(np.abs(g[ok] - r[ok]) <= 1e-12 * np.abs(r[ok])), key
