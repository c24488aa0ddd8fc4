"""The named cases of the lesion texture tests, each at the smallest shape at which its failure can still show, and the
restatement's tables for each, computed once and shared between the tests.

A case is {scan int16, labels uint8 | int32, mask uint8, all [D,H,W], n, runs}; `runs` lists the settings (label kind, n, levels,
distance, masked) at which the case is run.  Which kernel a run takes is decided by dram_label_glcm_plan(label_kind, n, levels,
distance) alone (0: table in LDS, n * 13 * levels^2 <= 24576 words; 1: runs reduced within a wave), so a case reaches both plans
on one input by its n and its levels: labels above a run's n belong to nobody, and the expected table is the restatement's at
that n.

The kernel takes tiles of 16 x 64 voxels in (y, x) and marches along z in segments of at least 8 * distance planes (a volume of
D >= 16 * distance is split), one block for every two work items."""
import functools

import numpy as np

import texture_restatement as TR

LO, WIDTH = -1000, 75


def plan(label_kind, n, levels, distance=1):
    from dram_amd import _lib
    return _lib.lib.dram_label_glcm_plan(label_kind, n, levels, distance)


def _blocky(rng, shape, top, block, holes, dtype):
    """Labels 0..top in blocks of `block` voxels a side, a share `holes` of the voxels then re-drawn one by one."""
    coarse = rng.integers(0, top + 1, size=tuple(-(-s // block) for s in shape))
    lab = np.kron(coarse, np.ones((block,) * 3, dtype=np.int64))[:shape[0], :shape[1], :shape[2]]
    redraw = rng.random(shape) < holes
    lab[redraw] = rng.integers(0, top + 1, size=int(redraw.sum()))
    return lab.astype(dtype)


def _textured(rng, shape):
    """A scan with flat, noisy and striped parts and values on both sides of the window -1000 .. 200 HU."""
    z, y, x = np.meshgrid(*(np.arange(s) for s in shape), indexing="ij")
    scan = rng.integers(-1300, 500, size=shape)
    scan = np.where((z + y) % 5 < 2, -700 + 300 * ((x // 2) % 2), scan)             # stripes
    scan = np.where((x + y) % 7 == 0, -400, scan)                                   # flat
    return scan.astype(np.int16)


def _both_kinds(n_levels_distance_masked):
    return tuple((kind, *rest) for kind in (0, 1) for rest in n_levels_distance_masked)


@functools.lru_cache(maxsize=None)
def case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "odd":                                                    # no row a multiple of 16 bytes, no dimension of the tile; two z segments
        shape = (19, 21, 37)
        lab = _blocky(rng, shape, 4, 3, 0.1, np.int32)                    # n = 3: label 4 is n + 1
        lab[rng.random(shape) < 0.02] = -2
        lab[0, 0, :3] = (-(1 << 31), 1 << 30, 3)
        runs = tuple((1, n, levels, d, m) for n, levels in ((3, 2), (3, 16), (8, 16), (1, 32), (3, 32)) for d in (1, 2, 4) for m in (False, True))
    elif name == "odd_u8":
        shape = (19, 21, 37)
        lab = _blocky(rng, shape, 4, 3, 0.1, np.uint8)
        lab[0, 0, :2] = (255, 4)
        runs = tuple((0, n, levels, d, m) for n, levels in ((3, 2), (3, 16), (8, 16), (3, 32)) for d in (1, 2, 4) for m in (False, True))
    elif name == "tiles":                                                # 3 x 3 tiles, nine planes in one march
        shape = (9, 40, 150)
        lab = _blocky(rng, shape, 5, 4, 0.05, np.uint8)
        runs = _both_kinds(((5, 16, 1, False), (5, 16, 1, True), (8, 16, 1, False), (5, 32, 2, True)))
    elif name == "segments_d2":                                          # two z segments at distance 2, two tiles in x and in y
        shape = (37, 20, 70)
        lab = _blocky(rng, shape, 3, 5, 0.05, np.uint8)
        runs = _both_kinds(((3, 16, 2, False), (3, 32, 2, True)))
    elif name == "segments_d4":                                          # two z segments at distance 4: a halo wider than one
        shape = (70, 18, 20)
        lab = _blocky(rng, shape, 2, 6, 0.05, np.uint8)
        runs = _both_kinds(((2, 16, 4, False), (2, 32, 4, True), (8, 16, 4, True)))
    elif name == "full_box":                                             # one label up to every face; the last x tile is two voxels wide
        shape = (5, 17, 66)
        lab = np.ones(shape, np.uint8)
        runs = _both_kinds(((1, 16, 1, False), (1, 16, 2, False), (1, 16, 4, False), (8, 16, 1, False), (8, 16, 4, False)))
    elif name == "checkerboard":                                         # face-diagonal neighbours carry the same label, axis neighbours do not
        shape = (10, 20, 70)
        z, y, x = np.meshgrid(*(np.arange(s) for s in shape), indexing="ij")
        lab = (1 + (z + y + x) % 2).astype(np.uint8)
        runs = _both_kinds(((2, 16, 1, False), (2, 16, 2, False), (2, 32, 1, True)))
    else:
        raise KeyError(name)
    scan = _textured(rng, shape)
    mask = (rng.random(shape) < 0.8).astype(np.uint8)
    for a in (scan, lab, mask):
        a.setflags(write=False)
    return {"scan": scan, "labels": lab, "mask": mask, "runs": runs}


def names():
    return ["odd", "odd_u8", "tiles", "segments_d2", "segments_d4", "full_box", "checkerboard"]


@functools.lru_cache(maxsize=None)
def expected(name, n, levels, distance, masked):
    c = case(name)
    t = TR.glcm(c["scan"], c["labels"], n, c["mask"] if masked else None, levels, LO, WIDTH, distance)
    t.setflags(write=False)
    return t


def as_kind(labels, kind):
    return np.ascontiguousarray(labels, dtype=np.uint8 if kind == 0 else np.int32)


def box_pairs(shape, distance):
    """Per direction the ordered pairs (p, p + distance * offset) inside a box."""
    return [int(np.prod([max(0, s - distance * abs(o)) for s, o in zip(shape, off)])) for off in TR.OFFSETS]
