"""The named masks of the connected-component tests, each at the smallest shape at which its failure can still show, and the
restatement's labelling of each, computed once per (case, connectivity) and shared between the CPU and GPU tests."""
import functools

import numpy as np

import components_restatement as CR


def _mask(shape, points=()):
    m = np.zeros(shape, dtype=np.uint8)
    for p in points:
        m[p] = 1
    return m


def _row_with_runs():
    m = np.zeros((1, 1, 300), dtype=np.uint8)
    for a, b in ((0, 1), (3, 70), (71, 72), (128, 193), (255, 257), (299, 300)):     # runs across the 64- and 256-voxel seams
        m[0, 0, a:b] = 1
    return m


def _serpentine():
    """One path through every other row of (1,33,33), joined at alternating ends: one component whose chain of parents is
    hundreds of voxels long (a propagation with a fixed number of sweeps does not reach the end)."""
    m = np.zeros((1, 33, 33), dtype=np.uint8)
    m[0, 0::2, :] = 1
    for k, y in enumerate(range(1, 33, 2)):
        m[0, y, 32 if k % 2 == 0 else 0] = 1
    return m


def _comb(mirrored=False):
    """Teeth along x (every other row of every other slice) joined only by the plane x = 129: the unions that make it one
    component come last in raster order and cross every tile seam.  Mirrored: joined at x = 0."""
    m = np.zeros((4, 40, 130), dtype=np.uint8)
    m[0::2, 0::2, :] = 1
    m[:, :, 129] = 1
    return np.ascontiguousarray(m[:, :, ::-1]) if mirrored else m


def _checkerboard():
    z, y, x = np.meshgrid(np.arange(16), np.arange(16), np.arange(40), indexing="ij")
    return ((x + y + z) % 2).astype(np.uint8)


def _random(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


CASES = {
    "one_set": lambda: np.ones((1, 1, 1), dtype=np.uint8),
    "one_unset": lambda: np.zeros((1, 1, 1), dtype=np.uint8),
    "empty": lambda: np.zeros((4, 5, 6), dtype=np.uint8),
    "full": lambda: np.ones((2, 2, 2), dtype=np.uint8),
    "row_runs": _row_with_runs,
    # the voxel at x = W - 1 must not see x = 0 of the next row, nor the last row of a slice the first row of the next one
    # (in row_wrap (0,1,0) and (1,0,0) share an edge, so it is four components at connectivity 1 only; row_wrap_apart moves the
    # row pair one row down in a (2,4,5) volume, where no two of the four voxels touch at any connectivity)
    "row_wrap": lambda: _mask((2, 3, 5), [(0, 0, 4), (0, 1, 0), (0, 2, 4), (1, 0, 0)]),
    "row_wrap_apart": lambda: _mask((2, 4, 5), [(0, 1, 4), (0, 2, 0), (0, 3, 4), (1, 0, 0)]),
    "touch_face": lambda: _mask((2, 2, 2), [(0, 0, 0), (0, 0, 1)]),
    "touch_edge": lambda: _mask((2, 2, 2), [(0, 0, 0), (0, 1, 1)]),
    "touch_corner": lambda: _mask((2, 2, 2), [(0, 0, 0), (1, 1, 1)]),
    "serpentine": _serpentine,
    "comb": _comb,
    "comb_mirrored": lambda: _comb(True),
    "checkerboard": _checkerboard,
}
RANDOM_SHAPES = [(7, 9, 11), (16, 16, 16), (5, 6, 70), (3, 130, 5)]
for _si, _shape in enumerate(RANDOM_SHAPES):
    for _di, _density in enumerate((0.2, 0.35, 0.5)):
        CASES["random_%dx%dx%d_%02d" % (*_shape, int(_density * 100))] = functools.partial(_random, _shape, _density, 100 + 10 * _si + _di)

# component counts that are known without running anything: {case: {connectivity: n}}
KNOWN_COUNTS = {
    "one_set": {1: 1, 2: 1, 3: 1}, "one_unset": {1: 0, 2: 0, 3: 0}, "empty": {1: 0, 2: 0, 3: 0}, "full": {1: 1, 2: 1, 3: 1},
    "row_runs": {1: 6, 2: 6, 3: 6},
    "row_wrap": {1: 4, 2: 3, 3: 3}, "row_wrap_apart": {1: 4, 2: 4, 3: 4},
    "touch_face": {1: 1, 2: 1, 3: 1}, "touch_edge": {1: 2, 2: 1, 3: 1}, "touch_corner": {1: 2, 2: 2, 3: 1},
    "serpentine": {1: 1, 2: 1, 3: 1},
    "comb": {1: 1, 2: 1, 3: 1}, "comb_mirrored": {1: 1, 2: 1, 3: 1},
    "checkerboard": {1: 5120, 2: 1, 3: 1},
}
STATS_CASES = [name for name in CASES if name.startswith(("random", "comb"))]
CONNECTIVITIES = (1, 2, 3)


@functools.lru_cache(maxsize=None)
def mask_of(name):
    m = CASES[name]()
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def expected(name, connectivity):
    """(labels, n) of the restatement; read-only, computed once."""
    labels, n = CR.label(mask_of(name), connectivity)
    labels.setflags(write=False)
    return labels, n


def other_mask(name):
    """A second mask of the case's shape for the `hits` column."""
    m = mask_of(name)
    return (np.random.default_rng(len(name) + m.size).random(m.shape) < 0.4).astype(np.uint8)
