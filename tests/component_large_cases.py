"""Masks for the connected-component kernels at the sizes only a whole scan reaches: more than 1024 tiles of 1024 voxels, so that
`cc_scan_kernel` walks several laps with its carry, and more than 16384 x 256 elements for the grid-strided `cc_relabel_kernel`.
Every expectation is known by construction (vectorised numpy; the flood fill of components_restatement.label only ever sees a
7 x 9 x 12 block), and every generator takes the shape, so that tests/test_components_cpu.py can hold the construction against
the flood fill at SMALL."""
import functools

import numpy as np

import components_restatement as CR

TILE = 1024                               # csrc/components.hip: CC_TILE, and the tiles per lap of cc_scan_kernel
LARGE = (33, 250, 260)                    # 2,145,000 voxels = 2095 tiles: laps of 1024, 1024 and 47 tiles; W is no multiple of 64
SMALL = (5, 20, 39)
GAP = (TILE * TILE, 2 * TILE * TILE)      # the voxels whose tile counts form the whole second lap of the scan
CONNECTIVITIES = (1, 2, 3)

RELABEL_CAP = 16384 * 256                 # elements of one lap of cc_relabel_kernel at its grid cap
RELABEL_NVOX = RELABEL_CAP + 300
RELABEL_N = 1000


def tiles_of(shape):
    return -(-int(np.prod(shape)) // TILE)


def tile_counts(first_voxels, shape):
    """Roots (first voxels of the components, as a boolean volume) per tile: what cc_flatten hands to cc_scan."""
    flat = np.zeros(tiles_of(shape) * TILE, dtype=np.int64)
    flat[:first_voxels.size] = first_voxels.ravel()
    return flat.reshape(-1, TILE).sum(axis=1)


def _isolated(mask):
    """No two set voxels touch: every set voxel is its own component, numbered in raster order."""
    labels = (np.cumsum(mask.ravel(), dtype=np.int64).reshape(mask.shape) * mask).astype(np.int32)
    return mask, labels, int(mask.sum())


def lattice_thinned(shape, connectivity=1, seed=21):
    """Voxels with z, y, x all even, each set with probability 0.5: no two are 26-adjacent, so the labelling is the same at
    every connectivity."""
    mask = np.zeros(shape, dtype=np.uint8)
    sub = mask[::2, ::2, ::2]
    sub[...] = np.random.default_rng(seed).random(sub.shape) < 0.5
    return _isolated(mask)


def lattice_gap(shape, connectivity=1, seed=22, gap=GAP):
    """lattice_thinned with the voxels [gap[0], gap[1]) cleared: at LARGE one whole lap of zero counts between populated ones."""
    mask = lattice_thinned(shape, connectivity, seed)[0]
    mask.reshape(-1)[gap[0]:gap[1]] = 0
    return _isolated(mask)


CELL, BLOCK, N_BLOCKS = (8, 10, 13), (7, 9, 12), 8


@functools.lru_cache(maxsize=None)
def _blocks():
    rng = np.random.default_rng(23)
    return [(rng.random(BLOCK) < 0.35).astype(np.uint8) for _ in range(N_BLOCKS)]


@functools.lru_cache(maxsize=None)
def _block_labelled(b, crop, connectivity):
    """Block b cut to `crop` (a cell at the volume's far faces), labelled by the flood fill: (mask, labels, the local (z, y, x)
    of every component's first voxel in raster order)."""
    m = np.ascontiguousarray(_blocks()[b][:crop[0], :crop[1], :crop[2]])
    labels, n = CR.label(m, connectivity)
    flat = labels.ravel()
    first = np.full(n + 1, flat.size, dtype=np.int64)
    np.minimum.at(first, flat, np.arange(flat.size))
    return m, labels, np.stack(np.unravel_index(first[1:], labels.shape), axis=1).reshape(n, 3)


def tiled_random(shape, connectivity):
    """Cells of 8 x 10 x 13 voxels, each with one of eight random 7 x 9 x 12 blocks (cycled) and a clear voxel along every axis,
    so a component never leaves its cell: it is (cell, local label), its first voxel is known, and the global number is the
    rank of that voxel's linear index."""
    D, H, W = shape
    mask, labels = np.zeros(shape, dtype=np.uint8), np.zeros(shape, dtype=np.int32)
    cells, firsts = [], []
    grid = [range(0, n, c) for n, c in zip(shape, CELL)]
    for k, (z0, y0, x0) in enumerate((z, y, x) for z in grid[0] for y in grid[1] for x in grid[2]):
        crop = (min(BLOCK[0], D - z0), min(BLOCK[1], H - y0), min(BLOCK[2], W - x0))
        m, local, first = _block_labelled(k % N_BLOCKS, crop, connectivity)
        sl = (slice(z0, z0 + crop[0]), slice(y0, y0 + crop[1]), slice(x0, x0 + crop[2]))
        mask[sl] = m
        cells.append((sl, local, len(first)))
        firsts.append(((first[:, 0] + z0) * H + first[:, 1] + y0) * W + first[:, 2] + x0)
    firsts = np.concatenate(firsts)
    number = np.empty(firsts.size, dtype=np.int32)
    number[np.argsort(firsts)] = np.arange(1, firsts.size + 1, dtype=np.int32)
    at = 0
    for sl, local, n in cells:
        labels[sl] = np.concatenate([np.zeros(1, dtype=np.int32), number[at:at + n]])[local]
        at += n
    return mask, labels, int(firsts.size)


def comb_large(shape, connectivity=1, mirrored=False):
    """component_cases._comb at any shape: teeth along x on every other row of every other slice, joined only by the plane
    x = W - 1 (mirrored: x = 0).  One component whose unions cross every tile seam."""
    mask = np.zeros(shape, dtype=np.uint8)
    mask[0::2, 0::2, :] = 1
    mask[:, :, -1] = 1
    if mirrored:
        mask = np.ascontiguousarray(mask[:, :, ::-1])
    return mask, mask.astype(np.int32), 1


def comb_large_mirrored(shape, connectivity=1):
    return comb_large(shape, connectivity, mirrored=True)


GENERATORS = {"lattice_thinned": lattice_thinned, "lattice_gap": lattice_gap, "tiled_random": tiled_random,
              "comb_large": comb_large, "comb_large_mirrored": comb_large_mirrored}
# the comb is one component at every connectivity; the long union chains are what it is for, and one connectivity runs them
LABEL_CASES = [(name, c) for name in ("lattice_thinned", "lattice_gap", "tiled_random") for c in CONNECTIVITIES] + \
              [("comb_large", 1), ("comb_large_mirrored", 1)]
STATS_CASES = ["tiled_random", "lattice_thinned"]


@functools.lru_cache(maxsize=None)
def large(name, connectivity=1):
    """(mask, expected labels, n) at LARGE; read-only, built once."""
    mask, labels, n = GENERATORS[name](LARGE, connectivity)
    mask.setflags(write=False)
    labels.setflags(write=False)
    return mask, labels, n


def other_mask(shape, seed=24):
    return (np.random.default_rng(seed).random(shape) < 0.4).astype(np.uint8)


def stats(labels, n, other=None):
    """components_restatement.stats without its loop over the voxels: bincount for voxels and hits, minimum.at / maximum.at
    per axis for the boxes.  A label outside 1..n counts nowhere."""
    labels = np.asarray(labels)
    flat = labels.ravel()
    at = np.flatnonzero((flat >= 1) & (flat <= n))
    k = flat[at] - 1
    voxels = np.bincount(k, minlength=n).astype(np.int64)
    hits = None if other is None else np.bincount(k[np.asarray(other).ravel()[at] != 0], minlength=n).astype(np.int64)
    bbox = np.tile(np.array([labels.shape[0], 0, labels.shape[1], 0, labels.shape[2], 0], dtype=np.int32), (n, 1))
    for axis, coord in enumerate(np.unravel_index(at, labels.shape)):
        coord = coord.astype(np.int32)
        np.minimum.at(bbox[:, 2 * axis], k, coord)
        np.maximum.at(bbox[:, 2 * axis + 1], k, coord + 1)
    return voxels, bbox, hits


# element indices of relabel_case's labels that hold a value outside 0..n: the first block, both sides of the lap seam at
# 16384 * 256, the ragged tail
RELABEL_BAD = (3, 200, 255, RELABEL_CAP - 2, RELABEL_CAP - 1, RELABEL_CAP, RELABEL_CAP + 1, RELABEL_NVOX - 30, RELABEL_NVOX - 2,
               RELABEL_NVOX - 1)


@functools.lru_cache(maxsize=None)
def relabel_case():
    """(labels [RELABEL_NVOX] int32, lut [n + 1] int32, n, expected labels, expected mask): random labels in 0..n, a random table
    with zeros, negative and large entries, and at RELABEL_BAD labels below 0 and above n in turn."""
    rng = np.random.default_rng(25)
    n = RELABEL_N
    labels = rng.integers(0, n + 1, size=RELABEL_NVOX).astype(np.int32)
    bad = [-1, n + 1, np.iinfo(np.int32).min, np.iinfo(np.int32).max, -n, n + 7]
    for j, i in enumerate(RELABEL_BAD):
        labels[i] = bad[j % len(bad)]
    lut = rng.integers(-3, 2 * n, size=n + 1).astype(np.int32)
    lut[0] = 0
    lut[rng.choice(np.arange(1, n + 1), n // 4, replace=False)] = 0
    lut[n] = 123456                                         # the last entry is in range: l <= n, not l < n
    labels[RELABEL_CAP + 5] = labels[7] = n
    inside = (labels >= 0) & (labels <= n)
    expected = np.where(inside, lut[np.clip(labels, 0, n)], 0).astype(np.int32)
    out = (labels, lut, n, expected, (expected != 0).astype(np.uint8))
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
