"""The named cases of the lesion shape tests, each at the smallest shape at which its failure can still show, and the
restatement's tables for each, computed once and shared between the CPU and GPU tests.

A case is {labels uint8 | int32 [D,H,W], n}.  Which kernel a case takes is decided by dram_label_shape_plan(label_kind, n) alone
(0: table in LDS, 1: runs reduced within a wave); `variants` lists every (label kind, n) at which a case is run: its own kind
and the other one where the labels fit, its own n and, to force the other plan, n raised to the first n past the LDS regime
(found by asking the library; the expected tables are the restatement's at that n).

The kernel takes tiles of 16 x 16 cell rows and marches along x in chunks of 128 bytes per row (128 uint8 or 32 int32 voxels),
a segment of at least two chunks per work item, 512 blocks at most."""
import functools

import numpy as np

import shape_restatement as SR

W_VALUES = (1, 2, 63, 64, 65)


def plan(label_kind, n):
    from dram_amd import _lib
    return _lib.lib.dram_label_shape_plan(label_kind, n)


@functools.lru_cache(maxsize=None)
def first_n_past_lds():
    n = 1
    while plan(1, n) == 0:
        n += 1
    return n


def _blobs(shape, count, seed, dtype):
    rng = np.random.default_rng(seed)
    lab = np.zeros(shape, dtype=dtype)
    g = np.meshgrid(*(np.arange(s, dtype=np.float64) for s in shape), indexing="ij")
    for k in range(1, count + 1):
        c = [rng.uniform(0, s - 1) for s in shape]
        r = [rng.uniform(1.5, max(2.0, min(9.0, s / 3.0))) for s in shape]
        inside = sum(((g[a] - c[a]) / r[a]) ** 2 for a in range(3)) <= 1.0
        lab[inside & (rng.random(shape) < 0.97)] = k                     # later blobs overwrite earlier ones; a few holes
    return lab


@functools.lru_cache(maxsize=None)
def case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "one_voxel":
        lab, n = np.ones((1, 1, 1), np.uint8), 1
    elif name == "corner_voxel":
        lab, n = np.zeros((3, 4, 5), np.uint8), 1
        lab[2, 3, 4] = 1
    elif name == "full_box":
        lab, n = np.ones((3, 4, 5), np.uint8), 1
    elif name == "diagonal_pair":                                        # two labels that meet diagonally inside one cell
        lab, n = np.zeros((4, 4, 4), np.uint8), 2
        lab[1, 1, 1], lab[2, 2, 2] = 1, 2
    elif name == "cavity":
        lab, n = np.ones((5, 5, 5), np.uint8), 1
        lab[2, 2, 2] = 0
    elif name == "ring":
        lab, n = np.ones((1, 5, 5), np.uint8), 1
        lab[0, 1:4, 1:4] = 0
    elif name == "above_n_u8":                                           # labels above n and zeros mixed in
        lab, n = rng.integers(0, 10, size=(5, 6, 7)).astype(np.uint8), 5
        lab[0, 0, :3] = (255, 6, 5)
    elif name == "above_n_i32":
        lab, n = rng.integers(-2, 10, size=(5, 6, 7)).astype(np.int32), 5
        lab[0, 0, :4] = (-1, 1 << 30, -(1 << 31), 6)
    elif name == "random_u8":
        lab, n = rng.integers(0, 6, size=(7, 9, 11)).astype(np.uint8), 5
    elif name == "random_i32_300":                                       # about 300 small labels: plan 1 at its own n
        lab, n = np.zeros((20, 24, 28), np.int32), 300
        blocks = rng.integers(1, 301, size=(5, 6, 7))                    # 4 x 4 x 4 blocks, each of one label, a third of them empty
        lab[:] = np.kron(blocks, np.ones((4, 4, 4), dtype=np.int64)).astype(np.int32)
        lab[rng.random(lab.shape) < 0.35] = 0
    elif name == "blobs":                                                # several tiles, several blocks, two chunks of uint8
        lab, n = _blobs((40, 72, 136), 12, 5, np.uint8), 12
    elif name == "wide_u8":                                              # three chunks of uint8: two segments, one starts inside the row
        lab, n = _blobs((3, 18, 300), 9, 6, np.uint8), 9
    elif name == "grid_stride_i32":                                      # 2 tiles x 257 segments = 514 work items for 512 blocks
        lab, n = _blobs((2, 17, 16420), 7, 7, np.int32), 7
        lab[rng.random(lab.shape) < 0.002] = 3
    elif name.startswith("w"):
        lab, n = rng.integers(0, 4, size=(3, 5, int(name[1:]))).astype(np.uint8), 3
    else:
        raise KeyError(name)
    lab.setflags(write=False)
    return {"labels": lab, "n": n}


def names():
    return ["one_voxel", "corner_voxel", "full_box", "diagonal_pair", "cavity", "ring", "above_n_u8", "above_n_i32", "random_u8",
            "random_i32_300", "blobs", "wide_u8", "grid_stride_i32"] + [f"w{w}" for w in W_VALUES]


@functools.lru_cache(maxsize=None)
def expected(name, n=None):
    """The restatement's tables of a case at its own n, or at a raised n (labels of the volume up to it then count)."""
    c = case(name)
    t = SR.tables(c["labels"], c["n"] if n is None else n)
    for v in t.values():
        v.setflags(write=False)
    return t


def variants(name):
    """[(label kind, n)]: both kinds where the case allows it, both plans."""
    c = case(name)
    lab, n = c["labels"], c["n"]
    kinds = [0 if lab.dtype == np.uint8 else 1]
    if lab.dtype == np.uint8:
        kinds.append(1)
    elif lab.min() >= 0 and lab.max() <= 255 and n <= 255:
        kinds.append(0)
    past = first_n_past_lds()
    out = []
    for kind in kinds:
        for m in sorted({n, max(n, past)} | ({past - 1} if n < past else set())):
            if not (kind == 0 and m > 255):
                out.append((kind, m))
    return out


def as_kind(labels, kind):
    return np.ascontiguousarray(labels, dtype=np.uint8 if kind == 0 else np.int32)
