"""The lesion shape tables restated in plain numpy (nothing of dram_amd.shape is imported): the histogram of 2x2x2 neighbourhood
configurations per label from eight shifted views of the zero-padded volume and a bincount, the moments as direct sums, and a
direct count of the lattice pairs that cross a label's boundary."""
import numpy as np

DIRECTIONS = ((1, 0, 0), (0, 1, 0), (0, 0, 1),
              (1, 1, 0), (1, -1, 0), (1, 0, 1), (1, 0, -1), (0, 1, 1), (0, 1, -1),
              (1, 1, 1), (1, 1, -1), (1, -1, 1), (1, -1, -1))


def _valid(labels, n):
    lab = np.asarray(labels).astype(np.int64)
    lab[(lab < 0) | (lab > n)] = 0
    return lab


def tables(labels, n):
    """{"cfg": int64 [n,256], "mom": int64 [n,10]} of include/dram_hip.h (dram_label_shape)."""
    lab = _valid(labels, n)
    D, H, W = lab.shape
    pad = np.pad(lab, 1)
    views = [pad[dz:dz + D + 1, dy:dy + H + 1, dx:dx + W + 1] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]   # bit dz*4 + dy*2 + dx
    some = views[0] > 0
    for v in views[1:]:
        some = some | (v > 0)
    corners = np.stack([v[some] for v in views])                         # [8, occupied cells]
    cfg = np.zeros(n * 256, dtype=np.int64)
    for j in range(8):
        lj = corners[j]
        first = lj > 0                                                   # a label counts once per cell: at its first corner
        c = np.zeros(lj.shape, dtype=np.int64)
        for i in range(8):
            same = corners[i] == lj
            c |= same.astype(np.int64) << i
            if i < j:
                first &= ~same
        cfg += np.bincount((lj[first] - 1) * 256 + c[first], minlength=n * 256)
    z, y, x = np.nonzero(lab)
    k = lab[z, y, x] - 1
    cols = (np.ones_like(z), z, y, x, z * z, y * y, x * x, z * y, z * x, y * x)
    mom = np.zeros((n, 10), dtype=np.int64)
    for e, col in enumerate(cols):
        np.add.at(mom[:, e], k, col.astype(np.int64))
    return {"cfg": cfg.reshape(n, 256), "mom": mom}


def crossings_direct(labels, k):
    """Per direction, the lattice pairs (p, p + v) with exactly one end carrying label k, counted on the padded lattice."""
    a = np.pad(np.asarray(labels).astype(np.int64) == k, 1)
    D, H, W = a.shape
    out = []
    for v in DIRECTIONS:
        lo = [max(0, -s) for s in v]
        hi = [dim - max(0, s) for s, dim in zip(v, (D, H, W))]
        p = a[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        q = a[lo[0] + v[0]:hi[0] + v[0], lo[1] + v[1]:hi[1] + v[1], lo[2] + v[2]:hi[2] + v[2]]
        out.append(int(np.count_nonzero(p != q)))
    return out


def ball(shape, centre, r, spacing):
    """The digitised ball |p - centre| <= r (mm) of a lattice with `spacing`, centre in voxel indices (fractions allowed)."""
    g = np.meshgrid(*(np.arange(s, dtype=np.float64) for s in shape), indexing="ij")
    d2 = sum(((g[a] - centre[a]) * spacing[a]) ** 2 for a in range(3))
    return (d2 <= r * r).astype(np.uint8)
