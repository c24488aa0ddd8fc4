"""Test-time augmentation of the per-lobe inference: a plain numpy fp64 restatement, the cases, the inputs and the
tolerances of tests/test_gpu_tta_kernels.py and tests/test_gpu_tta.py (checked on the host by tests/test_tta_cpu.py).  Host
code only: numpy and torch on the CPU.  Written from the definition in include/dram_hip.h ("test-time augmentation"), not from
the kernels.

Tolerances, by counting roundings as tests/test_surface_cpu.py does.  U = 2^-24 is the unit roundoff of fp32: one fp32 operation
whose result lies in [0, 1] is off by at most U.

  SIGMOID_TOL = 4 U   the sigmoid's own budget as tests/infer_kernel_cases.py states it for PASTE_TOL: expf within 2 ulp, one
                      addition, one division.
  RESIZE_TOL = 11 U   PASTE_TOL's other share: the 8 products and 7 additions of the align-corners combination.  (PASTE_TOL is
                      their sum, 15 U, rounded up to 16 U.)
  mean_tol(V) = SIGMOID_TOL + (V - 1) U + U
                      V - 1 additions and one division.  An addition whose result is at most k rounds by at most k U.  Over
                      the header's binary tree the results of one level add up to at most V, and there are ceil(log2 V)
                      levels: the sum's error is at most U V ceil(log2 V), after the division by V at most U ceil(log2 V)
                      <= (V - 1) U.  (Added left to right it would be U (2 + ... + V) / V <= (V - 1) U as well: the bound
                      does not lean on the tree.)  The division rounds a value in [0, 1]: U.
  pasted mean         mean_tol(V) + RESIZE_TOL: the resize is a convex combination, it does not amplify what it is given.
  var_tol(V)          the check of the spread is on s^2 against the fp64 variance.  e_v = fl(p_v - m) is off by at most
                      d = SIGMOID_TOL + mean_tol(V) + U; |e_v| <= 1, so fl(e_v^2) is off by at most 2 d + d^2 + U.  The sum of V
                      such terms is V var <= V / 4, so each of the V - 1 additions rounds by at most U V / 4; after the division
                      by V: (V - 1) U / 4, and the division itself rounds var <= 1/4: U / 4.
                          var_tol(V) = 2 d + d^2 + U + (V - 1) U / 4 + U / 4
  spread_tol(V, s)    s itself only where the reference s >= S_MIN = 2^-8: |sqrt(a) - sqrt(b)| = |a - b| / (sqrt(a) + sqrt(b))
                      <= var_tol(V) / s, plus the square root's own rounding of a value <= 1/2: U.  Below S_MIN nothing is
                      claimed about s beyond what the bound on s^2 says: the square root of an error near zero is not small
                      (|sqrt(a) - sqrt(b)| <= sqrt(|a - b|) is all there is: `spread_point_tol`)."""
import functools
import itertools
import math

import numpy as np
import torch

import infer_kernel_cases as K
from infer_kernel_cases import MAX_CHUNKS, PASTE_CHUNKS, PASTE_R, PASTE_TOL, U, VOLUME, box
from oracle import dram_oracle as O

MAX_VIEWS = 48
SIGMOID_TOL = 4 * U
RESIZE_TOL = 11 * U
assert SIGMOID_TOL + RESIZE_TOL <= PASTE_TOL
S_MIN = 2.0 ** -8
IDENTITY = ((0, 1, 2), (0, 0, 0))


def mean_tol(V):
    return SIGMOID_TOL + (V - 1) * U + U


def var_tol(V, p_tol=SIGMOID_TOL, m_tol=None):
    d = p_tol + (mean_tol(V) if m_tol is None else m_tol) + U
    return 2 * d + d * d + U + (V - 1) * U / 4 + U / 4


def spread_tol(V, s_ref):
    return var_tol(V) / s_ref + U


def spread_point_tol(vt, s_ref):
    """The bound on |s - s_ref| at every point, given the bound vt on s^2: the smaller of sqrt(vt) and vt / s_ref, plus U."""
    return np.minimum(math.sqrt(vt), vt / np.maximum(s_ref, 1e-300)) + U


# ------------------------------------------------------------------------------------------------ views
FLIPS = tuple(((n >> 2) & 1, (n >> 1) & 1, n & 1) for n in range(8))
FLIP_VIEWS = tuple(((0, 1, 2), f) for f in FLIPS)
FULL_VIEWS = tuple((p, f) for p in itertools.permutations(range(3)) for f in FLIPS)
KEEP_X_VIEWS = tuple(v for v in FULL_VIEWS if v[0][2] == 2)       # 16
MOVE_X_VIEWS = tuple(v for v in FULL_VIEWS if v[0][2] != 2)       # 32
CYCLE_VIEW = ((1, 2, 0), (1, 0, 0))                               # a 3-cycle: its inverse is another permutation


def apply_view(x, view):
    """viewed[..., o] = x[..., i] with i[perm[k]] = flip[k] ? n-1-o[k] : o[k] over the last three axes."""
    perm, flip = view
    shape = x.shape[-3:]
    o = np.indices(tuple(shape[perm[k]] for k in range(3)), sparse=True)
    i = [None] * 3
    for k in range(3):
        i[perm[k]] = (shape[perm[k]] - 1 - o[k]) if flip[k] else o[k]
    return x[(Ellipsis,) + tuple(np.broadcast_arrays(*i))]


def inverse_view(view):
    """The view that undoes `view`: o[k] = F_k(i[perm[k]]) read as a move from the viewed array back."""
    perm, flip = view
    inv = [perm.index(a) for a in range(3)]
    return tuple(inv), tuple(flip[inv[a]] for a in range(3))


def compose_views(first, then):
    """The single view equal to apply_view(apply_view(x, first), then)."""
    (p1, f1), (p2, f2) = first, then
    # y[m] = x[i], i[p1[k]] = F1_k(m[k]);  z[o] = y[m], m[p2[k]] = F2_k(o[k])  ->  i[p1[p2[k]]] = F1_{p2[k]}(F2_k(o[k]))
    return tuple(p1[p2[k]] for k in range(3)), tuple(f1[p2[k]] ^ f2[k] for k in range(3))


def views_arg(views):
    import ctypes
    flat = [int(a) for perm, flip in views for a in tuple(perm) + tuple(flip)]
    return (ctypes.c_int * len(flat))(*flat)


# ------------------------------------------------------------------------------------------------ combine
def combine_ref(dense, views, mutate=None):
    """dense [V, L, R, R, R] (fp32 logits) -> (m, var, s) [L, R, R, R] in fp64: p_v(i) = sigmoid(dense[v][l][o_v(i)]), m the
    mean over the views, var the population variance, s its square root.  `mutate` plants one mistake (test_tta_cpu.py shows
    that each moves the result by more than ten tolerances):
      "forward"  the view's own move in place of its inverse on the way back to the canonical grid
      "noflip"   the flips dropped on the way back
      "logits"   the logits averaged, the sigmoid taken of the average
      "sample"   division by V - 1 in the variance"""
    V = len(views)
    assert dense.shape[0] == V
    d = dense.astype(np.float64)
    back = []
    for v, view in enumerate(views):
        w = inverse_view(view)
        if mutate == "forward":
            w = view
        elif mutate == "noflip":
            w = (w[0], (0, 0, 0))
        back.append(apply_view(d[v], w))
    z = np.stack(back)
    p = 1.0 / (1.0 + np.exp(-z))
    m = 1.0 / (1.0 + np.exp(-z.mean(0))) if mutate == "logits" else p.mean(0)
    var = ((p - m) ** 2).sum(0) / ((V - 1) if mutate == "sample" else V)
    return m, var, np.sqrt(var)


def tree_sum32(terms):
    """The header's sum of V fp32 arrays over the binary tree of the view index, operation by operation in fp32 on the host:
    complete aligned blocks of 2^k views summed pairwise, the blocks that V's binary digits leave joined from the last upwards."""
    terms = [np.asarray(t, dtype=np.float32) for t in terms]

    def block(lo, n):
        return terms[lo] if n == 1 else block(lo, n // 2) + block(lo + n // 2, n // 2)
    blocks, lo = [], 0
    for b in reversed(range(len(terms).bit_length())):
        if (len(terms) >> b) & 1:
            blocks.append(block(lo, 1 << b))
            lo += 1 << b
    acc = blocks[-1]
    for blk in reversed(blocks[:-1]):
        acc = blk + acc
    assert acc.dtype == np.float32
    return acc


def sigmoid32(d):
    """lobe_paste_kernel's expression in fp32 on the host: 1 / (1 + exp(-d))."""
    d = np.asarray(d, dtype=np.float32)
    out = np.float32(1) / (np.float32(1) + np.exp(-d))
    assert out.dtype == np.float32
    return out


# name -> (R, L, views, how dense is made)
#   "equivariant": dense[v] = view_v(dense[0]): every view shows the same probabilities
#   "random":      independent logits per view, uniform in [-12, 12] with +-40 planted
SHAPES = ((12, 3), (10, 8))       # R^3 = 1728 and 1000: no multiple of a block, boxes cut on every axis; L = 8 x 48 views
EQUIVARIANT_EXACT = {2: (FULL_VIEWS[0], FULL_VIEWS[29]), 4: FULL_VIEWS[0::13][:4], 8: FULL_VIEWS[0::6]}
EQUIVARIANT_ULP = {3: (FULL_VIEWS[0], FULL_VIEWS[20], FULL_VIEWS[40]), 48: FULL_VIEWS}
RANDOM_CASES = {"full48": FULL_VIEWS, "flip8": FLIP_VIEWS, "move_x_32": MOVE_X_VIEWS, "keep_x_16": KEEP_X_VIEWS,
                "cycle_3": (IDENTITY, CYCLE_VIEW, CYCLE_VIEW), "eleven": FULL_VIEWS[5::4][:11]}


@functools.lru_cache(maxsize=None)
def base_logits(R, L):
    a = (4.0 * np.random.default_rng(100 + R + L).standard_normal((L, R, R, R))).astype(np.float32)
    a.setflags(write=False)
    return a


def equivariant_dense(R, L, views):
    return np.ascontiguousarray(np.stack([apply_view(base_logits(R, L), v) for v in views]))


@functools.lru_cache(maxsize=None)
def random_dense(R, L, name):
    V = len(RANDOM_CASES[name])
    g = np.random.default_rng(200 + R + L + V)
    d = g.uniform(-12.0, 12.0, size=(V, L, R, R, R)).astype(np.float32)
    flat = d.reshape(-1)
    where = g.choice(flat.size, size=max(8, flat.size // 50), replace=False)
    flat[where] = np.where(g.random(where.size) < 0.5, -40.0, 40.0).astype(np.float32)
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def random_reference(R, L, name):
    return combine_ref(random_dense(R, L, name), RANDOM_CASES[name])


# ------------------------------------------------------------------------------------------------ paste of probabilities
def paste_prob_inputs():
    """Two fields (3, R, R, R) in [0, 1] and [0, 1/2] -- a mean and a spread --, and the lobe map of K.paste_inputs()."""
    g = K.rng(33)
    shape = (len(PASTE_CHUNKS), PASTE_R, PASTE_R, PASTE_R)
    prob = g.random(shape, dtype=np.float32)
    prob2 = (0.5 * g.random(shape, dtype=np.float32)).astype(np.float32)
    _, lobe, _ = K.paste_inputs()
    return prob, prob2, lobe


def paste_prob_ref(prob, lobe, chunks, R, htp0, mutate=None):
    """(htp float64, written bool): a copy of htp0 with the align-corners resize of prob[l] written where lobe == label inside
    chunk l's box, the chunks in order (K.lobe_paste_ref without the sigmoid).  mutate="nolobe": the lobe test dropped."""
    htp = np.asarray(htp0, dtype=np.float64).copy()
    written = np.zeros(htp.shape, dtype=bool)
    for l, c in enumerate(chunks):
        assert prob[l].shape == (R, R, R)
        field = K.trilinear_ac_ref(prob[l].astype(np.float64), c[3:6])
        sel = np.ones(field.shape, dtype=bool) if mutate == "nolobe" else lobe[box(c)] == c[6]
        htp[box(c)][sel] = field[sel]
        written[box(c)][sel] = True
    return htp, written


# ------------------------------------------------------------------------------------------------ end to end
SCAN_ARGS = ((41, 57, 66), (2.5, 1.0, 1.0))
SCAN_R = 16
MODEL_TOL = 1e-4       # tests/test_gpu_inference.py::test_lobe_inference_matches_oracle: the device model against the oracle's


def slim_model(norm="bn"):
    """The `_model` recipe of tests/test_gpu_inference.py (copied): the slim DC3D, HeNorm-initialised, with non-trivial running
    statistics so that eval-mode BatchNorm is exercised.  On the CPU; the caller moves it."""
    import models
    from dram_amd.configs import SLIM
    torch.manual_seed(3)
    m = models.DC3D(**SLIM, norm_method=norm)
    m.init(models.HeNorm(mode="fan_in"))
    g = torch.Generator().manual_seed(4)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm3d):
            mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g) * 0.1)
            mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) + 0.5)
    return m


@functools.lru_cache(maxsize=None)
def scan_inputs():
    from dram_amd.inference import synthetic_ct
    return synthetic_ct(*SCAN_ARGS, seed=7, n_lesions=8)       # shared: nobody writes to it


def htp_tol(V):
    """The heat map end to end: the existing test's tolerance (the model's share) plus the ensemble's and the resize's."""
    return MODEL_TOL + mean_tol(V) + RESIZE_TOL


def e2e_var_tol(V):
    """s^2 end to end: every probability is off by at most MODEL_TOL + SIGMOID_TOL, the mean by no more than that plus its own
    additions and division."""
    return var_tol(V, p_tol=MODEL_TOL + SIGMOID_TOL, m_tol=MODEL_TOL + mean_tol(V))


def run_tta_ref(cfg, params, buffers, scan, lobe, spacing, views, resample, norm_method="bn", window=(-1000.0, -300.0),
                border=5.0, forward=None):
    """O.evaluate_scan with the ensemble in the middle, from the oracle's own pieces in the order evaluate_scan uses them:
    find_crops, windowing, resample_itk_linear, the forward on every view of the chunk (apply_view), torch.sigmoid, each map
    taken back to the canonical grid (inverse_view), mean and population standard deviation over the views in fp64 at the
    chunk's resolution, both rounded once to fp32, resized by the oracle's upsample_trilinear_ac (what evaluate_scan calls;
    np_trilinear_ac is the same rule in another summation order and would not reproduce evaluate_scan bit for bit) and pasted
    where the lobe is; then binary_cam.  With the identity as the only view every step is evaluate_scan's and the result is
    equal to it exactly.  Returns a dict: htp, spread (float32 [D,H,W]), mask, threshold, ratio and, per label, the chunk-level
    fp64 `s` (for the point-wise bound on the spread)."""
    V = len(views)
    htp = np.zeros(scan.shape, dtype=np.float32)
    spread = np.zeros(scan.shape, dtype=np.float32)
    chunk_s, crops = {}, {}
    with torch.no_grad():
        for label in np.unique(lobe)[1:]:
            lobe_binary = lobe == label
            sl = O.find_crops(lobe_binary, spacing, border)
            lobe_chunk = lobe_binary[sl]
            scan_chunk = scan[sl].astype(np.float32).copy()
            scan_chunk[lobe_chunk == 0] = -2048
            img = O.windowing(scan_chunk, from_span=window, to_span=(0.0, 1.0)).astype(np.float32)
            chunk = O.resample_itk_linear(img, (resample,) * 3)
            probs = []
            for view in views:
                t = torch.from_numpy(np.ascontiguousarray(apply_view(chunk, view)))[None, None]
                dense = forward(t) if forward is not None else \
                    O.dc3d_forward(cfg, params, buffers, t, training=False, norm_method=norm_method)
                p = torch.sigmoid(dense)[0, 0].numpy()
                probs.append(apply_view(p, inverse_view(view)).astype(np.float64))
            p = np.stack(probs)
            m = p.sum(0) / V
            s = np.sqrt(((p - m) ** 2).sum(0) / V)
            for field, out in ((m, htp), (s, spread)):
                t = torch.from_numpy(np.ascontiguousarray(field.astype(np.float32)))[None, None]
                up = O.upsample_trilinear_ac(t, size=tuple(lobe_chunk.shape))[0, 0].numpy()
                view_out = out[sl]
                view_out[lobe_chunk] = up[lobe_chunk]
            chunk_s[int(label)], crops[int(label)] = s, sl
    lung = lobe > 0
    _, th = O.binary_cam(htp[lung])
    return {"htp": htp, "spread": spread, "mask": htp > th, "threshold": th, "ratio": float((htp * lung).sum() / lung.sum()),
            "chunk_s": chunk_s, "crops": crops}


def spread_bound_map(ref, lobe, vt):
    """[D,H,W] fp64: the point-wise bound on |spread - ref["spread"]| -- spread_point_tol at the chunk's resolution, resized
    like the spread itself (a convex combination of the chunk-level errors) plus the resize's own RESIZE_TOL and the U / 2 of
    the reference's rounding to fp32; 0 outside the lobes."""
    out = np.zeros(lobe.shape, dtype=np.float64)
    for label, s in ref["chunk_s"].items():
        sl = ref["crops"][label]
        sel = lobe[sl] == label
        b = K.trilinear_ac_ref(spread_point_tol(vt, s), sel.shape) + RESIZE_TOL + U
        out[sl][sel] = b[sel]
    return out
