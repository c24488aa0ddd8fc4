"""Cases, inputs and a float64 restatement for the six PCM entry points of csrc/pcm.hip (host only: torch on the CPU).

Shared by tests/test_pcm_kernels_cpu.py and tests/test_gpu_pcm_kernels.py.  Three things live here:
  * the restatement: attention_split / attention_sum / aggregate in plain torch, generic in dtype, on dense tensors and an
    ARBITRARY list of integer offsets (shifted, zero-padded views as in oracle.dram_oracle.pcm_forward; nothing assumes that
    the offset set equals its mirror image).  The raw per-edge quantities are kept as graph nodes, so torch.autograd in
    float64 gives the intermediates the kernels write (ds, ds2) next to dtheta, dphi, dattn and dv;
  * the inputs: made so that float32 and float64 take every discrete decision alike (see *_inputs);
  * the cases, each with a comment that says which kernel, launch or branch it reaches.

One grid serves every case: (D, H, W) = (5, 9, 13), B = 2.  S = 585 nodes: blockIdx.x = 0 and 1 are full blocks of 256, block 2
holds 73 nodes and 183 idle threads; blockIdx.y (or .z) = 1 is the second sample.  The three extents differ, so a swapped
stride cannot cancel."""
from collections import namedtuple
from functools import lru_cache

import torch
import torch.nn.functional as F

from oracle import dram_oracle as O

GRID, B = (5, 9, 13), 2
S = GRID[0] * GRID[1] * GRID[2]
PCM_RELU, PCM_L2NORM = 1, 2                         # flags (csrc/pcm.hip)
SCALE_NONE, SCALE_RSQRT_DEG, SCALE_100 = 0, 1, 2    # scale_mode
SUM_COSINE, SUM_HEU1, SUM_HEU2 = 0, 1, 2            # dram_pcm_attention_sum_* mode
L2EPS, COS_EPS, HEU_EPS = 1e-12, 1e-8, 1e-7
MARGIN = 4.0              # kernel error <= MARGIN * e32 (tests/test_gpu_oneshot_shapes.py)
FLOOR = 1e-6              # relative floor where e32 == 0
ZERO_NODE = (1, 2, 5, 1)  # (b, z, y, x) of the theta = 0 node of the L2 cases: flat index 300, in block 1, 18 edges on k3
ZERO_NODE_DATTN = 2.0 ** -40


# ------------------------------------------------------------------------------------------------ offset sets
def _k3():
    return [tuple(int(v) for v in o) for o in O.pcm_offsets(3, 2, False)]


def _k5():
    return [tuple(int(v) for v in o) for o in O.pcm_offsets(5, 3, True)]


def _skew():
    """128 offsets, the table limit, in a scrambled order.  Built from four groups:
      a) 70: dz in {1, 2}, dy in -2..2, dx in -3..3;
      b) 19: dz = 0 with dy in {2, 3}, dx in -2..2, or with dy in -1..1, dx in {2, 3, 4};
      c) 23: dz = 3 with dy in {-6, -3, 0, 3, 6}, dx in {-6, -2, 2, 6} (|6| leaves H = 9 from most rows and W = 13 from
         about half of the columns), and three with dz = 4;
      d) 16 with |dz| in {5, 6}: never inside D = 5; eight of them are the mirror images of the other eight.
    Apart from d) every offset points to a later plane, a later row or a later column, so its mirror image is absent, and
    the nodes with z = 4, y >= 7, x >= 11 have no edge inside the grid."""
    a = [(dz, dy, dx) for dz in (1, 2) for dy in range(-2, 3) for dx in range(-3, 4)]
    b = [(0, dy, dx) for dy in (2, 3) for dx in range(-2, 3)] + [(0, dy, dx) for dy in (-1, 0, 1) for dx in (2, 3, 4)]
    c = [(3, dy, dx) for dy in (-6, -3, 0, 3, 6) for dx in (-6, -2, 2, 6)] + [(4, 0, 0), (4, 1, -1), (4, -1, 1)]
    half = [(5, 0, 0), (6, 0, 0), (5, 1, 2), (6, 1, -1), (5, -2, 3), (6, 2, 2), (5, 0, -1), (6, -3, 0)]
    d = half + [(-z, -y, -x) for z, y, x in half]
    offs = a + b + c + d
    perm = torch.randperm(len(offs), generator=torch.Generator().manual_seed(128)).tolist()
    return [offs[i] for i in perm]


OFFSETS = {"k3": _k3(), "k5": _k5(), "skew": _skew()}


class Stencil:
    """Shifted, zero-padded views of [B, C, D, H, W] tensors for a list of offsets."""

    def __init__(self, offsets, grid):
        self.offs = [tuple(int(v) for v in o) for o in offsets]
        self.grid = tuple(int(v) for v in grid)
        self.R = max(1, max(abs(v) for o in self.offs for v in o))

    def pad(self, t):
        return F.pad(t, (self.R,) * 6)

    def view(self, tp, o):
        """tp = pad(t): t at node + o, zero outside the grid."""
        R, (D, H, W) = self.R, self.grid
        return tp[..., R + o[0]:R + o[0] + D, R + o[1]:R + o[1] + H, R + o[2]:R + o[2] + W]

    def shifted(self, t, o):
        return self.view(self.pad(t), o)

    def valid(self, dtype=torch.float64):
        """[1, E, D, H, W]: 1 where node + o_e lies inside the grid."""
        ones = self.pad(torch.ones((1, 1) + self.grid, dtype=dtype))
        return torch.cat([self.view(ones, o) for o in self.offs], dim=1)


# ------------------------------------------------------------------------------------------------ the restatement
def _edge_dots(st, theta, php, lo, hi, leaf):
    """[B, E, D, H, W]: sum_{lo <= f < hi} theta_f(i) * phi_f(i + o_e); 0 at non-edges (phi is zero-padded)."""
    if hi <= lo:
        z = torch.zeros((theta.shape[0], len(st.offs)) + st.grid, dtype=theta.dtype)
        return z.requires_grad_(True) if leaf else z
    return torch.stack([(theta[:, lo:hi] * st.view(php[:, lo:hi], o)).sum(1) for o in st.offs], dim=1)


def attention_split(theta, phi, offsets, flags, scale_mode, F_relu, keep=None):
    """dram_pcm_attention_split_fwd: [B, E, D, H, W] = softmax over node i's in-grid edges of
    scale(deg_i) * n_i( act(sum_{f < F_relu} theta_f phi_f) + sum_{f >= F_relu} theta_f phi_f ).
    A non-edge has weight exactly 0; a node without an in-grid edge has a zero row.
    keep (a dict): receives the two raw dots as graph nodes with retained gradients -- "dot_act" (its gradient is the
    kernel's ds: behind the ReLU gate, subgradient 0 at 0) and "dot_raw" (its gradient is ds2)."""
    st = Stencil(offsets, theta.shape[2:])
    valid = st.valid(theta.dtype)
    deg = valid.sum(1, keepdim=True)
    php = st.pad(phi)
    d1 = _edge_dots(st, theta, php, 0, F_relu, keep is not None)
    d2 = _edge_dots(st, theta, php, F_relu, theta.shape[1], keep is not None)
    if keep is not None:
        for t in (d1, d2):
            if t.requires_grad:
                t.retain_grad()
        keep["dot_act"], keep["dot_raw"] = d1, d2
    u = (F.relu(d1) if flags & PCM_RELU else d1) + d2
    if flags & PCM_L2NORM:      # F.normalize over the node's edges; vector_norm's gradient at the zero vector is 0
        u = u / torch.linalg.vector_norm(u * valid, dim=1, keepdim=True).clamp_min(L2EPS)
    if scale_mode == SCALE_RSQRT_DEG:
        u = u / torch.sqrt(deg.clamp_min(1.0))
    elif scale_mode == SCALE_100:
        u = u * 100.0
    # an edgeless node: every entry takes part in the softmax (finite), then `* valid` makes the row and its gradient 0
    logits = torch.where(valid.bool() | (deg == 0), u, torch.full_like(u, float("-inf")))
    return torch.softmax(logits, dim=1) * valid


def attention_sum(theta, phi, offsets, mode, keep=None):
    """dram_pcm_attention_sum_fwd (the comment above pcm_sum_value): a_e = v_e / (eps + sum_k v_k) over the in-grid edges,
      cosine: v = theta.phi / (max(|theta|, 1e-8) max(|phi|, 1e-8)), eps = 0
      heu1:   u = theta.phi / (1 + |theta - phi|_1), v = u where u >= 0.03 else 0 (a constant gate), eps = 1e-7
      heu2:   v = relu(u), eps = 1e-7
    keep["v"]: the per-edge similarities as a graph node; its gradient is the kernel's ds."""
    st = Stencil(offsets, theta.shape[2:])
    valid = st.valid(theta.dtype)
    php = st.pad(phi)
    vs = []
    for o in st.offs:
        q = st.view(php, o)
        dot = (theta * q).sum(1)
        if mode == SUM_COSINE:      # (vector_norm, not sqrt(sum): its gradient at the zero padding is 0, not NaN)
            v = dot / (torch.linalg.vector_norm(theta, dim=1).clamp_min(COS_EPS) * torch.linalg.vector_norm(q, dim=1).clamp_min(COS_EPS))
        else:
            u = dot / (1.0 + (theta - q).abs().sum(1))
            v = u * (~(u < 0.03)).to(u.dtype).detach() if mode == SUM_HEU1 else F.relu(u)
        vs.append(v)
    v_raw = torch.stack(vs, dim=1)
    if keep is not None:
        if v_raw.requires_grad:
            v_raw.retain_grad()
        keep["v"] = v_raw
    v = v_raw * valid
    return v / ((0.0 if mode == SUM_COSINE else HEU_EPS) + v.sum(1, keepdim=True))


def aggregate(attn, v, offsets):
    """dram_pcm_aggregate_fwd: out[b, c, i] = sum_e attn[b, e, i] * v[b, c, i + o_e]."""
    st = Stencil(offsets, v.shape[2:])
    vp = st.pad(v)
    return sum(attn[:, e:e + 1] * st.view(vp, o) for e, o in enumerate(st.offs))


def scatter_adjoint(w, src, offsets):
    """pcm_scatter_adjoint_kernel: out[b, c, j] = sum_e w[b, e, j - o_e] * src[b, c, j - o_e]."""
    st = Stencil(offsets, src.shape[2:])
    return sum(st.shifted(w[:, e:e + 1] * src, tuple(-c for c in o)) for e, o in enumerate(st.offs))


# ------------------------------------------------------------------------------------------------ cases
SplitCase = namedtuple("SplitCase", "id offs F flags scale F_relu seed")
SumCase = namedtuple("SumCase", "id offs F mode seed")
AggCase = namedtuple("AggCase", "id offs C seed")

# dram_pcm_attention_split_fwd -> pcm_attn_fwd_kernel; _bwd -> pcm_attn_bwd_kernel + pcm_scatter_adjoint_kernel.
# Every case: three blocks along x (blockIdx.x = 0, 1, 2) and blockIdx.y = 0, 1 (B = 2).
SPLIT_CASES = [
    # the seven (flags, scale_mode) pairs of functional.PCM_MERGE_MODES, F_relu = F = 5: one adjoint launch, c_lo = 0
    SplitCase("sm", "k3", 5, 0, SCALE_NONE, 5, 11),                                   # no activation, scale 1
    SplitCase("scaled_dot_product", "k3", 5, 0, SCALE_RSQRT_DEG, 5, 12),              # 1/sqrt(deg): deg 6, 9, 13, 18 on this grid
    SplitCase("scaled_dot_product_relu", "k3", 5, PCM_RELU, SCALE_RSQRT_DEG, 5, 13),  # the ReLU gate of pass C
    SplitCase("smrelu", "k3", 5, PCM_RELU, SCALE_NONE, 5, 14),
    SplitCase("smscaled", "k3", 5, 0, SCALE_100, 5, 15),                              # scale 100 (inputs 8x finer and smaller)
    SplitCase("l2sm", "k3", 5, PCM_L2NORM, SCALE_NONE, 5, 16),                        # pass B (vdv); ZERO_NODE: the PCM_L2EPS clamp
    SplitCase("l2smrelu", "k3", 5, PCM_RELU | PCM_L2NORM, SCALE_NONE, 5, 17),         # both flags
    # the split activation: ds2 is written, dtheta reads ds for f < 3 and ds2 above, two adjoint launches (c_lo = 0 on
    # ds and channels 0..2, c_lo = 3 on ds2 and channels 3..4)
    SplitCase("relu_split3", "k3", 5, PCM_RELU, SCALE_RSQRT_DEG, 3, 18),
    # nothing inside the activation: ds is all zero, the first adjoint launch is skipped, the second has c_lo = 0
    SplitCase("relu_split0", "k3", 5, PCM_RELU, SCALE_RSQRT_DEG, 0, 19),
    # F_relu < F without a ReLU: the forward adds the two partial dots, the backward runs unsplit (ds2 null)
    SplitCase("plain_split3", "k3", 5, 0, SCALE_RSQRT_DEG, 3, 20),
    # one feature plane, the 125-offset stencil with a self loop (offsets up to +-2: wider than the z-halo of a plane)
    SplitCase("k5_f1", "k5", 1, 0, SCALE_RSQRT_DEG, 1, 21),
    # E = 128, the table limit; asymmetric offsets (i + o_e forward against j - o_e in the adjoint), offsets that never
    # land inside the grid, nodes without any edge (the deg == 0 branch of the forward, scale = 0 in the backward)
    SplitCase("skew", "skew", 5, 0, SCALE_RSQRT_DEG, 5, 22),
    SplitCase("skew_relu", "skew", 5, PCM_RELU, SCALE_RSQRT_DEG, 5, 23),
]

# dram_pcm_attention_sum_fwd -> pcm_attn_sum_fwd_kernel; _bwd -> pcm_attn_sum_bwd_kernel + pcm_attn_sum_dphi_kernel
SUM_CASES = [
    SumCase("cosine", "k3", 5, SUM_COSINE, 31),     # the norm clamps' `live` branch
    SumCase("heu1", "k3", 5, SUM_HEU1, 32),         # backward through the ABI: the 0.03 gate as a constant (gt = 0 / 1)
    SumCase("heu2", "k3", 5, SUM_HEU2, 33),
    SumCase("heu2_k5_f64", "k5", 64, SUM_HEU2, 34),        # F = PCM_SUM_MAXF: all of acc[64]; 125 offsets
    SumCase("cosine_k5_f64", "k5", 64, SUM_COSINE, 35),
]

# dram_pcm_aggregate_fwd -> pcm_aggregate_fwd_kernel (blockIdx.y = channel, .z = sample);
# _bwd -> pcm_aggregate_dattn_kernel + pcm_scatter_adjoint_kernel (gridDim.y = C, c_lo = 0)
AGG_CASES = [
    AggCase("k3_c1", "k3", 1, 41),
    AggCase("k3_c7", "k3", 7, 42),
    AggCase("skew_c1", "skew", 1, 43),              # E = 128, asymmetric: dv gathers at j - o_e
    AggCase("skew_c7", "skew", 7, 44),
]
CASES = {c.id: c for c in SPLIT_CASES}
CASES.update({c.id: c for c in SUM_CASES})
CASES.update({"agg_" + c.id: c for c in AGG_CASES})
assert len(CASES) == len(SPLIT_CASES) + len(SUM_CASES) + len(AGG_CASES)


def is_split(c):
    """The host's `split`: two gradients per edge only with an activation that covers a part of the planes."""
    return c.F_relu < c.F and bool(c.flags & PCM_RELU)


# ------------------------------------------------------------------------------------------------ inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _dyadic(shape, g, step, lim, positive=False):
    """Random nonzero multiples of `step` in [-lim, lim] (float64, exactly representable in float32)."""
    n = int(round(lim / step))
    k = torch.randint(1, n + 1, shape, generator=g).double()
    if not positive:
        k = k * (torch.randint(0, 2, shape, generator=g).double() * 2.0 - 1.0)
    return k * step


def _rounded(t):
    """float64 holding the float32 rounding of t."""
    return t.float().double()


@lru_cache(maxsize=None)
def split_inputs(cid):
    """(theta, phi, dattn) in float64, every value a float32 number.  theta, phi: nonzero multiples of 1/8 in [-2, 2]
    (scale_mode 100: of 1/64 in [-1/4, 1/4], so that 100 * logit does not saturate the softmax): every dot is exact in
    float32 and the ReLU gate, exact zeros included, falls alike in both precisions.  L2 cases: theta = 0 at ZERO_NODE (all
    its dots 0: ss = 0, the PCM_L2EPS clamp, l2live == false); dattn is scaled by 2^-40 there, an exact operation, so that
    the 1 / PCM_L2EPS in that node's gradient gives a ds of order one -- at order 1e12 its 18 values alone would decide
    both error measures of ds and dtheta."""
    c = CASES[cid]
    g = _gen(c.seed)
    step, lim = (1.0 / 64, 0.25) if c.scale == SCALE_100 else (0.125, 2.0)
    theta = _dyadic((B, c.F) + GRID, g, step, lim)
    phi = _dyadic((B, c.F) + GRID, g, step, lim)
    dattn = _rounded(torch.randn((B, len(OFFSETS[c.offs])) + GRID, generator=g, dtype=torch.float64))
    if c.flags & PCM_L2NORM:
        b, z, y, x = ZERO_NODE
        theta[b, :, z, y, x] = 0.0
        dattn[b, :, z, y, x] *= ZERO_NODE_DATTN
    return theta, phi, dattn


def heu_integers(theta, phi, offsets):
    """For theta, phi in multiples of 1/8: integer tensors (k, m, valid) with u = k / (64 + 8 m) per edge."""
    st = Stencil(offsets, theta.shape[2:])
    t8, p8 = theta * 8.0, st.pad(phi * 8.0)
    k = torch.stack([(t8 * st.view(p8, o)).sum(1) for o in st.offs], dim=1)
    m = torch.stack([(t8 - st.view(p8, o)).abs().sum(1) for o in st.offs], dim=1)
    return k, m, st.valid().expand_as(k).bool()


def sum_input_conditions(c, theta, phi):
    """What SUM inputs must satisfy (asserted for every case in tests/test_pcm_kernels_cpu.py): (no heu1 tie at 0.03, the
    smallest per-node sum of similarities)."""
    offs = OFFSETS[c.offs]
    with torch.no_grad():
        row = (attention_sum_raw(theta, phi, offs, c.mode)).sum(1)
    tie = False
    if c.mode == SUM_HEU1:
        k, m, valid = heu_integers(theta, phi, offs)
        tie = bool(((100.0 * k == 3.0 * (64.0 + 8.0 * m)) & valid).any())
    return (not tie), float(row.min())


def attention_sum_raw(theta, phi, offsets, mode):
    """The un-normalised similarities v_e (0 at non-edges)."""
    keep = {}
    attention_sum(theta, phi, offsets, mode, keep)
    return keep["v"].detach() * Stencil(offsets, theta.shape[2:]).valid(theta.dtype)


MIN_ROW_SUM = 1e-3        # every node's sum of similarities: 1e4 x the 1e-7 of the heu modes, far from cosine's bare 0


@lru_cache(maxsize=None)
def sum_inputs(cid):
    """(theta, phi, dattn) as split_inputs.  heu: multiples of 1/8 in [-2, 2], so dot and L1 distance are exact and
    u = k / (64 + 8 m) for integers k, m: the 0.03 gate is ambiguous only at an exact tie 100 k = 3 (64 + 8 m); cosine:
    positive multiples of 1/8 (no norm near its clamp, no edge sum near 0).  The seed is the first one from the case's own
    for which there is no tie and every node's similarities sum to MIN_ROW_SUM or more (a node whose edges are all gated has
    a = 0 / 1e-7 and a ds of 1e7 * dattn, which alone would decide the error measures of ds)."""
    c = CASES[cid]
    for seed in range(c.seed, c.seed + 1000, 100):
        g = _gen(seed)
        theta = _dyadic((B, c.F) + GRID, g, 0.125, 2.0, positive=c.mode == SUM_COSINE)
        phi = _dyadic((B, c.F) + GRID, g, 0.125, 2.0, positive=c.mode == SUM_COSINE)
        dattn = _rounded(torch.randn((B, len(OFFSETS[c.offs])) + GRID, generator=g, dtype=torch.float64))
        no_tie, low = sum_input_conditions(c, theta, phi)
        if no_tie and low >= MIN_ROW_SUM:
            return theta, phi, dattn
    raise AssertionError(f"{cid}: no admissible seed")


@lru_cache(maxsize=None)
def agg_inputs(cid):
    """(attn, v, dout): attn random in [0, 1) with exact zeros at non-edges; v, dout standard normal; float32 numbers."""
    c = CASES[cid]
    g = _gen(c.seed)
    offs = OFFSETS[c.offs]
    attn = _rounded(torch.rand((B, len(offs)) + GRID, generator=g, dtype=torch.float64)) * Stencil(offs, GRID).valid()
    v = _rounded(torch.randn((B, c.C) + GRID, generator=g, dtype=torch.float64))
    dout = _rounded(torch.randn((B, c.C) + GRID, generator=g, dtype=torch.float64))
    return attn, v, dout


def inputs(cid):
    c = CASES[cid]
    return split_inputs(cid) if isinstance(c, SplitCase) else sum_inputs(cid) if isinstance(c, SumCase) else agg_inputs(cid)


# ------------------------------------------------------------------------------------------------ evaluation
def _skip_plane(t, plane):
    if plane is None:
        return t
    t = t.clone()
    t[:, plane] = 0.0
    return t


def evaluate(cid, dtype=torch.float64, offsets=None, skip_plane=None):
    """Every output of the case's forward and backward entry points, from the restatement in `dtype` and torch.autograd.
    offsets / skip_plane: the corrupted evaluations of the sensitivity test (another offset table; one feature plane, or
    value channel, left out of every sum)."""
    c = CASES[cid]
    offs = OFFSETS[c.offs] if offsets is None else offsets
    if isinstance(c, AggCase):
        attn, v, dout = (t.detach().clone().to(dtype) for t in agg_inputs(cid))
        attn = attn.requires_grad_(True)
        v, dout = _skip_plane(v, skip_plane).requires_grad_(True), _skip_plane(dout, skip_plane)
        out = aggregate(attn, v, offs)
        out.backward(dout)
        return {"out": out.detach(), "dattn": attn.grad, "dv": v.grad}
    theta, phi, dattn = (t.detach().clone().to(dtype) for t in inputs(cid))
    theta = _skip_plane(theta, skip_plane).requires_grad_(True)
    phi = _skip_plane(phi, skip_plane).requires_grad_(True)
    keep = {}
    if isinstance(c, SumCase):
        attn = attention_sum(theta, phi, offs, c.mode, keep)
        attn.backward(dattn)
        return {"attn": attn.detach(), "ds": keep["v"].grad, "dtheta": theta.grad, "dphi": phi.grad}
    attn = attention_split(theta, phi, offs, c.flags, c.scale, c.F_relu, keep)
    attn.backward(dattn)
    res = {"attn": attn.detach(), "ds": keep["dot_act"].grad, "dtheta": theta.grad, "dphi": phi.grad}
    if is_split(c):
        res["ds2"] = keep["dot_raw"].grad
    return res


def errs(got, ref64):
    """(max-abs over max |ref|, relative L2) of `got` against the float64 reference (tests/test_gpu_oneshot_shapes.py)."""
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape, (tuple(got.shape), tuple(ref64.shape))
    d = got - ref64
    return d.abs().max().item() / ref64.abs().max().item(), d.norm().item() / ref64.norm().item()


@lru_cache(maxsize=None)
def reference(cid):
    """(ref64, e32): the float64 outputs, and per output the error (max, L2) of the float32 evaluation of the same
    restatement on the CPU.  An output whose reference is identically 0 (ds of relu_split0) has e32 None: it is compared
    exactly."""
    ref64, r32 = evaluate(cid, torch.float64), evaluate(cid, torch.float32)
    e32 = {k: (errs(r32[k], v) if float(v.abs().max()) > 0.0 else None) for k, v in ref64.items()}
    return ref64, e32


def tolerance(e32_pair):
    """(max, L2) bound of one output: MARGIN * e32, FLOOR where e32 is exactly 0."""
    return tuple(MARGIN * e if e > 0.0 else FLOOR for e in e32_pair)


def edgeless_nodes(offs_name):
    """[D, H, W] bool: nodes without any in-grid edge."""
    return Stencil(OFFSETS[offs_name], GRID).valid().sum(1)[0] == 0
