"""The OneShot transform and consistency-loss kernels (csrc/resample.hip: permute_flip, resize_nearest, trilinear
align_corners=False forward / backward, affine_sample forward / scatter backward; csrc/loss.hip: sigmoid,
masked smooth-L1) at shapes of many blocks, several plane groups and ragged tails, per element against plain torch
CPU ops -- the calls the reference's classes make (dram/data_transforms.py:1140-1239, dram/metrics.py:434-452).

All of these kernels index a plane as blockIdx.x * 256 + threadIdx.x; the trilinear and affine-sample kernels take
TRI_CPT = 8 planes per blockIdx.y (except trilinear_bwd_general_kernel: one plane per blockIdx.y).  Shapes here are
non-cubic, S is not a multiple of 256 and spans 8 to 100+ blocks, plane counts are 1, 8 and 11 (two plane groups, the
second with a tail of 3), and there is one training-size case per op at 80^3.

Tolerances:
* index transforms, nearest, the all-outside affine case, the structural properties of smooth-L1: bit-exact;
* trilinear and affine sample: no fixed number.  The same torch op is evaluated on the CPU in fp32 as well; e32 is its
  error against the fp64 evaluation (max-abs over max |ref|, and relative L2).  The kernel's error against fp64 must be
  <= 4 * e32: the kernels blend z/y before x, contract to fmaf, compute coordinates in fp32 in their own order and scatter
  with atomics in arbitrary order -- a few roundings more or fewer, where a wrong tap, weight, plane or block is an error
  of 1e-2 to 1.  Where every weight is exactly 0 or 1 (the tiny extent-1 cases: e32 = 0) the 1e-5 of
  tests/test_gpu_transforms.py is the floor, there and only there.  Every case prints its figures before it asserts
  (profiles/oneshot_accuracy.txt is that output of one run);
* sigmoid: derived -- one expf (2 ulp), an add, a reciprocal and up to three multiplies: relative error <= 16 * 2^-24
  per element for p and for dy * p * (1 - p); |x| > 80 (results at or below the fp32 denormal range) absolutely;
* smooth-L1 and the whole loss: 2e-5 * max(1, |ref|) for the loss scalars, 1e-4 max-relative for gradient tensors
  (the numbers of tests/test_gpu_train_step.py)."""
import itertools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import dram_oracle as O

pytestmark = pytest.mark.gpu
FREQ = {k: 1.0 / 6 for k in range(6)}


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _errs(got, ref64):
    """(max-abs over max |ref|, relative L2) of `got` against the fp64 reference."""
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape, (tuple(got.shape), tuple(ref64.shape))
    d = got - ref64
    return d.abs().max().item() / ref64.abs().max().item(), d.norm().item() / ref64.norm().item()


def _check_against_e32(label, what, got, ref64, ref32, floor=0.0):
    """kernel error <= 4 * (torch CPU fp32's own error), in both metrics; prints the row first."""
    k_max, k_l2 = _errs(got, ref64)
    e_max, e_l2 = _errs(ref32, ref64)
    print(f"oneshot-accuracy: {label} {what:4s} HIP max {k_max:.2e} L2 {k_l2:.2e}   torch-CPU-fp32 max {e_max:.2e} L2 {e_l2:.2e}")
    assert math.isfinite(k_max) and math.isfinite(k_l2), (label, what)
    assert k_max <= max(4.0 * e_max, floor), (label, what, "max", k_max, e_max)
    assert k_l2 <= max(4.0 * e_l2, floor), (label, what, "L2", k_l2, e_l2)


# --------------------------------------------------------------------------------------- permute / flip
def test_all_signed_permutations_bit_exact():
    """6 permutations x 8 flip masks on 6 planes of 9 x 20 x 33 (S = 5940: 24 blocks, the last one with 52 voxels):
    forward against permute + flip, backward against the inverse (flip back, inverse permutation), bit for bit."""
    from dram_amd import functional as HF
    x = _rand((2, 3, 9, 20, 33), 1)
    n = 0
    for perm in itertools.permutations(range(3)):
        for flip in itertools.product((0, 1), repeat=3):
            xg = x.cuda().requires_grad_(True)
            y = HF.spatial_permute_flip(xg, perm, flip)
            dims = [2 + k for k in range(3) if flip[k]]
            want = x.permute(0, 1, 2 + perm[0], 2 + perm[1], 2 + perm[2])
            want = torch.flip(want, dims) if dims else want
            assert torch.equal(y.detach().cpu(), want.contiguous()), (perm, flip)
            dy = _rand(tuple(want.shape), 100 + n)
            (y * dy.cuda()).sum().backward()
            inv = [0, 0, 0]
            for k in range(3):
                inv[perm[k]] = k
            back = torch.flip(dy, dims) if dims else dy
            back = back.permute(0, 1, 2 + inv[0], 2 + inv[1], 2 + inv[2]).contiguous()
            assert torch.equal(xg.grad.cpu(), back), (perm, flip)
            n += 1
    assert n == 48


@pytest.mark.parametrize("kind,arg", [("flip", (2,)), ("flip", (4,)), ("flip", (2, 3, 4)), ("flip", (-1, -3)),
                                      ("rot", ((2, 3), 1)), ("rot", ((4, 2), 3)), ("rot", ((3, 4), 2)), ("rot", ((4, 3), 1))])
def test_flip_rot90_classes_at_training_size(kind, arg):
    """Flip3DOneShot / Rotate903DOneShot on 2 planes of 80 x 64 x 48 (960 blocks) against torch.flip / torch.rot90,
    forward and backward, bit for bit."""
    from dram_amd import transforms as T
    x = _rand((1, 2, 80, 64, 48), 2)
    xc = x.clone().requires_grad_(True)
    if kind == "flip":
        t, want = T.Flip3DOneShot(flip_axis=arg), torch.flip(xc, arg)
    else:
        t, want = T.Rotate903DOneShot(rotate_axis=arg[0], rotate_times=arg[1]), torch.rot90(xc, arg[1], arg[0])
    xg = x.cuda().requires_grad_(True)
    y = t({"#image": xg})["#image"]
    assert torch.equal(y.detach().cpu(), want.detach().contiguous()), (kind, arg)
    dy = _rand(tuple(want.shape), 3)
    (want * dy).sum().backward()
    (y * dy.cuda()).sum().backward()
    assert torch.equal(xg.grad.cpu(), xc.grad), (kind, arg)


# --------------------------------------------------------------------------------------- nearest
NEAREST_CASES = [
    # input shape, size, scale_factor
    ((1, 11, 9, 20, 33), (13, 31, 40), None),        # up on every axis, 11 planes
    ((2, 4, 9, 20, 33), (5, 11, 17), None),          # down on every axis
    ((1, 1, 9, 20, 33), (12, 10, 50), None),         # mixed
    ((3, 5, 9, 20, 33), None, (0.7, 1.3, 0.7)),      # factors that are not dyadic: the given factor maps the coordinates
    ((1, 3, 12, 21, 35), None, (1.3, 0.7, 2.0)),
    ((2, 4, 9, 20, 33), None, (0.5, 0.5, 0.5)),
    ((1, 2, 80, 80, 80), (70, 90, 80), None),        # the rescale pool of the consistency loss
]


@pytest.mark.parametrize("shape,size,sf", NEAREST_CASES)
def test_nearest_bit_exact(shape, size, sf):
    from dram_amd import functional as HF
    x = _rand(shape, 4)
    want = F.interpolate(x, size=size, scale_factor=sf, mode="nearest")
    got = HF.interpolate_nearest(x.cuda(), size=size, scale_factor=sf)
    assert torch.equal(got.cpu(), want), (shape, size, sf)


# --------------------------------------------------------------------------------------- trilinear, align_corners=False
# The backward kernel is chosen per call: every axis scale (= in/out, or 1/factor) > 0.5 -> trilinear_bwd_kernel (gather,
# TRI_CPT planes per blockIdx.y); any axis scale <= 0.5 (magnification >= 2) -> trilinear_bwd_general_kernel (one plane per
# blockIdx.y).  The forward kernel (TRI_CPT planes per blockIdx.y) is the same for all.
TRILINEAR_CASES = [
    # label, input shape, size, scale_factor, floor
    # --- trilinear_bwd_kernel (gather)
    ("gather_mixed_p11", (1, 11, 9, 20, 33), (7, 26, 40), None, 0.0),        # scales 1.286, 0.769, 0.825; 11 planes; So = 7280 (29 blocks, ragged)
    ("gather_half_p8", (2, 4, 9, 20, 33), None, (0.5, 0.5, 0.5), 0.0),       # factor 0.5: scales 2, 2, 2; 8 planes; S = 5940 (24 blocks, ragged)
    ("gather_factor_p1", (1, 1, 12, 21, 35), None, (0.7, 1.3, 0.7), 0.0),    # non-integer factors: scales 1.429, 0.769, 1.429; 1 plane
    ("gather_down_p3", (1, 3, 16, 30, 44), (7, 13, 19), None, 0.0),          # pure downscale: scales 2.286, 2.308, 2.316 (inputs no output touches)
    ("gather_p15", (3, 5, 9, 20, 33), (11, 17, 37), None, 0.0),              # scales 0.818, 1.176, 0.892; 15 planes (two groups, tail of 7)
    ("gather_Do1", (2, 2, 5, 20, 33), (1, 15, 30), None, 0.0),               # Do = 1: scales 5, 1.333, 1.1
    ("gather_Do1_tiny", (2, 2, 5, 6, 7), (1, 6, 7), None, 1e-5),             # Do = 1, y and x copied: every weight 0 or 1
    ("gather_80_70x90x80", (1, 2, 80, 80, 80), (70, 90, 80), None, 0.0),     # scales 1.143, 0.889, 1; the loss's rescale pool
    ("gather_80_90x70x80", (3, 1, 80, 80, 80), (90, 70, 80), None, 0.0),     # scales 0.889, 1.143, 1; 3 planes
    # --- trilinear_bwd_general_kernel (one plane per blockIdx.y)
    ("general_p11", (1, 11, 9, 20, 33), (18, 50, 40), None, 0.0),            # scales 0.5, 0.4, 0.825; 11 planes; S = 5940 (24 blocks, ragged)
    ("general_factor_p8", (2, 4, 9, 20, 33), None, (2.0, 1.0, 3.0), 0.0),    # factors: scales 0.5, 1, 0.333; 8 planes
    ("general_p1", (1, 1, 5, 6, 70), (5, 6, 256), None, 0.0),                # scales 1, 1, 0.273; 1 plane
    ("general_D1", (2, 2, 1, 20, 33), (3, 15, 30), None, 0.0),               # D = 1 -> Do = 3: scales 0.333, 1.333, 1.1
    ("general_D1_tiny", (2, 2, 1, 6, 7), (3, 6, 7), None, 1e-5),             # D = 1 -> Do = 3, y and x copied: every weight 0 or 1
]


@pytest.mark.parametrize("label,shape,size,sf,floor", TRILINEAR_CASES, ids=[c[0] for c in TRILINEAR_CASES])
def test_trilinear_fwd_bwd_against_fp64(label, shape, size, sf, floor):
    from dram_amd import functional as HF
    scales = [1.0 / f for f in sf] if sf else [i / o for i, o in zip(shape[2:], size)]
    assert label.startswith("general" if min(scales) <= 0.5 else "gather"), (label, scales)    # the kernel the case is built for
    x = _rand(shape, 5)
    x64 = x.double().requires_grad_(True)
    x32 = x.clone().requires_grad_(True)
    r64 = F.interpolate(x64, size=size, scale_factor=sf, mode="trilinear", align_corners=False)
    r32 = F.interpolate(x32, size=size, scale_factor=sf, mode="trilinear", align_corners=False)
    dy = _rand(tuple(r64.shape), 6)
    (r64 * dy.double()).sum().backward()
    (r32 * dy).sum().backward()
    xg = x.cuda().requires_grad_(True)
    y = HF.interpolate_trilinear(xg, size=size, scale_factor=sf)
    (y * dy.cuda()).sum().backward()
    _check_against_e32(f"trilinear {label}", "fwd", y, r64.detach(), r32.detach(), floor)
    _check_against_e32(f"trilinear {label}", "bwd", xg.grad, x64.grad, x32.grad, floor)


def test_rescale_class_at_training_size():
    """Rescale3DOneShot in size mode, 80^3 -> (70, 90, 80): "#image" trilinear with gradient, "#reference" nearest."""
    from dram_amd import transforms as T
    x, lab = _rand((1, 2, 80, 80, 80), 7), (_rand((1, 1, 80, 80, 80), 8) > 0).float()
    t = T.Rescale3DOneShot(None, (70, 90, 80), mode="size")
    xg = x.cuda().requires_grad_(True)
    res = t({"#image": xg, "#reference": lab.cuda(), "meta": 3})
    assert res["meta"] == 3
    assert torch.equal(res["#reference"].cpu(), F.interpolate(lab, size=(70, 90, 80), mode="nearest"))
    x64, x32 = x.double().requires_grad_(True), x.clone().requires_grad_(True)
    r64 = F.interpolate(x64, size=(70, 90, 80), mode="trilinear", align_corners=False)
    r32 = F.interpolate(x32, size=(70, 90, 80), mode="trilinear", align_corners=False)
    dy = _rand(tuple(r64.shape), 9)
    (r64 * dy.double()).sum().backward()
    (r32 * dy).sum().backward()
    (res["#image"] * dy.cuda()).sum().backward()
    _check_against_e32("rescale-class 80^3->(70,90,80)", "fwd", res["#image"], r64.detach(), r32.detach())
    _check_against_e32("rescale-class 80^3->(70,90,80)", "bwd", xg.grad, x64.grad, x32.grad)


# --------------------------------------------------------------------------------------- affine sample
def _f32(m):
    return [float(np.float32(v)) for v in m]


def _rot_x(theta):
    c, s = math.cos(theta), math.sin(theta)
    return _f32([1, 0, 0, 0, 0, c, -s, 0, 0, s, c, 0])


# anisotropic scale, shear and translation
GENERAL_34 = _f32([0.9, 0.15, -0.1, 0.05, 0.2, 1.2, 0.1, -0.1, -0.05, 0.1, 0.7, 0.08])
AFFINE_CASES = [
    # label, shape, matrix (rotations about x on D != H: the corners leave the volume, some of the 8 taps are out of range)
    ("rotx_0", (1, 11, 9, 20, 33), _rot_x(0.0)),
    ("rotx_0.3", (1, 11, 9, 20, 33), _rot_x(0.3)),
    ("rotx_pi/2", (1, 11, 9, 20, 33), _rot_x(math.pi / 2)),
    ("rotx_2.6", (1, 11, 9, 20, 33), _rot_x(2.6)),
    ("rotx_pi", (1, 11, 9, 20, 33), _rot_x(math.pi)),
    ("general_3x4", (1, 11, 9, 20, 33), GENERAL_34),
    ("general_3x4_p8", (2, 4, 12, 21, 35), GENERAL_34),
    ("rotx_0.7_p1", (1, 1, 12, 21, 35), _rot_x(0.7)),
    ("rotx_0.7_80", (1, 2, 80, 80, 80), _rot_x(0.7)),
]


def _grid_sample(x, m):
    theta = torch.tensor(m, dtype=x.dtype).view(1, 3, 4).repeat(x.shape[0], 1, 1)
    grid = F.affine_grid(theta, list(x.shape), align_corners=False)
    return F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=False)


@pytest.mark.parametrize("label,shape,m", AFFINE_CASES, ids=[c[0] for c in AFFINE_CASES])
def test_affine_sample_fwd_bwd_against_fp64(label, shape, m):
    from dram_amd import functional as HF
    x = _rand(shape, 10)
    x64, x32 = x.double().requires_grad_(True), x.clone().requires_grad_(True)
    r64, r32 = _grid_sample(x64, m), _grid_sample(x32, m)
    dy = _rand(shape, 11)
    (r64 * dy.double()).sum().backward()
    (r32 * dy).sum().backward()
    xg = x.cuda().requires_grad_(True)
    y = HF.affine_sample(xg, m)
    (y * dy.cuda()).sum().backward()
    _check_against_e32(f"affine {label}", "fwd", y, r64.detach(), r32.detach())
    _check_against_e32(f"affine {label}", "bwd", xg.grad, x64.grad, x32.grad)


def test_rotate3dx_class_uses_the_same_matrix():
    """Rotate3DXOneShot (the class) equals HF.affine_sample with its get_rot_mat(), bit for bit in the forward."""
    from dram_amd import functional as HF
    from dram_amd import transforms as T
    x = _rand((1, 3, 9, 20, 33), 12).cuda()
    t = T.Rotate3DXOneShot()
    t.theta = np.array([2.6])
    assert t.get_rot_mat() == _rot_x(2.6)
    assert torch.equal(t({"#image": x})["#image"], HF.affine_sample(x, _rot_x(2.6)))


def test_affine_sample_all_outside_is_exactly_zero():
    """A translation by two volume widths moves every sample point (and all 8 taps) outside: forward and backward are
    exactly zero, as grid_sample's zeros padding gives."""
    from dram_amd import functional as HF
    m = _f32([1, 0, 0, 4.0, 0, 1, 0, 0, 0, 0, 1, 0])
    x = _rand((1, 11, 9, 20, 33), 13)
    assert _grid_sample(x, m).abs().max().item() == 0.0
    xg = x.cuda().requires_grad_(True)
    y = HF.affine_sample(xg, m)
    assert torch.count_nonzero(y).item() == 0
    (y * _rand(tuple(x.shape), 14).cuda()).sum().backward()
    assert torch.count_nonzero(xg.grad).item() == 0


# --------------------------------------------------------------------------------------- sigmoid
def test_sigmoid_grid_stride_and_saturation():
    """n = 5 * 80^3 + 3 > 8192 * 256: the grid-stride loop takes a second trip and ends in a ragged tail.  p and
    dx = dy * p * (1 - p) per element against fp64 at 16 * 2^-24 relative; the planted |x| > 80 absolutely."""
    from dram_amd import functional as HF
    n = 5 * 80 ** 3 + 3
    assert n > 8192 * 256
    g = torch.Generator().manual_seed(15)
    x = torch.randn(n, generator=g) * 6.0
    planted = [s * v for v in (math.inf, 100.0, 88.0, 80.0, 50.0, 20.0, 1e-8, 0.0) for s in (1.0, -1.0)]
    where = torch.randperm(n, generator=g)[:4 * len(planted)]
    where[0], where[1], where[2] = 0, n - 1, 8192 * 256        # first element, ragged tail, first element of the second trip
    x[where] = torch.tensor(planted * 4)
    dy = (0.5 + torch.rand(n, generator=g)) * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    xg = x.view(1, 1, 1, 1, n).cuda().requires_grad_(True)
    p = HF.sigmoid(xg)
    (p * dy.view_as(xg).cuda()).sum().backward()
    p, dx = p.detach().cpu().view(-1).double(), xg.grad.cpu().view(-1).double()
    x64 = x.double()
    p64, q64 = torch.sigmoid(x64), torch.sigmoid(-x64)          # 1 - p without cancellation
    dx64 = dy.double() * p64 * q64
    far = x.abs() > 80.0
    assert 0 < far.sum().item() <= n // 100
    tol = 16.0 * 2.0 ** -24
    near = ~far
    rel_p = ((p[near] - p64[near]).abs() / p64[near]).max().item()
    rel_dx = ((dx[near] - dx64[near]).abs() / dx64[near].abs()).max().item()
    print(f"oneshot-accuracy: sigmoid n={n} |x|<=80: max rel err p {rel_p:.2e} dx {rel_dx:.2e} (bound {tol:.2e})")
    assert rel_p <= tol, rel_p
    assert rel_dx <= tol, rel_dx
    assert (p[far] - p64[far]).abs().max().item() <= 1e-37
    assert (dx[far] - dx64[far]).abs().max().item() <= 1e-37
    assert (x == math.inf).sum().item() >= 1 and (x == -math.inf).sum().item() >= 1
    assert (p[x == math.inf] == 1.0).all().item() and torch.count_nonzero(p[x == -math.inf]).item() == 0
    assert torch.count_nonzero(dx[x.abs() == math.inf]).item() == 0


# --------------------------------------------------------------------------------------- masked smooth-L1
def _smooth_l1_inputs():
    N, C, dims = 3, 2, (1, 151, 163)
    S = dims[0] * dims[1] * dims[2]
    assert S == 3 * 8192 + 37                                   # four chunks of LCHUNK = 8192 per row, the last with 37 elements
    g = torch.Generator().manual_seed(16)
    a = torch.randn((N, C) + dims, generator=g) * 1.2           # |a - b| straddles 1
    b = torch.randn((N, C) + dims, generator=g) * 1.2
    af, bf = a.view(N, C, S), b.view(N, C, S)
    for k, d in enumerate((0.0, 1.0, -1.0)):                    # exact 0, +1 and -1, in the first, a middle and the last chunk
        for e in (5 + k, 8192 + 17 + k, S - 1 - k):
            bf[:, :, e] = 0.25
            af[:, :, e] = 0.25 + d
    r = torch.rand((N, 1) + dims, generator=g)
    mask = torch.where(r < 0.4, 0.5, torch.where(r < 0.6, -1.0, torch.where(r < 0.8, 1.0, 0.0)))
    mask[2] = torch.where(r[2] < 0.5, -1.0, 0.0)                # one sample with nothing selected
    mf = mask.view(N, S)
    for k in range(3):
        for e in (5 + k, 8192 + 17 + k, S - 1 - k):
            mf[:2, e] = 0.5
    return a, b, mask


def test_masked_smooth_l1_chunks_and_gradients():
    from dram_amd import functional as HF
    a, b, mask = _smooth_l1_inputs()
    gup = 0.37
    sel = mask.expand_as(a) > 0
    a64, b64 = a.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = F.smooth_l1_loss(a64[sel], b64[sel])
    (ref * gup).backward()
    ag, bg, mg = a.cuda().requires_grad_(True), b.cuda().requires_grad_(True), mask.cuda()
    loss = HF.masked_smooth_l1(ag, bg, mg)
    out = loss.grad_fn.saved_tensors[3].clone()                  # {mean, selected count}
    assert out.numel() == 2 and out[0].item() == loss.item()
    (loss * gup).backward()
    print(f"oneshot-accuracy: masked-smooth-L1 loss {loss.item():.8f} fp64 {ref.item():.8f} count {out[1].item():.0f}")
    assert abs(loss.item() - ref.item()) <= 2e-5 * max(1.0, abs(ref.item()))
    assert out[1].item() == float(sel.sum().item())
    da, db = ag.grad.cpu(), bg.grad.cpu()
    for got, want in ((da, a64.grad), (db, b64.grad)):
        err = (got.double() - want).abs().max().item() / want.abs().max().item()
        assert err <= 1e-4, err
    assert torch.count_nonzero(da[~sel]).item() == 0 and torch.count_nonzero(db[~sel]).item() == 0
    assert torch.count_nonzero(da[2]).item() == 0               # the sample whose mask is <= 0 everywhere
    assert torch.equal(db.view(torch.int32), (-da).view(torch.int32))
    # repeat-run determinism of the forward
    again = HF.masked_smooth_l1(ag.detach(), bg.detach(), mg)
    assert again.item() == loss.item()
    # one operand without gradient: the da-only and db-only calls
    a1 = a.cuda().requires_grad_(True)
    (HF.masked_smooth_l1(a1, b.cuda(), mg) * gup).backward()
    assert torch.equal(a1.grad.cpu().view(torch.int32), da.view(torch.int32))
    b1 = b.cuda().requires_grad_(True)
    (HF.masked_smooth_l1(a.cuda(), b1, mg) * gup).backward()
    assert torch.equal(b1.grad.cpu().view(torch.int32), db.view(torch.int32))


def test_masked_smooth_l1_empty_selection_is_nan():
    from dram_amd import functional as HF
    a, b, mask = _smooth_l1_inputs()
    mask = -mask.abs()
    sel = mask.expand_as(a) > 0
    assert sel.sum().item() == 0 and torch.isnan(F.smooth_l1_loss(a[sel], b[sel]))
    assert torch.isnan(HF.masked_smooth_l1(a.cuda(), b.cuda(), mask.cuda())).item()


# --------------------------------------------------------------------------------------- the whole consistency loss
def _standin(theta, kept):
    """The closed-form 3-output stand-in of the affloss golden (oracle/make_golden.py:gen_affloss; test scaffolding in
    torch ops), keeping the gradient of everything it returns, in each of its calls."""
    def model(imgs, lbs):
        a, b, c = theta[0], theta[1], theta[2]
        D, H, W = imgs.shape[-3:]
        rz = torch.linspace(0.0, 1.0, D, dtype=imgs.dtype, device=imgs.device).view(1, 1, D, 1, 1)
        rx = torch.linspace(0.0, 1.0, W, dtype=imgs.dtype, device=imgs.device).view(1, 1, 1, 1, W)
        dense = a * (imgs - 0.5) * 4.0 + b + 0.6 * c * rx - 0.4 * rz
        refined = 0.7 * dense - c * imgs
        cls = torch.cat([a * imgs + rz, imgs * imgs + b * c * rx], dim=1)
        for t in (dense, refined, cls):
            t.retain_grad()
            kept.append(t)
        return dense, refined, cls
    return model


CHAINS = {
    # rescale down (scales 1.429, 1.333, 1.4: gather backward), flip, a quarter turn that changes the shape
    "rescale_flip_rot": [("rescale", (14, 18, 20)), ("flip", (2, 4)), ("rot90", 1, (2, 3))],
    # quarter turn to (20, 28, 24), then z magnified 2x (scales 0.5, 1.167, 0.923: trilinear_bwd_general_kernel); S = 24960
    "rot_rescale_up": [("rot90", 3, (3, 4)), ("rescale", (40, 24, 26))],
    "flip": [("flip", (2, 3, 4))],
    "none": [],
}


@pytest.mark.parametrize("name", list(CHAINS))
def test_consistency_loss_per_element_gradients(name):
    """DeviceIntRegAffRefineLoss with a fixed transform chain against O.int_reg_aff_refine_loss in fp64: N = 3,
    volume 20 x 24 x 28 (S = 13440: two chunks of the loss kernels, the second ragged), ctss = 0 in the first sample.
    Compared: the three loss values and the gradient of all six tensors the model returned in its two calls."""
    from dram_amd import transforms as T
    from dram_amd.train_step import Batch, DeviceIntRegAffRefineLoss
    chain = CHAINS[name]
    N, D, H, W = 3, 20, 24, 28
    g = torch.Generator().manual_seed(17)
    zz = ((torch.arange(D) - (D - 1) / 2) / (0.45 * D)).view(D, 1, 1)
    yy = ((torch.arange(H) - (H - 1) / 2) / (0.45 * H)).view(1, H, 1)
    xx = ((torch.arange(W) - (W - 1) / 2) / (0.45 * W)).view(1, 1, W)
    lobes = ((zz ** 2 + yy ** 2 + xx ** 2) < 1.0).float().view(1, 1, D, H, W).repeat(N, 1, 1, 1, 1)
    images = torch.rand((N, 1, D, H, W), generator=g) * lobes
    lesions = ((images > 0.7) & (lobes > 0)).float()
    ctss = [0.0, 2.0, 4.0]
    theta0 = torch.tensor([1.5, -0.4, 0.8])
    w = (2.0, 0.5, 1.0)
    # oracle, fp64
    kept_r = []
    ref = O.int_reg_aff_refine_loss(_standin(theta0.double().requires_grad_(True), kept_r), chain, images.double(), lobes.double(), lesions.double(),
                                    ctss, FREQ, band_width=5e-2, smoothing=0.05)
    (w[0] * ref[0] + w[1] * ref[1] + w[2] * ref[2]).backward()
    # device
    objs = []
    for op in chain:
        if op[0] == "rescale":
            objs.append(T.Rescale3DOneShot(None, op[1], mode="size"))
        elif op[0] == "flip":
            objs.append(T.Flip3DOneShot(flip_axis=op[1]))
        else:
            objs.append(T.Rotate903DOneShot(rotate_axis=op[2], rotate_times=op[1]))

    def fixed_transform():
        def apply(sample):
            for t in objs:
                sample = t(sample)
            return sample
        apply.p = objs
        return apply
    loss = DeviceIntRegAffRefineLoss(rescale_jitter=[8, 10, 12, 14], band_width=5e-2, smoothing=0.05, freq_map=FREQ)
    loss.get_affine_transform = fixed_transform
    kept = []
    batch = Batch(images.cuda(), lobes.cuda(), lesions.cuda(), ctss, FREQ, band_width=5e-2)
    got = loss(_standin(theta0.cuda().requires_grad_(True), kept), batch)
    (w[0] * got[0] + w[1] * got[1] + w[2] * got[2]).backward()
    for nm, g_, r_ in zip(("reg", "aff", "seg"), got, ref):
        print(f"oneshot-accuracy: consistency-loss {name} {nm} {g_.item():.8f} fp64 {r_.item():.8f}")
        assert abs(g_.item() - r_.item()) <= 2e-5 * max(1.0, abs(r_.item())), (name, nm, g_.item(), r_.item())
    assert len(kept) == len(kept_r) == 6
    names = ("dense", "refined", "cls", "aff_dense", "aff_refined", "aff_cls")
    for nm, t, r in zip(names, kept, kept_r):
        assert tuple(t.shape) == tuple(r.shape), (name, nm)
        assert t.grad is not None and r.grad is not None, (name, nm)
        rmax = r.grad.abs().max().item()
        if rmax == 0.0:     # (the empty chain compares cls with itself: no gradient at all)
            assert torch.count_nonzero(t.grad).item() == 0, (name, nm)
            continue
        err = (t.grad.cpu().double() - r.grad).abs().max().item() / rmax
        print(f"oneshot-accuracy: consistency-loss {name} grad {nm} max-rel err {err:.2e}")
        assert err <= 1e-4, (name, nm, err)
