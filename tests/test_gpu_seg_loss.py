"""GPU tests of the device BootBinCrossEntropy and BinaryCrossEntropySmooth (dram_amd/losses.py, functional.boot_bce /
bce_smooth; kernels dram_boot_bce_* / dram_bce_smooth_* of csrc/loss.hip) against the fp64 restatement that
tests/test_seg_loss_cpu.py pins to torch, to the oracle and to the reference's own classes.

Bounds.  Values and gradients are held to what tests/test_gpu_intreg_loss.py holds the fused losses to: a loss within
2e-5 max(1, |ref|), a gradient within 1e-4 of its largest element.  (The arithmetic would allow less: a logf of a few
2^-24 relative and fp64 sums put the loss within about 1e-6, a gradient element within about ten fp32 roundings; the
project's figure is kept so that one number covers every loss of the tree.)  torch's own fp32 evaluation on the CPU is
asserted to meet the same bounds, so they are not fitted to the kernels.  Where an input sits ON a clamp bound the
yardstick is torch's fp32 evaluation (an fp64 evaluation puts 1 - p on the other side of the bound), element for element
within 2e-6: about sixteen fp32 roundings lie between the two evaluations, 16 x 2^-24 = 1e-6, and the two terms of an
inside element cancel by at most a quarter at the inputs used.

Every shape is the smallest that reaches the path it is there for; the whole file takes a few seconds."""
import numpy as np
import pytest
import torch

import seg_loss_restatement as R
from oracle import dram_oracle as O
from seg_loss_restatement import torch_bce_smooth

pytestmark = pytest.mark.gpu
VAL_TOL, GRAD_TOL, EDGE_TOL = 2e-5, 1e-4, 2e-6


def _hf():
    from dram_amd import functional as HF
    return HF


def _chunk():
    from dram_amd import _lib
    return _lib.lib.dram_seg_loss_chunk()


def _boot(p, t, voi, s=0.1, g=None):
    """(loss tensor, gradient tensor) of the device loss; inputs on the device."""
    p = p.detach().requires_grad_(True)
    loss = _hf().boot_bce(p, t, voi, s)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    (loss if g is None else loss * g).backward()
    return loss.detach(), p.grad


def _smooth(p, t, s=1.0, g=None):
    p = p.detach().requires_grad_(True)
    loss = _hf().bce_smooth(p, t, s)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    (loss if g is None else loss * g).backward()
    return loss.detach(), p.grad


def _cpu_autograd(fn, p, *rest):
    p = p.detach().clone().requires_grad_(True)
    loss = fn(p, *rest)
    loss.backward()
    return loss.detach(), p.grad


def _exact_case(n, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.tensor([0.25, 0.5, 0.75])[torch.randint(0, 3, (n,), generator=g)]
    voi = (torch.rand(n, generator=g) < 0.6).float()
    t = ((torch.rand(n, generator=g) < 0.4) & (voi > 0)).float()
    return p, t, voi


def _random_case(shape, seed, voi_share=0.6, t_share=0.4, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    p = torch.sigmoid(torch.randn(shape, generator=g) * scale)
    voi = (torch.rand(shape, generator=g) < voi_share).float()
    t = ((torch.rand(shape, generator=g) < t_share) & (voi > 0)).float()
    return p, t, voi


def _same(a, b):
    """The same bits (a nan equals itself here)."""
    return a.shape == b.shape and torch.equal(a.reshape(-1).view(torch.int32), b.reshape(-1).view(torch.int32))


def _close(got, ref):
    return abs(got - ref) <= VAL_TOL * max(1.0, abs(ref))


def _structural_sizes():
    c = 4096          # dram_seg_loss_chunk(), asserted in the test; 256 partials are one sweep of the finish block
    return [c - 1, c, c + 1, 3 * c + 77, 1, 256 * c + 1]


@pytest.mark.parametrize("n", _structural_sizes())
def test_structural_sizes_exact_counts_and_same_bits(n):
    """Block boundaries, one element, and one partial more than the finish block takes in one sweep, on inputs whose counts
    and sum of t are exact: the fp64 totals must be THE integers, and two runs the same bits."""
    HF = _hf()
    assert _chunk() == 4096
    p, t, voi = _exact_case(n, seed=n % 97)
    if n == 1:
        voi[0], t[0] = 1.0, 1.0
    pg, tg, vg = p.cuda(), t.cuda(), voi.cuda()
    tot = HF.boot_bce_totals(pg, tg, vg).cpu().numpy()
    assert tot[0] == float((voi < 1e-7).sum()) and tot[2] == float((voi > 0).sum()) and tot[3] == float(t.sum())
    ref = R.boot_bce_sums(p, t, voi)
    assert np.allclose(tot, ref, rtol=1e-6, atol=0)
    tot_s = HF.bce_smooth_totals(pg, tg).cpu().numpy()
    assert tot_s[0] == float(t.sum()) and np.allclose(tot_s, R.bce_smooth_sums(p, t), rtol=1e-6, atol=0)
    l1, g1 = _boot(pg, tg, vg)
    l2, g2 = _boot(pg, tg, vg)
    assert _same(l1, l2) and _same(g1, g2)
    assert torch.equal(HF.boot_bce_totals(pg, tg, vg).cpu(), torch.from_numpy(tot))
    s1, h1 = _smooth(pg, tg, 0.5)
    s2, h2 = _smooth(pg, tg, 0.5)
    assert _same(s1, s2) and _same(h1, h2)
    want = R.boot_bce(p, t, voi, 0.1)
    print(n, "boot", l1.item(), want, "smooth", s1.item(), R.bce_smooth(p, t, 0.5))
    assert (np.isnan(want) and np.isnan(l1.item())) or _close(l1.item(), want)
    assert _close(s1.item(), R.bce_smooth(p, t, 0.5))
    gref = R.boot_bce_grad(p, t, voi, 0.1)
    assert np.abs(g1.cpu().numpy() - gref).max() <= GRAD_TOL * np.abs(gref).max()
    href = R.bce_smooth_grad(p, t, 0.5)
    assert np.abs(h1.cpu().numpy() - href).max() <= GRAD_TOL * np.abs(href).max()


# odd sizes on two and four blocks, a 5-d batch, one row of 7; then rare and common targets (both alpha clamps are in the
# edge tests; here alpha is inside and at each bound with random p)
VALUE_CASES = [((2, 1, 9, 17, 23), 0.6, 0.4, 0.1), ((1, 1, 13, 32, 32), 0.5, 0.03, 0.3), ((7,), 0.5, 0.5, 0.1),
               ((3, 1, 11, 19, 21), 0.7, 0.96, 0.0), ((5000,), 0.4, 0.5, 1.0)]


@pytest.mark.parametrize("shape,voi_share,t_share,s", VALUE_CASES)
def test_boot_bce_matches_fp64_restatement(shape, voi_share, t_share, s):
    p, t, voi = _random_case(shape, seed=len(shape) + shape[-1], voi_share=voi_share, t_share=t_share)
    voi.view(-1)[0], voi.view(-1)[-1], t.view(-1)[-1] = 1.0, 0.0, 0.0       # an inside and an outside at any size
    ref, gref = R.boot_bce(p, t, voi, s), R.boot_bce_grad(p, t, voi, s)
    loss, grad = _boot(p.cuda(), t.cuda(), voi.cuda(), s)
    err = np.abs(grad.cpu().numpy() - gref).max() / np.abs(gref).max()
    l32, g32 = _cpu_autograd(lambda q: O.boot_bce(q, t, voi, s), p)
    err32 = np.abs(g32.numpy() - gref).max() / np.abs(gref).max()
    print(shape, "loss", loss.item(), ref, "torch fp32", l32.item(), "grad rel err", err, "torch fp32", err32)
    assert grad.shape == p.shape
    assert _close(loss.item(), ref) and err <= GRAD_TOL
    assert _close(l32.item(), ref) and err32 <= GRAD_TOL          # the bound is one torch's own fp32 meets


@pytest.mark.parametrize("shape,voi_share,t_share,s", VALUE_CASES)
def test_bce_smooth_matches_fp64_restatement(shape, voi_share, t_share, s):
    smooth = 0.5 + s
    p, t, _ = _random_case(shape, seed=3 + shape[-1], voi_share=1.0, t_share=t_share)
    ref, gref = R.bce_smooth(p, t, smooth), R.bce_smooth_grad(p, t, smooth)
    loss, grad = _smooth(p.cuda(), t.cuda(), smooth)
    err = np.abs(grad.cpu().numpy() - gref).max() / np.abs(gref).max()
    l32, g32 = _cpu_autograd(lambda q: torch_bce_smooth(q, t, smooth), p)
    err32 = np.abs(g32.numpy() - gref).max() / np.abs(gref).max()
    print(shape, "loss", loss.item(), ref, "torch fp32", l32.item(), "grad rel err", err, "torch fp32", err32)
    assert grad.shape == p.shape
    assert _close(loss.item(), ref) and err <= GRAD_TOL
    assert _close(l32.item(), ref) and err32 <= GRAD_TOL


@pytest.mark.parametrize("case", ["mixed", "rare", "common", "noinside"])
def test_reference_golden_fp32(golden_dir, case):
    """The reference's own classes run in fp32 on the CPU (tests/golden/segloss.npz), elements beyond both clamps included:
    there the reference forms 1 - p in fp32, as the kernels do, and the values must still agree."""
    import os
    from dram_amd import BinaryCrossEntropySmooth, BootBinCrossEntropy
    z = np.load(os.path.join(golden_dir, "segloss.npz"))
    dev = lambda k: torch.from_numpy(z[f"{case}/{k}"]).float().cuda()
    p = dev("p").requires_grad_(True)
    loss = BootBinCrossEntropy(float(z[f"{case}/smoothing"]))(p, dev("t"), dev("voi"), class_weights=[1.0, 2.0])
    loss.backward()
    ref, gref = float(z[f"{case}/boot32"]), z[f"{case}/gboot32"]
    assert _close(loss.item(), ref)
    assert np.abs(p.grad.cpu().numpy() - gref).max() <= GRAD_TOL * np.abs(gref).max()
    assert ((p.grad.cpu().numpy() == 0) == (gref == 0)).all()
    q = dev("p").requires_grad_(True)
    loss = BinaryCrossEntropySmooth(float(z[f"{case}/smooth"]))(q, dev("t"))
    loss.backward()
    ref, gref = float(z[f"{case}/bce32"]), z[f"{case}/gbce32"]
    assert _close(loss.item(), ref)
    assert np.abs(q.grad.cpu().numpy() - gref).max() <= GRAD_TOL * np.abs(gref).max()
    assert ((q.grad.cpu().numpy() == 0) == (gref == 0)).all()


def test_voi_all_zero_is_the_outside_term_alone():
    p, t, _ = _random_case((4099,), seed=21)
    t.zero_()
    voi = torch.zeros_like(p)
    loss, grad = _boot(p.cuda(), t.cuda(), voi.cuda(), 0.1)
    ref = float(np.mean(-np.log(np.clip(1.0 - p.double().numpy(), 1e-7, 1 - 1e-7))))
    assert _close(loss.item(), ref) and _close(R.boot_bce(p, t, voi, 0.1), ref)
    gref = R.boot_bce_grad(p, t, voi, 0.1)
    assert np.abs(grad.cpu().numpy() - gref).max() <= GRAD_TOL * np.abs(gref).max()


def test_voi_all_one_is_nan_with_torchs_gradient():
    p, t, _ = _random_case((4099,), seed=22)
    voi = torch.ones_like(p)
    t = (torch.rand(p.shape, generator=torch.Generator().manual_seed(1)) < 0.4).float()
    loss, grad = _boot(p.cuda(), t.cuda(), voi.cuda(), 0.1)
    l32, g32 = _cpu_autograd(lambda q: O.boot_bce(q, t, voi, 0.1), p)
    assert torch.isnan(l32) and torch.isnan(loss)
    assert torch.isfinite(g32).all() and torch.isfinite(grad).all()
    got, ref = grad.cpu(), g32
    assert ((got - ref).abs() <= EDGE_TOL * ref.abs()).all(), ((got - ref).abs() / ref.abs()).max()


@pytest.mark.parametrize("kind", ["none", "all"])
def test_both_alpha_clamps(kind):
    p, _, voi = _random_case((4099,), seed=23)
    t = torch.zeros_like(p) if kind == "none" else voi.clone()
    ref, gref = R.boot_bce(p, t, voi, 0.1), R.boot_bce_grad(p, t, voi, 0.1)
    assert R.boot_bce_from_sums(R.boot_bce_sums(p, t, voi), 0.1)[1] == (0.75 if kind == "none" else 0.25)
    loss, grad = _boot(p.cuda(), t.cuda(), voi.cuda(), 0.1)
    assert _close(loss.item(), ref) and np.abs(grad.cpu().numpy() - gref).max() <= GRAD_TOL * np.abs(gref).max()
    ts = torch.zeros_like(p) if kind == "none" else torch.ones_like(p)
    ref, gref = R.bce_smooth(p, ts, 1.0), R.bce_smooth_grad(p, ts, 1.0)
    assert R.bce_smooth_from_sums(R.bce_smooth_sums(p, ts), p.numel(), 1.0)[1] == (0.7 if kind == "none" else 0.3)
    loss, grad = _smooth(p.cuda(), ts.cuda(), 1.0)
    assert _close(loss.item(), ref) and np.abs(grad.cpu().numpy() - gref).max() <= GRAD_TOL * np.abs(gref).max()


def test_clamp_gradient_rule_at_the_bounds():
    """p at 0, 1, 0.5, eps, 1 - eps and the neighbouring floats, each with t in {0, 1}, inside and outside (the formula is
    defined for t = 1 outside too): the gradient
    passes where eps <= x <= 1 - eps, bounds included, and is exactly 0 elsewhere -- the pattern and the values of torch's
    fp32 autograd."""
    f = np.float32
    eps, hi = f(1e-7), f(1.0) - f(1e-7)
    pts = np.array([0.0, 1.0, 0.5, eps, hi, np.nextafter(eps, f(0)), np.nextafter(hi, f(1)), np.nextafter(eps, f(1)),
                    np.nextafter(hi, f(0)), 0.3, 0.9], dtype=np.float32)
    p = torch.from_numpy(np.tile(pts, 4))
    k = len(pts)
    t = torch.cat([torch.zeros(k), torch.ones(k), torch.zeros(k), torch.ones(k)])
    voi = torch.cat([torch.zeros(2 * k), torch.ones(2 * k)])
    loss, grad = _boot(p.cuda(), t.cuda(), voi.cuda(), 0.1)
    l32, g32 = _cpu_autograd(lambda q: O.boot_bce(q, t, voi, 0.1), p)
    got = grad.cpu()
    print("boot", loss.item(), l32.item(), "zeros", int((g32 == 0).sum()), "of", g32.numel())
    assert (g32 == 0).any() and (g32 != 0).any()
    assert ((got == 0) == (g32 == 0)).all(), (got, g32)
    assert ((got - g32).abs() <= EDGE_TOL * g32.abs()).all(), ((got - g32).abs() / g32.abs().clamp_min(1e-30)).max()
    assert abs(loss.item() - l32.item()) <= VAL_TOL * max(1.0, abs(l32.item()))
    # BinaryCrossEntropySmooth: its own bounds, 1e-6 and 1 - 1e-6
    lo, hs = f(1e-6), f(1.0) - f(1e-6)
    pts = np.array([0.0, 1.0, 0.5, lo, hs, np.nextafter(lo, f(0)), np.nextafter(hs, f(1)), np.nextafter(lo, f(1)),
                    np.nextafter(hs, f(0)), 0.3, 0.9], dtype=np.float32)
    p = torch.from_numpy(np.tile(pts, 2))
    t = torch.cat([torch.zeros(k), torch.ones(k)])
    loss, grad = _smooth(p.cuda(), t.cuda(), 1.0)
    l32, g32 = _cpu_autograd(lambda q: torch_bce_smooth(q, t, 1.0), p)
    got = grad.cpu()
    assert (g32 == 0).any() and (g32 != 0).any()
    assert ((got == 0) == (g32 == 0)).all(), (got, g32)
    assert ((got - g32).abs() <= EDGE_TOL * g32.abs()).all(), ((got - g32).abs() / g32.abs().clamp_min(1e-30)).max()
    assert abs(loss.item() - l32.item()) <= VAL_TOL * max(1.0, abs(l32.item()))


def test_uint8_bool_and_fp32_masks_give_the_same_bits():
    p, t, voi = _random_case((3 * 4096 + 77,), seed=24)
    pg = p.cuda()
    base = _boot(pg, t.cuda(), voi.cuda(), 0.1)
    for tt, vv in ((t.to(torch.uint8), voi.to(torch.uint8)), (t, voi.to(torch.uint8)), (t.to(torch.uint8), voi),
                   (t.bool(), voi.bool())):
        other = _boot(pg, tt.cuda(), vv.cuda(), 0.1)
        assert _same(base[0], other[0]) and _same(base[1], other[1])
    base = _smooth(pg, t.cuda(), 0.7)
    for tt in (t.to(torch.uint8), t.bool()):
        other = _smooth(pg, tt.cuda(), 0.7)
        assert _same(base[0], other[0]) and _same(base[1], other[1])


@pytest.mark.parametrize("n", [4096 + 5, 7])
def test_unaligned_views_give_the_same_bits(n):
    """Every tensor in turn, and all of them, offset by one element from an aligned base (4 bytes, or 1 for uint8)."""
    p, t, voi = _random_case((n,), seed=25)
    t8, v8 = t.to(torch.uint8), voi.to(torch.uint8)

    def off(x):
        buf = torch.empty(n + 1, dtype=x.dtype, device="cuda")
        buf[1:].copy_(x)
        view = buf[1:]
        assert view.data_ptr() % 16 != 0 and view.is_contiguous()
        return view
    base = _boot(p.cuda(), t.cuda(), voi.cuda(), 0.1)
    base_s = _smooth(p.cuda(), t.cuda(), 0.7)
    for args in ((off(p), t.cuda(), voi.cuda()), (p.cuda(), off(t), voi.cuda()), (p.cuda(), t.cuda(), off(voi)),
                 (off(p), off(t), off(voi)), (off(p), off(t8), off(v8)), (p.cuda(), off(t8), v8.cuda())):
        other = _boot(*args, 0.1)
        assert _same(base[0], other[0]) and _same(base[1], other[1])
    for args in ((off(p), t.cuda()), (p.cuda(), off(t)), (off(p), off(t8))):
        other = _smooth(*args, 0.7)
        assert _same(base_s[0], other[0]) and _same(base_s[1], other[1])


def test_upstream_gradient_scales_exactly():
    p, t, voi = _random_case((4096 + 5,), seed=26)
    pg, tg, vg = p.cuda(), t.cuda(), voi.cuda()
    for g in (3.0, -0.37):
        one, scaled = _boot(pg, tg, vg, 0.1), _boot(pg, tg, vg, 0.1, g=g)
        assert torch.equal(scaled[1], one[1] * torch.tensor(g, dtype=torch.float32).cuda())
        one, scaled = _smooth(pg, tg, 0.7), _smooth(pg, tg, 0.7, g=g)
        assert torch.equal(scaled[1], one[1] * torch.tensor(g, dtype=torch.float32).cuda())


def test_consistent_with_the_fused_refine_loss_and_through_sigmoid():
    """boot_bce(sigmoid(dense), pseudo, lobes > 0) is the `seg` term of the fused IntRegRefineLoss when the pseudo-label is
    built as oracle.int_reg_refine_loss builds it; and the gradient through HF.sigmoid is torch autograd's of the oracle."""
    HF = _hf()
    n, shape, s = 3, (9, 17, 23), 0.1
    g = torch.Generator().manual_seed(27)
    dense = torch.randn((n, 1) + shape, generator=g) * 2.0
    lobes = (torch.rand((n, 1) + shape, generator=g) > 0.4).float()
    lobes.view(n, -1)[:, 0], lobes.view(n, -1)[:, -1] = 1.0, 0.0
    lesions = ((torch.rand((n, 1) + shape, generator=g) > 0.5) & (lobes > 0)).float()
    keep = torch.tensor([1.0, 0.0, 1.0])
    targets = torch.tensor([[0.0, 0.1], [0.2, 0.3], [0.4, 0.9]])
    weight = torch.tensor([0.3, 0.25, 0.2])
    dg = dense.cuda().requires_grad_(True)
    probs = HF.sigmoid(dg)
    with torch.no_grad():
        pd = probs.detach().clone()
        pd[lobes.cuda() == 0] = 0.0
        pseudo = ((pd > 0.5) & (lesions.cuda() > 0)).float() * keep.cuda().view(-1, 1, 1, 1, 1)
    loss = HF.boot_bce(probs, pseudo, lobes.cuda() > 0, s)
    loss.backward()
    fused = HF.intreg_refine_loss(dense.cuda(), lobes.cuda(), lesions.cuda(), keep.cuda(), targets.cuda(), weight.cuda(), s)
    print("seg", loss.item(), "fused", fused[1].item())
    assert _close(loss.item(), fused[1].item())
    d64 = dense.double().requires_grad_(True)
    ref = O.boot_bce(torch.sigmoid(d64), pseudo.cpu().double(), lobes > 0, s)
    ref.backward()
    assert _close(loss.item(), ref.item())
    gref = d64.grad.numpy()
    assert np.abs(dg.grad.cpu().numpy() - gref).max() <= GRAD_TOL * np.abs(gref).max()


def test_interface():
    import dram_amd
    from dram_amd import BinaryCrossEntropySmooth, BootBinCrossEntropy, _lib
    assert BootBinCrossEntropy is dram_amd.losses.BootBinCrossEntropy
    p, t, voi = (x.cuda() for x in _random_case((2, 1, 4, 5, 6), seed=28))
    boot, bce = BootBinCrossEntropy(), BinaryCrossEntropySmooth(1.0)
    assert boot.smoothing == 0.1 and torch.equal(boot(p, t, voi), boot(p, t, voi, class_weights=(1.0, 3.0)))
    assert torch.isfinite(bce(p, t))
    for bad in ((p.cpu(), t, voi), (p, t.cpu(), voi), (p, t, voi.cpu())):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            boot(*bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bce(p, t.cpu())
    with pytest.raises(ValueError):
        boot(p, t[:1], voi)
    with pytest.raises(ValueError):
        boot(p, t, voi.view(-1))
    with pytest.raises(ValueError):
        bce(p, t[:, :, :2])
    with pytest.raises(TypeError):
        boot(p.double(), t, voi)
    with pytest.raises(TypeError):
        boot(p, t.to(torch.int16), voi)
    out = torch.zeros(1, device="cuda")
    state = torch.zeros(8, device="cuda")
    ws = torch.zeros(64, dtype=torch.float64, device="cuda")
    a = (p.data_ptr(), t.data_ptr(), voi.data_ptr())
    lib = _lib.lib
    assert lib.dram_boot_bce_fwd(None, a[1], a[2], 2, 2, p.numel(), 0.1, out.data_ptr(), state.data_ptr(), ws.data_ptr(),
                                 ws.numel() * 8, None) == -1
    assert lib.dram_boot_bce_bwd(a[0], a[1], a[2], 2, 2, p.numel(), 0.1, state.data_ptr(), out.data_ptr(), None, None) == -1
    assert lib.dram_bce_smooth_fwd(a[0], None, 2, p.numel(), 1.0, out.data_ptr(), state.data_ptr(), ws.data_ptr(),
                                   ws.numel() * 8, None) == -1
    assert lib.dram_bce_smooth_bwd(a[0], a[1], 2, p.numel(), 1.0, None, out.data_ptr(), out.data_ptr(), None) == -1
    assert lib.dram_boot_bce_fwd(a[0], a[1], a[2], 2, 2, -1, 0.1, out.data_ptr(), state.data_ptr(), ws.data_ptr(),
                                 ws.numel() * 8, None) == -1
    torch.cuda.synchronize()
    assert out.item() == 0.0 and not state.any() and not ws.any()          # nothing was launched
    # no elements: nan like the reference, an empty gradient, no launch
    e = torch.zeros(0, device="cuda", requires_grad=True)
    loss = boot(e, torch.zeros(0, device="cuda"), torch.zeros(0, device="cuda"))
    loss.backward()
    assert torch.isnan(loss) and e.grad.numel() == 0
    assert torch.isnan(bce(torch.zeros(0, device="cuda"), torch.zeros(0, device="cuda")))
