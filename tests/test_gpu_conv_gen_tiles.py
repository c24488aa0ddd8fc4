"""The three general-conv kernels (csrc/conv3d_gen.hip) beyond one tile per row and one box per split.

Each direction is called on its own through the C ABI (dram_conv3d_fwd, dram_conv3d_bwd_data, dram_conv3d_wgrad) on the cases
of tests/conv_gen_cases.py, whose block decodes tests/test_conv_gen_plan_cpu.py pins: several x and y blocks with ragged last
blocks and several channel tiles in the forward-shaped kernel (forward and backward-data phases, each WQ instantiation), and
several boxes per split, splits that cross from one sample into the next, a short last split and a short channel group in
backward-weights.  The reference is torch.nn.functional.conv3d with autograd in float64 on the CPU, computed once per case.

What a kernel may touch: every tensor handed to an entry point lies inside a larger device buffer, its base pointer `shift`
bytes off a 16-byte boundary.  Inputs are surrounded by NaN, so a halo or channel-tail read that leaves its tensor poisons the
result.  Outputs and the backward-weights workspace are NaN before the call and lie between GUARD words of a finite sentinel:
afterwards every output element must be finite (all of it written) and every guard word bit-identical (nothing else written).

Tolerance: max |got - ref| <= 1e-5 * max |ref| per tensor, the bound of test_conv_gen_matches_torch."""
import functools

import pytest
import torch
import torch.nn.functional as F

from dram_amd import _lib
from dram_amd import functional as HF

import conv_gen_cases as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
GUARD = 4096              # floats on either side of every output
SENTINEL = -12345.0
TOL = 1e-5
IDS = [c.name for c in G.CASES]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _offset(store, shift):
    """First element index >= GUARD of `store` whose address is `shift` bytes past a 16-byte boundary."""
    return GUARD + ((shift - (store.data_ptr() + 4 * GUARD)) % 16) // 4


def place_in(src, shift):
    """src (CPU) as a float32 device tensor `shift` bytes off 16-byte alignment, NaN on both sides."""
    store = torch.full((src.numel() + 2 * GUARD + 4,), NAN, dtype=torch.float32, device=DEV)
    lo = _offset(store, shift)
    t = store[lo:lo + src.numel()].view(src.shape)
    t.copy_(src)
    assert t.data_ptr() % 16 == shift
    return t


class PlacedOut:
    """NaN-filled float32 output of `shape`, `shift` bytes off 16-byte alignment, between guard words."""

    def __init__(self, shape, shift):
        n = 1
        for d in shape:
            n *= d
        self.store = torch.full((n + 2 * GUARD + 4,), SENTINEL, dtype=torch.float32, device=DEV)
        self.lo = _offset(self.store, shift)
        self.hi = self.lo + n
        self.t = self.store[self.lo:self.hi].view(shape)
        self.t.fill_(NAN)
        assert self.t.data_ptr() % 16 == shift
        self.before = self._guards()

    def _guards(self):
        bits = self.store.view(torch.int32)
        return torch.cat([bits[:self.lo], bits[self.hi:]]).clone()

    def guards_intact(self):
        return torch.equal(self._guards(), self.before)


@functools.lru_cache(maxsize=None)
def data(name):
    """Inputs and the float64 reference of a case: x, w, bias, dy, y, dx, dw (CPU, float64), shared by its three tests."""
    c = next(c for c in G.CASES if c.name == name)
    g = torch.Generator().manual_seed(1 + IDS.index(name))
    x = torch.randn(c.N, c.Cin, *c.size, generator=g, dtype=torch.float64)
    w = torch.randn(c.Cout, c.Cin, *c.k, generator=g, dtype=torch.float64) / (c.Cin * c.k[0] * c.k[1] * c.k[2]) ** 0.5
    b = torch.randn(c.Cout, generator=g, dtype=torch.float64) if c.bias else None
    # the device sees float32 inputs; the reference takes the same numbers
    x, w = x.float().double(), w.float().double()
    b = b.float().double() if c.bias else None
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv3d(xr, wr, b, stride=c.s, padding=c.p)
    assert tuple(y.shape[2:]) == G.plan(c)["out"]
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64).float().double()
    y.backward(dy)
    return dict(x=x, w=w, b=b, dy=dy, y=y.detach(), dx=xr.grad, dw=wr.grad)


def compare(name, got, ref, where):
    """got (device) against ref (float64): all finite, then TOL * max |ref|; `where(index)` names the tile of an element."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    bad = ~torch.isfinite(got)
    if bool(bad.any()):
        idx = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {got.numel()} elements not finite (not written, or computed from "
                             f"a read outside an input); first at {idx}: {where(idx)}")
    err = (got - ref).abs()
    scale = ref.abs().max().item()
    print(f"conv-gen-tiles: {name}: max abs err {err.max().item():.3e} = {err.max().item() / scale:.3e} * max |ref|")
    wrong = err > TOL * scale
    if bool(wrong.any()):
        idx = tuple(int(v) for v in wrong.nonzero()[0])
        raise AssertionError(f"{name}: max abs err {err.max().item():.3e} > {TOL} * {scale:.3e}; {int(wrong.sum())} elements "
                             f"beyond the bound, first at {idx} (got {got[idx].item():.6g}, want {ref[idx].item():.6g}): {where(idx)}")


def _where_fwd(la):
    def where(idx):
        n, co, z, y, x = idx
        return (f"(n {n}, channel {co}, z {z}, y {y}, x {x}) = channel tile {co // 32}, y block {y // la['BY']}, "
                f"x block {x // la['BX']} of {la['nbx']} (BX {la['BX']}, WQ {la['WQ']})")
    return where


def _where_dx(dxplan):
    def where(idx):
        n, ci, z, y, x = idx
        out = []
        for a, i in zip(range(3), (z, y, x)):
            ph = next(ph for ph in dxplan["axes"][a] if ph["Q"] > 0 and (i - ph["oo"]) % ph["os"] == 0
                      and 0 <= (i - ph["oo"]) // ph["os"] < ph["Q"])
            out.append((ph, (i - ph["oo"]) // ph["os"]))
        (_, _), (phy, qy), (phx, qx) = out
        if any(ph["T"] == 0 for ph, _ in out):
            return f"(n {n}, channel {ci}, z {z}, y {y}, x {x}) in a phase without taps (zero fill)"
        BX = 16 if phx["Q"] <= 16 else 32
        return (f"(n {n}, channel {ci}, z {z}, y {y}, x {x}) = phase r (z {out[0][0]['r']}, y {phy['r']}, x {phx['r']}), "
                f"grid x {qx} of {phx['Q']}, x block {qx // BX} (BX {BX}), y block {qy // (256 // BX)}")
    return where


def _where_dw(c, w):
    def where(idx):
        co, ci, kz, ky, kx = idx
        return (f"(co {co}, ci {ci}, tap {kz} {ky} {kx}) = channel tile {co // 32}, channel group {ci // w['CIB']} of {w['nci']}; "
                f"{w['nboxes']} boxes in {w['nsplit']} splits of {w['boxes_per_split']}")
    return where


def _blame_split(c, w, slabs, idx):
    """After a wrong dw element: the first split whose slab disagrees with the float64 sum over its own boxes."""
    d = data(c.name)
    co, ci = idx[0], idx[1]
    O = G.plan(c)["out"]
    xr = d["x"][:, ci:ci + 1]
    for split in range(w["nsplit"]):
        lo, hi = split * w["boxes_per_split"], min((split + 1) * w["boxes_per_split"], w["nboxes"])
        dy = torch.zeros(c.N, 1, *O, dtype=torch.float64)
        for box in range(lo, hi):
            bx, r = box % w["nbx"], box // w["nbx"]
            by, r = r % w["nby"], r // w["nby"]
            bz, n = r % w["nbz"], r // w["nbz"]
            sl = (n, 0, slice(2 * bz, 2 * bz + 2), slice(4 * by, 4 * by + 4), slice(32 * bx, 32 * bx + 32))
            dy[sl] = d["dy"][(n, co) + sl[2:]]
        wr = torch.zeros(1, 1, *c.k, dtype=torch.float64, requires_grad=True)
        F.conv3d(xr, wr, None, stride=c.s, padding=c.p).backward(dy)
        got = slabs[split, co, ci].double().cpu().view(c.k)
        if not bool(((got - wr.grad[0, 0]).abs() <= TOL * d["dw"].abs().max()).all()):
            return f"split {split} (boxes {lo}..{hi - 1}, {w['boxes_per_sample']} per sample) is the first whose slab is wrong"
    return "every split's slab agrees with its own boxes: the slab reduction is wrong"


@pytest.mark.parametrize("case", G.CASES, ids=IDS)
def test_forward(case):
    c, d, pl = case, data(case.name), G.plan(case)
    x, w = place_in(d["x"], c.shift), place_in(d["w"], c.shift)
    b = place_in(d["b"], c.shift) if c.bias else None
    y = PlacedOut(d["y"].shape, c.shift)
    before = HF.conv_gen_launch_counts()
    _lib.call("dram_conv3d_fwd", x.data_ptr(), w.data_ptr(), b.data_ptr() if c.bias else None, y.t.data_ptr(),
              *G.geom_args(c), _stream())
    torch.cuda.synchronize()
    after = HF.conv_gen_launch_counts()
    assert [a - b_ for a, b_ in zip(after, before)] == [1, 0, 0]
    compare(f"{c.name} y", y.t, d["y"], _where_fwd(pl["fwd"]))
    assert y.guards_intact(), "forward wrote outside y"


@pytest.mark.parametrize("case", G.CASES, ids=IDS)
def test_backward_data(case):
    c, d, pl = case, data(case.name), G.plan(case)
    dy, w = place_in(d["dy"], c.shift), place_in(d["w"], c.shift)
    dx = PlacedOut(d["x"].shape, c.shift)
    before = HF.conv_gen_launch_counts()
    _lib.call("dram_conv3d_bwd_data", dy.data_ptr(), w.data_ptr(), dx.t.data_ptr(), *G.geom_args(c), _stream())
    torch.cuda.synchronize()
    after = HF.conv_gen_launch_counts()
    # one launch per phase that has taps and grid points
    assert [a - b_ for a, b_ in zip(after, before)] == [0, len(pl["dx"]["launches"]), 0]
    compare(f"{c.name} dx", dx.t, d["dx"], _where_dx(pl["dx"]))
    assert dx.guards_intact(), "backward-data wrote outside dx"


@pytest.mark.parametrize("case", G.CASES, ids=IDS)
def test_backward_weights(case):
    c, d, pl = case, data(case.name), G.plan(case)
    wp = pl["wgrad"]
    x, dy = place_in(d["x"], c.shift), place_in(d["dy"], c.shift)
    ws_bytes = int(_lib.lib.dram_conv3d_wgrad_ws_bytes(*G.geom_args(c)))
    assert ws_bytes == wp["ws_bytes"]
    runs = []
    for _ in range(2):
        dw = PlacedOut(d["w"].shape, c.shift)
        ws = PlacedOut((wp["nsplit"], c.Cout, c.Cin, wp["T"]), c.shift)     # exactly ws_bytes
        before = HF.conv_gen_launch_counts()
        _lib.call("dram_conv3d_wgrad", x.data_ptr(), dy.data_ptr(), dw.t.data_ptr(), ws.t.data_ptr(), ws_bytes,
                  *G.geom_args(c), _stream())
        torch.cuda.synchronize()
        after = HF.conv_gen_launch_counts()
        assert [a - b_ for a, b_ in zip(after, before)] == [0, 0, 1]
        runs.append((dw, ws))
    dw, ws = runs[0]
    assert bool(torch.isfinite(ws.t).all()), "a slab element was not written, or summed a read outside x / dy"
    try:
        compare(f"{c.name} dw", dw.t, d["dw"], _where_dw(c, wp))
    except AssertionError as e:
        idx = tuple(int(v) for v in (~((dw.t.double().cpu() - d["dw"]).abs() <= TOL * d["dw"].abs().max())).nonzero()[0])
        raise AssertionError(f"{e}; {_blame_split(c, wp, ws.t, idx)}") from None
    for out, what in ((dw, "dw"), (ws, "the workspace")):
        assert out.guards_intact(), f"backward-weights wrote outside {what}"
    # the slabs are added in a fixed order: a second call gives the same bits
    assert torch.equal(runs[1][0].t, dw.t) and torch.equal(runs[1][1].t, ws.t)
    assert runs[1][0].guards_intact() and runs[1][1].guards_intact()
