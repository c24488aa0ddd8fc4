"""Micro-benchmark of the norm kernels of the fused engine's backward (dram_norm_bwd: reduce + finalise + apply, in place) and of
dram_row_affine_act at a full-resolution stage of the benchmark: [N, 64, 128^3]; then dram_norm_bwd_head / _pool_add against the
two-call compositions they replace (the 1x1x1 head's dx written out, the max-pool gradient accumulated, then dram_norm_bwd)."""
import os, sys
import torch
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bodyct-dram_amd")]
from dram_amd import _lib
N, C, S = int(os.environ.get("N", 16)), 64, 128 ** 3
dev = torch.device("cuda:0")
st = torch.cuda.current_stream().cuda_stream
g = torch.rand(N, C, S, device=dev); y = torch.rand(N, C, S, device=dev)
gamma = torch.rand(C, device=dev) + 0.5
mean = torch.rand(C, device=dev); rstd = torch.rand(C, device=dev) + 0.5
coef = torch.rand(2 * N * C, device=dev)
dgamma = torch.empty(C, device=dev); dbeta = torch.empty(C, device=dev)
ws = torch.empty(_lib.lib.dram_norm_ws_bytes(N, C, S), dtype=torch.uint8, device=dev)
out = torch.empty_like(g)
p = lambda t: t.data_ptr()
def bwd():
    _lib.call("dram_norm_bwd", p(g), p(y), p(gamma), p(mean), p(rstd), p(coef), p(g), p(dgamma), p(dbeta), 0, 1, 1, 1, N, C, S, p(ws), ws.numel(), st)
def act():
    _lib.call("dram_row_affine_act", p(y), p(coef), p(out), 1, N * C, S, st)
def t(fn, it=5):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(it): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / it
nb = g.numel() * 4
tb, ta = t(bwd), t(act)
print(f"norm_bwd [{N},{C},128^3]: {tb:.3f} ms = {5 * nb / tb / 1e9:.2f} TB/s (4R+1W)   row_affine_act: {ta:.3f} ms = {2 * nb / ta / 1e9:.2f} TB/s (1R+1W)")

E = 128
gh = torch.rand(N, 1, S, device=dev); wh = torch.rand(1, C, device=dev)
gp = torch.rand(N, C, S // 8, device=dev); idx = torch.randint(0, 8, (N, C, S // 8), dtype=torch.uint8, device=dev)
tail = (p(y), p(gamma), p(mean), p(rstd), p(coef))
def head_old():
    _lib.call("dram_conv3d_k1_bwd_lazy", p(gh), p(y), None, 0, p(wh), p(out), None, None, None, 0, N, C, 1, S, st)
    _lib.call("dram_norm_bwd", p(out), *tail, p(out), p(dgamma), p(dbeta), 0, 1, 1, 1, N, C, S, p(ws), ws.numel(), st)
def head_new():
    _lib.call("dram_norm_bwd_head", p(gh), p(wh), 1, *tail, p(out), p(dgamma), p(dbeta), 0, 1, 1, 1, N, C, S, p(ws), ws.numel(), st)
def pool_old():
    _lib.call("dram_maxpool3d_2_bwd_acc", p(gp), p(idx), p(g), N, C, E, E, E, st)
    bwd()
def pool_new():
    _lib.call("dram_norm_bwd_pool_add", p(g), p(gp), p(idx), E, E, E, *tail, p(g), p(dgamma), p(dbeta), 0, 1, 1, 1, N, C, p(ws), ws.numel(), st)
for name, old, new in (("head (Cout 1)", head_old, head_new), ("pool-add", pool_old, pool_new)):
    to, tn = t(old), t(new)
    print(f"{name}: two calls {to:.3f} ms, from the source {tn:.3f} ms")
