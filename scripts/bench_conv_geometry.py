"""Layer-level micro-benchmark of the general conv kernels (csrc/conv3d_gen.hip): forward, backward-data and
backward-weights of nn.Conv3d geometries other than 3x3x3 / pad 1 and 1x1x1.  Prints ms and executed TFLOP/s
(2 * Cin * Cout * taps * output voxels per direction), HIP-event timed.

Shape spec: N,Cin,Cout,D,H,W,kz,ky,kx,sz,sy,sx,pz,py,px; several separated by ';'."""
import argparse, os, sys
import torch
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bodyct-dram_amd")]
from dram_amd import functional as HF
from dram_amd import _lib

DEFAULT = ";".join([
    "4,64,64,64,64,64,5,5,5,1,1,1,2,2,2",
    "4,64,64,128,128,128,3,3,3,1,1,1,0,0,0",
    "4,64,64,128,128,128,1,3,3,1,1,1,0,1,1",
    "4,32,64,128,128,128,3,3,3,2,2,2,1,1,1",
])
ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default=DEFAULT)
ap.add_argument("--iters", type=int, default=5)
args = ap.parse_args()
dev = torch.device("cuda:0")
st = torch.cuda.current_stream().cuda_stream


def timeit(fn, iters):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


for spec in args.shapes.split(";"):
    geom = [int(v) for v in spec.split(",")]
    N, Ci, Co, D, H, W, kz, ky, kx, sz, sy, sx, pz, py, px = geom
    out = HF.conv_out_size((D, H, W), (kz, ky, kx), (sz, sy, sx), (pz, py, px))
    x = torch.rand(N, Ci, D, H, W, device=dev) - 0.5
    w = torch.randn(Co, Ci, kz, ky, kx, device=dev) / (Ci * kz * ky * kx) ** 0.5
    y = torch.empty(N, Co, *out, device=dev)
    dy = torch.rand(N, Co, *out, device=dev) - 0.5
    dx = torch.empty_like(x)
    dw = torch.empty_like(w)
    nb = _lib.lib.dram_conv3d_wgrad_ws_bytes(*geom)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    flops = 2.0 * Ci * Co * kz * ky * kx * N * out[0] * out[1] * out[2]
    p = lambda t: t.data_ptr()
    t_f = timeit(lambda: _lib.call("dram_conv3d_fwd", p(x), p(w), None, p(y), *geom, st), args.iters)
    t_d = timeit(lambda: _lib.call("dram_conv3d_bwd_data", p(dy), p(w), p(dx), *geom, st), args.iters)
    t_w = timeit(lambda: _lib.call("dram_conv3d_wgrad", p(x), p(dy), p(dw), p(ws), nb, *geom, st), args.iters)
    name = f"[{N},{Ci}->{Co},{D}x{H}x{W}] k({kz},{ky},{kx}) s({sz},{sy},{sx}) p({pz},{py},{px})"
    print(f"{name:52s} fwd {t_f:8.3f} ms {flops / t_f / 1e9:6.1f} TF/s | bwd-data {t_d:8.3f} ms "
          f"{flops / t_d / 1e9:6.1f} TF/s | wgrad {t_w:8.3f} ms {flops / t_w / 1e9:6.1f} TF/s", flush=True)
