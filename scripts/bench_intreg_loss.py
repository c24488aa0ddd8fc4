"""Times dram_intreg_enc_loss_fwd/bwd (IntRegLoss: hinge + entropy, 8 B/voxel read) and, as the baseline, dram_intreg_loss_fwd/bwd
(IntRegRefineLoss, 12 B/voxel read) on the same 16x1x128^3 tensors through the C ABI: HIP events, median of 20 launches, GB/s of
the bytes each pass must move.

    python scripts/bench_intreg_loss.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bodyct-dram_amd")]
import torch
from dram_amd import _lib
from dram_amd.train_step import synthetic_batch

N, E = 16, 128
dev = "cuda"
b = synthetic_batch(N, E, 100, dev)
S = E ** 3
torch.manual_seed(0)
dense = torch.randn((N, 1, E, E, E), device=dev) * 2.0
out = torch.empty(2, device=dev)
gout = torch.tensor([2.0, 1.0], device=dev)
dd = torch.empty_like(dense)
keep = b.keep.reshape(-1).contiguous()
st = torch.cuda.current_stream().cuda_stream
p = lambda t: None if t is None else t.data_ptr()
lib = _lib.lib
ws_e = torch.empty(lib.dram_intreg_enc_loss_ws_bytes(N, S), dtype=torch.uint8, device=dev)
st_e = torch.empty(lib.dram_intreg_enc_loss_state_floats(N), device=dev)
ws_r = torch.empty(lib.dram_intreg_loss_ws_bytes(N, S), dtype=torch.uint8, device=dev)
st_r = torch.empty(lib.dram_intreg_loss_state_floats(N), device=dev)
runs = {
    "enc_fwd": (8, lambda: _lib.call("dram_intreg_enc_loss_fwd", p(dense), p(b.lobes), p(b.targets), p(b.weight), p(out), p(st_e), p(ws_e), ws_e.numel(), N, S, st)),
    "enc_bwd": (12, lambda: _lib.call("dram_intreg_enc_loss_bwd", p(dense), p(b.lobes), p(b.targets), p(b.weight), p(st_e), p(gout), p(dd), N, S, st)),
    "refine_fwd": (12, lambda: _lib.call("dram_intreg_loss_fwd", p(dense), None, p(b.lobes), p(b.lesions), p(keep), p(b.targets), p(b.weight), 0.1, p(out), p(st_r), p(ws_r), ws_r.numel(), N, S, st)),
    "refine_bwd": (16, lambda: _lib.call("dram_intreg_loss_bwd", p(dense), None, p(b.lobes), p(b.lesions), p(keep), p(b.targets), p(b.weight), p(st_r), p(gout), 0.1, p(dd), None, N, S, st)),
}
for name, (bpv, fn) in runs.items():
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    med = ts[len(ts) // 2]
    print(f"{name}: median {med * 1e3:.1f} us, min {ts[0] * 1e3:.1f} us, {bpv} B/voxel -> {N * S * bpv / (med * 1e-3) / 1e9:.0f} GB/s (median), out {out.tolist()}", flush=True)
