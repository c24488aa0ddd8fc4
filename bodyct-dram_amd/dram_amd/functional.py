"""torch.autograd Functions over the libdram_hip.so C ABI.

PyTorch is plumbing here: it owns the HBM buffers (caching allocator), the HIP
stream and the autograd tape; every forward / backward computation is a call
into the hand-written gfx950 kernels.  All tensors are fp32 NCDHW contiguous.
There is no fallback: CPU tensors raise.
"""
import ctypes
import math

import numpy as np
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import call

NORM_BATCH, NORM_GROUP = 0, 1


def _stream():
    return torch.cuda.current_stream().cuda_stream


class KernelTimer:
    """Optional HIP-event timing of individual kernel launches on the stream they run on
    (used by bench.py for the roofline line).  Disabled (None) by default: zero overhead."""

    def __init__(self):
        self.records = []   # (key, flops, bytes, start_event, end_event)

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for key, flops, nbytes, e0, e1 in self.records:
            d = out.setdefault(key, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
            d["launches"] += 1
            d["ms"] += e0.elapsed_time(e1)
            d["flops"] += flops
            d["bytes"] += nbytes
        return out


TIMER = None   # set to a KernelTimer() to record


def _timed_call(key, flops, nbytes, name, *args):
    if TIMER is None:
        call(name, *args)
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call(name, *args)
    e1.record()
    TIMER.records.append((key, flops, nbytes, e0, e1))


# kernel families of the 3x3x3 conv (include/dram_hip.h DRAM_K3_*)
K3_FWD_DIRECT, K3_FWD_WZ, K3_FWD_WZY, K3_WGRAD_DIRECT, K3_WGRAD_VEC, K3_WGRAD_WZ, K3_WGRAD_WZ_LAZY, K3_WGRAD_C1, \
    K3_FWD_C1, K3_WGRAD_WZY, K3_KINDS = range(11)


def conv_fwd_kernel_name(dhw, Cout, Cin, fused=False, dst_split=None, src=None):
    """Name of the forward / backward-data kernel instantiation the library launches for this shape, as rocprofv3
    prints it -- asked of the library itself (dram_conv3d_k3_fwd_choice_src: the same fwd_choice the launch goes through).
    `fused`: the variant with lazy operands / the statistics epilogue; `dst_split` = (C1, C2, D2, H2, W2) when the
    output is written to two tensors (backward-data of a conv whose input was a virtual concat); `src` = (x1, x2, ox): the
    source tensors of the launch (x2 the cropped second one or None, ox its window's x offset) -- a source off 16-byte
    alignment, or a crop window that is, sends a (z,y)-shaped launch to the z-only kernel."""
    c1, c2, d2, h2, w2 = dst_split if dst_split is not None else (Cout, 0, 0, 0, 0)
    sc2 = sd2 = sh2 = sw2 = sox = mis = 0
    if src is not None:
        x1, x2, sox = src
        mis = int(x1.data_ptr() % 16 != 0 or (x2 is not None and x2.data_ptr() % 16 != 0))
        if x2 is not None:
            sc2, sd2, sh2, sw2 = (int(v) for v in x2.shape[1:])
    buf = ctypes.create_string_buffer(96)
    kind = _lib.lib.dram_conv3d_k3_fwd_choice_src(Cin, Cout, dhw[0], dhw[1], dhw[2], c1, c2, d2, h2, w2, int(bool(fused)),
                                                  sc2, sd2, sh2, sw2, int(sox), mis, buf, len(buf))
    if kind < 0:
        raise _lib.DramHipError(f"dram_conv3d_k3_fwd_choice_src: {_lib.lib.dram_last_error().decode()}")
    return buf.value.decode()


def conv_wgrad_kernel_name(N, dhw, Cout, C1, C2=0, lazy=False):
    """Name of the backward-weights kernel instantiation for x = x1[N, C1] ++ crop(x2[N, C2]) (dram_conv3d_k3_wgrad_choice:
    the same wgrad_plan the launch goes through)."""
    buf = ctypes.create_string_buffer(96)
    kind = _lib.lib.dram_conv3d_k3_wgrad_choice(N, C1, C2, Cout, dhw[0], dhw[1], dhw[2], int(bool(lazy)), buf, len(buf))
    if kind < 0:
        raise _lib.DramHipError(f"dram_conv3d_k3_wgrad_choice: {_lib.lib.dram_last_error().decode()}")
    return buf.value.decode()


def conv_kernel_rows():
    """Names of all 3x3x3 conv kernel instantiations of the library, in the spelling of conv_fwd_kernel_name and
    conv_wgrad_kernel_name (dram_conv3d_k3_kernel_rows: the row tables every launch goes through)."""
    buf = ctypes.create_string_buffer(8192)
    n = _lib.lib.dram_conv3d_k3_kernel_rows(buf, len(buf))
    if n < 0:
        raise _lib.DramHipError(f"dram_conv3d_k3_kernel_rows: {_lib.lib.dram_last_error().decode()}")
    rows = buf.value.decode().splitlines()
    assert len(rows) == n
    return rows


def conv_launch_counts():
    """Launches per 3x3x3 conv kernel family (index = K3_*) since the library was loaded."""
    arr = (ctypes.c_ulonglong * K3_KINDS)()
    call("dram_conv3d_k3_launch_counts", ctypes.cast(arr, ctypes.c_void_p), K3_KINDS)
    return list(arr)


def _p(t):
    return None if t is None else t.data_ptr()


def _chk(t, name, ndim=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: tensor is on {t.device}; the DRAM HIP path only runs on a ROCm device "
                           f"(there is no CPU fallback)")
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected float32, got {t.dtype}")
    if ndim is not None and t.dim() != ndim:
        raise ValueError(f"{name}: expected {ndim}-d tensor, got shape {tuple(t.shape)}")
    return t.contiguous()


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def crop_offsets(small, big):
    """Start offsets of crop_concat_5d's centre crop: ceil((b - a) / 2) (reference parts.py:42-44)."""
    return tuple(int(math.ceil((b - a) / 2)) for a, b in zip(small, big))


# --------------------------------------------------------------------------- conv 3x3x3
# Packed filters of inference calls: inside `with cached_packs():` (the fused engine's no-gradient branch, LobeInference) a
# filter that has not changed since it was packed (same tensor, same storage, same in-place version counter) is not packed
# again -- whole-scan inference repacked all 14 filters of the network for every scan (1.1 ms of a 27 ms scan).  Training
# never takes this path (torch runs every autograd Function's forward with gradients disabled, so the grad mode cannot be
# the switch): the optimiser bumps the version every step, and a cache of packed filters (4x the parameters) would only
# cost memory there.
import contextlib as _contextlib
import weakref as _weakref
_PACK_CACHE_ON = 0


@_contextlib.contextmanager
def cached_packs():
    global _PACK_CACHE_ON
    _PACK_CACHE_ON += 1
    try:
        yield
    finally:
        _PACK_CACHE_ON -= 1


_PACK_CACHE = {}      # id(weight tensor) -> (weak reference to it, {mode: (data_ptr, version, packed)}); (a WeakKeyDictionary would
                      # compare tensors with ==, i.e. elementwise)


def _pack_cached(w):
    """The cache entry of tensor `w` ({mode: ...}) or None."""
    ent = _PACK_CACHE.get(id(w))
    return ent[1] if ent is not None and ent[0]() is w else None


def _pack(w, mode):
    co, ci = w.shape[0], w.shape[1]
    cacheable = _PACK_CACHE_ON > 0
    if cacheable:
        modes = _pack_cached(w)
        hit = modes.get(mode) if modes is not None else None
        if hit is not None and hit[0] == w.data_ptr() and hit[1] == w._version and hit[2].device == w.device:
            return hit[2]
    wt = torch.empty(_lib.lib.dram_conv3d_k3_packed_floats(co, ci), dtype=torch.float32, device=w.device)
    call("dram_conv3d_k3_pack_weights", _p(w), _p(wt), co, ci, mode, _stream())
    if cacheable:
        modes = _pack_cached(w)
        if modes is None:
            key = id(w)
            try:
                ref = _weakref.ref(w, lambda _r, key=key: _PACK_CACHE.pop(key, None))
            except TypeError:       # (a tensor subclass without weak references: no cache)
                return wt
            modes = {}
            _PACK_CACHE[key] = (ref, modes)
        modes[mode] = (w.data_ptr(), w._version, wt)
    elif _pack_cached(w) is not None:
        del _PACK_CACHE[id(w)]      # a training call: drop what an earlier evaluation pass left
    return wt


class CatView:
    """x1[n, C1, D, H, W] ++ centre-crop(x2[n, C2, D2, H2, W2]) along the channels, never materialised (x2 may be None): the
    source of a 3x3x3 conv (crop_concat_5d of reference parts.py:37-46,153 fused into it), or the split destination of its
    backward-data.  `channels`: what the filter expects of C1 + C2."""
    __slots__ = ("x1", "x2", "C1", "C2", "dhw2", "off")

    def __init__(self, x1, x2, dhw, channels=None):
        self.x1, self.x2, self.C1 = x1, x2, x1.shape[1]
        self.C2, self.dhw2, self.off = 0, (0, 0, 0), (0, 0, 0)
        if x2 is not None:
            self.C2, self.dhw2 = x2.shape[1], tuple(x2.shape[2:])
            if x2.shape[0] != x1.shape[0]:
                raise ValueError("conv3d: batch sizes of the two inputs differ")
            if not all(a <= b for a, b in zip(dhw, self.dhw2)):
                raise ValueError("conv3d: the second (skip) tensor must be at least as large as the first")
            self.off = crop_offsets(dhw, self.dhw2)
        if channels is not None and self.C1 + self.C2 != channels:
            raise ValueError(f"conv3d: input has {self.C1 + self.C2} channels, weight expects {channels}")

    def args(self):
        """(p1, C1, p2, C2, D2, H2, W2, oz, oy, ox) of the C ABI."""
        return (_p(self.x1), self.C1, _p(self.x2), self.C2, *self.dhw2, *self.off)

    @property
    def src(self):
        """conv_fwd_kernel_name's `src`, when this view is the source of the launch."""
        return self.x1, self.x2, self.off[2]

    @property
    def split(self):
        """conv_fwd_kernel_name's `dst_split`, when this view is the destination of the launch."""
        return (self.C1, self.C2, *self.dhw2) if self.x2 is not None else None


def _k3_cost(Ci, Co, y):
    """(flops, bytes) the KernelTimer books for a 3x3x3 conv launch over the voxels of y[n, ., D, H, W]."""
    vox = y.shape[0] * y.shape[2] * y.shape[3] * y.shape[4]
    return 54.0 * Ci * Co * vox, 4.0 * (Ci + Co) * vox


def conv3d_k3_launch_fwd(src, wt, bias, y, lazy=None, parts=None, nparts=0):
    """y[n, Co, D, H, W] = conv3d(src, w) (+ bias); `src` a CatView, `wt` = _pack(w, 0).  lazy = None: plain sources.
    lazy = (coef1, relu1, coef2, relu2): the fused variant -- a source with a coef is normalised (+ReLU) on load, and the
    moments of y go to parts[n * Co * nparts * 3] when given."""
    n, Co, D, H, W = y.shape
    Ci = src.C1 + src.C2
    key = conv_fwd_kernel_name((D, H, W), Co, Ci, fused=lazy is not None, src=src.src) if TIMER is not None else None
    if lazy is None:
        _timed_call(key, *_k3_cost(Ci, Co, y), "dram_conv3d_k3_fwd_ex", *src.args(), _p(wt), _p(bias),
                    _p(y), Co, None, 0, 0, 0, 0, 0, 0, 0, n, D, H, W, _stream())
    else:
        coef1, relu1, coef2, relu2 = lazy
        _timed_call(key, *_k3_cost(Ci, Co, y), "dram_conv3d_k3_fwd_fused", _p(src.x1), src.C1, _p(coef1), int(relu1),
                    _p(src.x2), src.C2, _p(coef2), int(relu2), *src.dhw2, *src.off, _p(wt), _p(bias), _p(y),
                    _p(parts), nparts, n, Co, D, H, W, _stream())


def conv3d_k3_dx2(x2, dhw):
    """The gradient buffer of a cropped second source: backward-data writes its crop window only, so it starts as zeros
    unless the window is the whole tensor."""
    return torch.empty_like(x2) if tuple(x2.shape[2:]) == tuple(dhw) else torch.zeros_like(x2)


def conv3d_k3_launch_bwd_data(dy, wt, dx1, dx2=None):
    """Backward-data of y = conv3d(x1 ++ crop(x2), w): the transposed conv of dy (`wt` = _pack(w, 1)) into dx1 and, when
    given, the crop window of dx2 (conv3d_k3_dx2)."""
    n, Co, D, H, W = dy.shape
    dst = CatView(dx1, dx2, (D, H, W))
    Ci = dst.C1 + dst.C2
    key = conv_fwd_kernel_name((D, H, W), Ci, Co, dst_split=dst.split, src=(dy, None, 0)) if TIMER is not None else None
    _timed_call(key, *_k3_cost(Ci, Co, dy), "dram_conv3d_k3_fwd_ex", _p(dy), Co, None, 0, 0, 0, 0, 0, 0, 0, _p(wt), None,
                *dst.args(), n, D, H, W, _stream())


def conv3d_k3_launch_wgrad(src, dy, w, lazy=(None, 0, None, 0)):
    """dw (like w) of y = conv3d(src, w) from dy[n, Co, D, H, W]; `src` a CatView, lazy = (coef1, relu1, coef2, relu2) as in
    conv3d_k3_launch_fwd (all plain by default)."""
    n, Co, D, H, W = dy.shape
    Ci = src.C1 + src.C2
    coef1, relu1, coef2, relu2 = lazy
    dw = torch.empty_like(w)
    ws = _ws(_lib.lib.dram_conv3d_k3_wgrad_ws_bytes(n, Ci, Co, D, H, W), dy.device)
    key = conv_wgrad_kernel_name(n, (D, H, W), Co, src.C1, src.C2, lazy=coef1 is not None or coef2 is not None) \
        if TIMER is not None else None
    _timed_call(key, *_k3_cost(Ci, Co, dy), "dram_conv3d_k3_wgrad_fused", _p(src.x1), src.C1, _p(coef1), int(relu1),
                _p(src.x2), src.C2, _p(coef2), int(relu2), *src.dhw2, *src.off, _p(dy), _p(dw), _p(ws), ws.numel(),
                n, Co, D, H, W, _stream())
    return dw


class Conv3dK3Fn(Function):
    """y = conv3d(cat(x1, crop(x2)), w, bias), k=3, stride 1, zero pad 1.  x2 may be None.
    (nn.Conv3d of reference parts.py:95,105,133,142,177,185; crop_concat_5d of parts.py:153 fused.)"""

    @staticmethod
    def forward(ctx, x1, x2, w, bias):
        x1 = _chk(x1, "conv3d input", 5)
        w = _chk(w, "conv3d weight", 5)
        N, C1, D, H, W = x1.shape
        Co, Ci = w.shape[0], w.shape[1]
        if tuple(w.shape[2:]) != (3, 3, 3):
            raise ValueError(f"Conv3dK3Fn: kernel {tuple(w.shape[2:])} is not 3x3x3")
        if x2 is not None:
            x2 = _chk(x2, "conv3d second input", 5)
        src = CatView(x1, x2, (D, H, W), channels=Ci)
        if bias is not None:
            bias = _chk(bias, "conv3d bias", 1)
        y = torch.empty((N, Co, D, H, W), dtype=torch.float32, device=x1.device)
        conv3d_k3_launch_fwd(src, _pack(w, 0), bias, y)
        ctx.save_for_backward(x1, x2, w)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x1, x2, w = ctx.saved_tensors
        dy = _chk(dy, "conv3d grad_output", 5)
        N, Co, D, H, W = dy.shape
        dx1 = dx2 = dw = db = None
        need1 = ctx.needs_input_grad[0]
        need2 = x2 is not None and ctx.needs_input_grad[1]
        if need1 or need2:
            dx1 = torch.empty_like(x1)
            if x2 is not None:
                dx2 = conv3d_k3_dx2(x2, (D, H, W))
            conv3d_k3_launch_bwd_data(dy, _pack(w, 1), dx1, dx2)   # filter of the transposed conv: [27][Co][Ci]
            if not need1:
                dx1 = None
            if not need2:
                dx2 = None
        if ctx.needs_input_grad[2]:
            dw = conv3d_k3_launch_wgrad(CatView(x1, x2, (D, H, W)), dy, w)
        if ctx.has_bias and ctx.needs_input_grad[3]:
            S = D * H * W
            db = torch.empty(Co, dtype=torch.float32, device=dy.device)
            ws = _ws(_lib.lib.dram_channel_sum_ws_bytes(N, Co, S), dy.device)
            call("dram_channel_sum", _p(dy), _p(db), _p(ws), ws.numel(), N, Co, S, _stream())
        return dx1, dx2, dw, db


def conv3d_k3(x, w, bias=None, skip=None):
    return Conv3dK3Fn.apply(x, skip, w, bias)


# --------------------------------------------------------------------------- conv 1x1x1 (+bias)
class Conv3dK1Fn(Function):
    """The regression head top_layer = nn.Conv3d(C, out_ch, 1) (reference models.py:109-110,145)."""

    @staticmethod
    def forward(ctx, x, w, bias):
        x = _chk(x, "conv1x1 input", 5)
        w = _chk(w, "conv1x1 weight", 5)
        N, Ci, D, H, W = x.shape
        Co = w.shape[0]
        if w.shape[1] != Ci or tuple(w.shape[2:]) != (1, 1, 1):
            raise ValueError(f"conv1x1: weight {tuple(w.shape)} does not match input channels {Ci}")
        if bias is not None:
            bias = _chk(bias, "conv1x1 bias", 1)
        y = torch.empty((N, Co, D, H, W), dtype=torch.float32, device=x.device)
        call("dram_conv3d_k1_fwd", _p(x), _p(w), _p(bias), _p(y), N, Ci, Co, D * H * W, _stream())
        ctx.save_for_backward(x, w)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = _chk(dy, "conv1x1 grad_output", 5)
        N, Ci, D, H, W = x.shape
        Co, S = w.shape[0], D * H * W
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(w) if ctx.needs_input_grad[1] else None
        db = torch.empty(Co, dtype=torch.float32, device=x.device) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        ws = _ws(_lib.lib.dram_conv3d_k1_bwd_ws_bytes(N, Ci, Co, S), x.device)
        call("dram_conv3d_k1_bwd", _p(dy), _p(x), _p(w), _p(dx), _p(dw), _p(db), _p(ws), ws.numel(),
             N, Ci, Co, S, _stream())
        return dx, dw, db


def conv3d_k1(x, w, bias=None):
    return Conv3dK1Fn.apply(x, w, bias)


# --------------------------------------------------------------------------- general conv
# kernel families of the general conv (include/dram_hip.h DRAM_CONV_GEN_*)
GEN_FWD, GEN_BWD_DATA, GEN_WGRAD, GEN_KINDS = range(4)


def conv_gen_launch_counts():
    """Launches per general-conv kernel family (index = GEN_*) since the library was loaded."""
    arr = (ctypes.c_ulonglong * GEN_KINDS)()
    call("dram_conv3d_gen_launch_counts", ctypes.cast(arr, ctypes.c_void_p), GEN_KINDS)
    return list(arr)


def _triple(v, name):
    t = tuple(int(e) for e in v) if isinstance(v, (tuple, list)) else (int(v),) * 3
    if len(t) != 3:
        raise ValueError(f"conv3d: {name} needs 1 or 3 values, got {v}")
    return t


def conv_out_size(size, kernel, stride, padding):
    """Output size of nn.Conv3d per axis (dilation 1): (I + 2p - k) // s + 1; ValueError if below 1."""
    out = tuple((i + 2 * p - k) // s + 1 if i + 2 * p >= k else 0 for i, k, s, p in zip(size, kernel, stride, padding))
    if min(out) < 1:
        raise ValueError(f"conv3d: input {tuple(size)} with kernel {tuple(kernel)}, stride {tuple(stride)} and padding "
                         f"{tuple(padding)} gives output size {out}")
    return out


class Conv3dGenFn(Function):
    """y = conv3d(x, w, bias, stride, padding) for kernels 1..7, padding 0..max(k-1, 1) and stride 1 or 2 per axis
    (nn.Conv3d of reference parts.py:66-196 / models.py:54-112 built with other kernel_sizes / padding_list /
    conv_strides than the standard 3x3x3 pad 1 and 1x1x1 pad 0)."""

    @staticmethod
    def forward(ctx, x, w, bias, stride, padding):
        x = _chk(x, "conv3d input", 5)
        w = _chk(w, "conv3d weight", 5)
        N, Ci, D, H, W = x.shape
        Co = w.shape[0]
        k = tuple(w.shape[2:])
        if w.shape[1] != Ci:
            raise ValueError(f"conv3d: input has {Ci} channels, weight expects {w.shape[1]}")
        out = conv_out_size((D, H, W), k, stride, padding)
        if bias is not None:
            bias = _chk(bias, "conv3d bias", 1)
        y = torch.empty((N, Co) + out, dtype=torch.float32, device=x.device)
        geom = (N, Ci, Co, D, H, W) + k + tuple(stride) + tuple(padding)
        vox = N * out[0] * out[1] * out[2]
        flops = 2.0 * Ci * Co * k[0] * k[1] * k[2] * vox
        _timed_call("conv3d_gen_fwd_kernel", flops, 4.0 * (Ci * D * H * W * N + Co * vox), "dram_conv3d_fwd",
                    _p(x), _p(w), _p(bias), _p(y), *geom, _stream())
        ctx.save_for_backward(x, w)
        ctx.has_bias = bias is not None
        ctx.geom = geom
        ctx.flops = flops
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = _chk(dy, "conv3d grad_output", 5)
        geom = ctx.geom
        N, Co = geom[0], geom[2]
        st = _stream()
        dx = dw = db = None
        nbytes = 4.0 * (x.numel() + dy.numel())
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            _timed_call("conv3d_gen_bwd_data", ctx.flops, nbytes, "dram_conv3d_bwd_data", _p(dy), _p(w), _p(dx), *geom, st)
        if ctx.needs_input_grad[1]:
            dw = torch.empty_like(w)
            ws = _ws(_lib.lib.dram_conv3d_wgrad_ws_bytes(*geom), dy.device)
            _timed_call("conv3d_gen_wgrad_kernel", ctx.flops, nbytes, "dram_conv3d_wgrad", _p(x), _p(dy), _p(dw), _p(ws),
                        ws.numel(), *geom, st)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            S = dy.shape[2] * dy.shape[3] * dy.shape[4]
            db = torch.empty(Co, dtype=torch.float32, device=dy.device)
            ws = _ws(_lib.lib.dram_channel_sum_ws_bytes(N, Co, S), dy.device)
            call("dram_channel_sum", _p(dy), _p(db), _p(ws), ws.numel(), N, Co, S, st)
        return dx, dw, db, None, None


def conv3d_gen(x, w, bias=None, stride=1, padding=0):
    """General 3-D convolution (zero padding, dilation 1, groups 1); see Conv3dGenFn."""
    return Conv3dGenFn.apply(x, w, bias, _triple(stride, "stride"), _triple(padding, "padding"))


# --------------------------------------------------------------------------- norm (+ReLU)
class NormActFn(Function):
    """BatchNorm3d / GroupNorm with optional fused ReLU (normal_wrapper + act_wrapper,
    reference parts.py:17-35,48-54).  `running_mean/var` are updated in place when given
    (training BatchNorm with track_running_stats)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, kind, groups, use_batch_stats, momentum, eps, relu):
        x = _chk(x, "norm input")
        if x.dim() < 3:
            raise ValueError("norm: expected (N, C, *spatial)")
        N, C = x.shape[0], x.shape[1]
        S = x.numel() // (N * C)
        dev = x.device
        nstat = C if kind == NORM_BATCH else N * groups
        y = torch.empty_like(x)
        save_mean = torch.empty(nstat, dtype=torch.float32, device=dev)
        save_rstd = torch.empty(nstat, dtype=torch.float32, device=dev)
        rowcoef = torch.empty(2 * N * C, dtype=torch.float32, device=dev)
        st = _stream()
        if gamma is not None:
            gamma = _chk(gamma, "norm weight", 1)
        if beta is not None:
            beta = _chk(beta, "norm bias", 1)
        if use_batch_stats:
            ws = _ws(_lib.lib.dram_norm_ws_bytes(N, C, S), dev)
            call("dram_norm_fwd_train", _p(x), _p(gamma), _p(beta), _p(y), _p(save_mean), _p(save_rstd), _p(rowcoef),
                 _p(running_mean), _p(running_var), float(momentum), float(eps), kind, groups, int(relu),
                 N, C, S, _p(ws), ws.numel(), st)
        else:
            call("dram_bn_fwd_eval", _p(x), _p(gamma), _p(beta), _p(running_mean), _p(running_var), _p(y),
                 _p(save_mean), _p(save_rstd), _p(rowcoef), float(eps), int(relu), N, C, S, st)
        ctx.save_for_backward(x, gamma, save_mean, save_rstd, rowcoef)
        ctx.cfg = (kind, groups, bool(use_batch_stats), bool(relu), beta is not None)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, gamma, save_mean, save_rstd, rowcoef = ctx.saved_tensors
        kind, groups, batch_stats, relu, has_beta = ctx.cfg
        dy = _chk(dy, "norm grad_output")
        N, C = x.shape[0], x.shape[1]
        S = x.numel() // (N * C)
        dev = x.device
        dx = torch.empty_like(x)
        dgamma = torch.empty(C, dtype=torch.float32, device=dev) if gamma is not None else None
        dbeta = torch.empty(C, dtype=torch.float32, device=dev) if has_beta else None
        ws = _ws(_lib.lib.dram_norm_ws_bytes(N, C, S), dev)
        call("dram_norm_bwd", _p(dy), _p(x), _p(gamma), _p(save_mean), _p(save_rstd), _p(rowcoef), _p(dx),
             _p(dgamma), _p(dbeta), kind, groups, int(relu), int(batch_stats), N, C, S, _p(ws), ws.numel(), _stream())
        return dx, dgamma, dbeta, None, None, None, None, None, None, None, None


def norm_act(x, gamma, beta, running_mean, running_var, kind, groups, use_batch_stats, momentum, eps, relu):
    return NormActFn.apply(x, gamma, beta, running_mean, running_var, kind, groups, use_batch_stats, momentum, eps, relu)


def sync_bn_combine(local, group, running_mean, running_var, momentum):
    """Cross-rank combine of BatchNorm statistics.  `local`: this rank's fp64 [2C + 1] buffer, {mean, M2} per channel
    (the layout of dram_bn_stats) and its element count per channel in the last slot.  All-gather over `group`, Chan's
    parallel formula in fp64, running statistics (when given) from the GLOBAL moments.  Returns the global fp32 mean, the
    biased fp32 variance and the total count."""
    import torch.distributed as dist
    C = (local.numel() - 1) // 2
    world = dist.get_world_size(group)
    allst = [torch.empty_like(local) for _ in range(world)]
    dist.all_gather(allst, local, group=group)
    allst = torch.stack(allst)                                   # [world, 2C+1]
    cnt = allst[:, 2 * C].view(world, 1)
    means, m2s = allst[:, 0:2 * C:2], allst[:, 1:2 * C:2]
    total = cnt.sum()
    mean = (means * cnt).sum(0) / total
    m2 = (m2s + cnt * (means - mean) ** 2).sum(0)                # Chan's parallel combine
    var = m2 / total                                             # biased
    mean_f, var_f = mean.float(), var.float()
    if running_mean is not None:
        with torch.no_grad():
            unb = (m2 / (total - 1.0)).float() if float(total) > 1.0 else var_f
            running_mean.mul_(1.0 - momentum).add_(mean_f, alpha=momentum)
            running_var.mul_(1.0 - momentum).add_(unb, alpha=momentum)
    return mean_f, var_f, float(total)


def sync_bn_backward(dy, x, gamma, save_mean, save_rstd, rowcoef, total, group, relu, dx, has_beta):
    """Backward of a BatchNorm (+ReLU if `relu`) whose statistics span the `total` elements per channel of all ranks of
    `group`: this rank's {sum dy', sum dy'*xhat} in fp64, all-reduced, applied into `dx` (which may be `dy` itself).
    Returns (dgamma, dbeta) -- taken from the LOCAL sums, before the exchange (see SyncBatchNormFn) -- or None where the
    norm has no such parameter."""
    import torch.distributed as dist
    N, C = x.shape[0], x.shape[1]
    S = x.numel() // (N * C)
    st = _stream()
    ws = _ws(_lib.lib.dram_norm_ws_bytes(N, C, S), x.device)
    sums = torch.empty(2 * C, dtype=torch.float64, device=x.device)
    call("dram_bn_bwd_sums", _p(dy), _p(x), _p(save_mean), _p(save_rstd), _p(rowcoef), _p(sums), int(relu), N, C, S,
         _p(ws), ws.numel(), st)
    dbeta = sums[0::2].float() if has_beta else None
    dgamma = sums[1::2].float() if gamma is not None else None
    dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=group)
    call("dram_bn_bwd_apply_sums", _p(dy), _p(x), _p(gamma), _p(save_mean), _p(save_rstd), _p(rowcoef), _p(sums),
         float(total), _p(dx), int(relu), N, C, S, _p(ws), ws.numel(), st)
    return dgamma, dbeta


class SyncBatchNormFn(Function):
    """Training-mode BatchNorm whose statistics span all ranks of a process group (nn.SyncBatchNorm, the
    reference's normal_wrapper "sbn", parts.py:32-33, under data parallelism).  Two exchanges per layer and
    direction, 2*C doubles each: all-gather of {mean, M2, count} in forward (combined with Chan's formula in
    fp64), all-reduce of {sum dy', sum dy'*xhat} in backward -- like torch's SyncBatchNorm, the parameter
    gradients stay local sums and are averaged by the data-parallel gradient all-reduce."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, momentum, eps, relu, group):
        x = _chk(x, "sync-bn input")
        N, C = x.shape[0], x.shape[1]
        S = x.numel() // (N * C)
        dev = x.device
        st = _stream()
        ws = _ws(_lib.lib.dram_norm_ws_bytes(N, C, S), dev)
        local = torch.empty(2 * C + 1, dtype=torch.float64, device=dev)
        call("dram_bn_stats", _p(x), _p(local), N, C, S, _p(ws), ws.numel(), st)
        local[2 * C] = float(N * S)
        mean_f, var_f, total = sync_bn_combine(local, group, running_mean, running_var, momentum)
        y = torch.empty_like(x)
        save_mean = torch.empty(C, dtype=torch.float32, device=dev)
        save_rstd = torch.empty(C, dtype=torch.float32, device=dev)
        rowcoef = torch.empty(2 * N * C, dtype=torch.float32, device=dev)
        if gamma is not None:
            gamma = _chk(gamma, "sync-bn weight", 1)
        if beta is not None:
            beta = _chk(beta, "sync-bn bias", 1)
        call("dram_bn_fwd_eval", _p(x), _p(gamma), _p(beta), _p(mean_f), _p(var_f), _p(y), _p(save_mean), _p(save_rstd),
             _p(rowcoef), float(eps), int(relu), N, C, S, st)
        ctx.save_for_backward(x, gamma, save_mean, save_rstd, rowcoef)
        ctx.cfg = (bool(relu), beta is not None, total, group)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, gamma, save_mean, save_rstd, rowcoef = ctx.saved_tensors
        relu, has_beta, total, group = ctx.cfg
        dy = _chk(dy, "sync-bn grad_output")
        dx = torch.empty_like(x)
        dgamma, dbeta = sync_bn_backward(dy, x, gamma, save_mean, save_rstd, rowcoef, total, group, relu, dx, has_beta)
        return dx, dgamma, dbeta, None, None, None, None, None, None


def sync_batch_norm(x, gamma, beta, running_mean, running_var, momentum, eps, relu, group=None):
    return SyncBatchNormFn.apply(x, gamma, beta, running_mean, running_var, momentum, eps, relu, group)


class ReLUFn(Function):
    @staticmethod
    def forward(ctx, x):
        x = _chk(x, "relu input")
        y = torch.empty_like(x)
        call("dram_relu_fwd", _p(x), _p(y), x.numel(), _stream())
        ctx.save_for_backward(y)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = _chk(dy, "relu grad_output")
        dx = torch.empty_like(dy)
        call("dram_relu_bwd", _p(dy), _p(y), _p(dx), dy.numel(), _stream())
        return dx


def relu(x):
    return ReLUFn.apply(x)


# --------------------------------------------------------------------------- max pool 2x2x2
class PReLUFn(Function):
    """nn.PReLU (act_wrapper "prelu", reference parts.py:51-52)."""

    @staticmethod
    def forward(ctx, x, a):
        x, a = _chk(x, "prelu input"), _chk(a, "prelu weight", 1)
        if x.dim() < 2:
            raise ValueError("prelu: expected (N, C, *spatial)")
        N, C = x.shape[0], x.shape[1]
        if a.numel() not in (1, C):
            raise ValueError(f"prelu: {a.numel()} parameters for {C} channels")
        y = torch.empty_like(x)
        call("dram_prelu_fwd", _p(x), _p(a), _p(y), N, C, a.numel(), x.numel() // (N * C), _stream())
        ctx.save_for_backward(x, a)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, a = ctx.saved_tensors
        dy = _chk(dy, "prelu grad_output")
        N, C = x.shape[0], x.shape[1]
        S = x.numel() // (N * C)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        da = torch.empty_like(a)
        ws = _ws(_lib.lib.dram_prelu_bwd_ws_bytes(N, C, S), x.device)
        call("dram_prelu_bwd", _p(dy), _p(x), _p(a), _p(dx), _p(da), _p(ws), ws.numel(), N, C, a.numel(), S, _stream())
        return dx, da


def prelu(x, a):
    return PReLUFn.apply(x, a)


def dropout_constants(p):
    """(threshold24, scale) of dram_dropout for drop probability p: an element is kept iff its 24-bit uniform is
    >= threshold24 = round(p * 2^24), so the kept share is exactly 1 - threshold24 / 2^24; scale is the fp64 quotient
    1 / (1 - p) rounded once to fp32 (0 when p == 1: everything is dropped)."""
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"dropout probability has to be between 0 and 1, but got {p}")
    return int(round(p * 2 ** 24)), (0.0 if p == 1.0 else float(np.float32(1.0 / (1.0 - p))))


class DropoutFn(Function):
    """nn.Dropout in training mode (reference parts.py:95-96).  The mask is Philox4x32-10 of (seed, offset, element index)
    (include/dram_hip.h) and is recomputed in the backward pass: ctx keeps two integers and no tensor.  Seed and offset are
    the device generator's, and a call advances its offset by 4 as an ATen kernel that consumes up to four values per
    thread does, so torch.manual_seed, get_rng_state / set_rng_state and torch.utils.checkpoint's RNG preservation apply."""

    @staticmethod
    def forward(ctx, x, p):
        x = _chk(x, "dropout input")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("dropout: the stream is capturing a graph; the generator's offset cannot be read there "
                               "(graph capture of dropout is not supported)")
        ctx.threshold24, ctx.scale = dropout_constants(p)
        gen = torch.cuda.default_generators[x.device.index]
        ctx.seed, ctx.offset = gen.initial_seed(), gen.get_offset()
        gen.set_offset(ctx.offset + 4)
        y = torch.empty_like(x)
        call("dram_dropout", _p(x), _p(y), x.numel(), ctx.threshold24, ctx.scale, ctx.seed, ctx.offset, _stream())
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        dy = _chk(dy, "dropout grad_output")
        dx = torch.empty_like(dy)
        call("dram_dropout", _p(dy), _p(dx), dy.numel(), ctx.threshold24, ctx.scale, ctx.seed, ctx.offset, _stream())
        return dx, None


def dropout(x, p):
    return DropoutFn.apply(x, p)


class GlobalMaxFn(Function):
    """F.adaptive_max_pool3d(x, 1).view(B, C) (reference models.py:41-42)."""

    @staticmethod
    def forward(ctx, x):
        x = _chk(x, "global max input")
        B, C = x.shape[0], x.shape[1]
        S = x.numel() // (B * C)
        out = torch.empty((B, C), dtype=torch.float32, device=x.device)
        idx = torch.empty((B, C), dtype=torch.int64, device=x.device)
        call("dram_global_max_fwd", _p(x), _p(out), _p(idx), B * C, S, _stream())
        ctx.save_for_backward(idx)
        ctx.shape = tuple(x.shape)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        dout = _chk(dout, "global max grad_output")
        dx = torch.empty(ctx.shape, dtype=torch.float32, device=dout.device)
        B, C = ctx.shape[0], ctx.shape[1]
        call("dram_global_max_bwd", _p(dout), _p(idx), _p(dx), B * C, dx.numel() // (B * C), _stream())
        return dx


def global_max(x):
    return GlobalMaxFn.apply(x)


class MaxPool2Fn(Function):
    """nn.MaxPool3d(2, 2, 0) (reference parts.py:191)."""

    @staticmethod
    def forward(ctx, x):
        x = _chk(x, "maxpool input", 5)
        N, C, D, H, W = x.shape
        out = torch.empty((N, C, D // 2, H // 2, W // 2), dtype=torch.float32, device=x.device)
        idx = torch.empty(out.shape, dtype=torch.uint8, device=x.device)
        call("dram_maxpool3d_2_fwd", _p(x), _p(out), _p(idx), N, C, D, H, W, _stream())
        ctx.save_for_backward(idx)
        ctx.in_shape = tuple(x.shape)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        dout = _chk(dout, "maxpool grad_output", 5)
        N, C, D, H, W = ctx.in_shape
        dx = torch.empty(ctx.in_shape, dtype=torch.float32, device=dout.device)
        call("dram_maxpool3d_2_bwd", _p(dout), _p(idx), _p(dx), N, C, D, H, W, _stream())
        return dx


def max_pool3d_2(x):
    return MaxPool2Fn.apply(x)


POOL_LIMITS = "kernel 1..5, stride 1..5 and padding 0..kernel/2 per axis, dilation 1, ceil_mode=False"


def max_pool3d_geometry(shape, kernel_size, stride=None, padding=0):
    """(kernel, stride, padding, output size), each a 3-tuple, of nn.MaxPool3d(kernel_size, stride, padding) with dilation 1
    and floor mode on an input whose last three dimensions are shape[-3:].  Ints mean all three axes and stride=None the
    kernel size, as in torch.  ValueError where torch refuses too (padding above kernel/2, an output extent below 1);
    NotImplementedError for sizes the kernel does not take."""
    def triple(v, name):
        t = tuple(int(e) for e in v) if isinstance(v, (tuple, list)) else (int(v),) * 3
        if len(t) != 3:
            raise ValueError(f"max_pool3d: {name} needs 1 or 3 values, got {v}")
        return t
    k = triple(kernel_size, "kernel_size")
    s = k if stride is None or (isinstance(stride, (tuple, list)) and len(stride) == 0) else triple(stride, "stride")
    p = triple(padding, "padding")
    if min(k) < 1 or min(s) < 1 or min(p) < 0:
        raise ValueError(f"max_pool3d: kernel {k} and stride {s} must be positive and padding {p} non-negative")
    if max(k) > 5 or max(s) > 5:
        raise NotImplementedError(f"max_pool3d: kernel {k} / stride {s} is not implemented; supported: {POOL_LIMITS}")
    if any(pp > kk // 2 for kk, pp in zip(k, p)):
        raise ValueError(f"max_pool3d: padding {p} must be at most half of the kernel {k}")
    size = tuple(int(n) for n in shape[-3:])
    out = tuple((n + 2 * pp - kk) // ss + 1 if n + 2 * pp >= kk else 0 for n, kk, ss, pp in zip(size, k, s, p))
    if len(size) != 3 or min(size) < 1 or min(out) < 1:
        raise ValueError(f"max_pool3d: input {size} with kernel {k}, stride {s} and padding {p} gives output size {out}")
    return k, s, p, out


class MaxPoolFn(Function):
    """nn.MaxPool3d(kernel_size, stride, padding) with dilation 1 and floor mode (pool_ksize / pool_strides / pool_pad of
    reference parts.py:157-196).  Keeps the uint8 window offsets of the maxima and the geometry."""

    @staticmethod
    def forward(ctx, x, kernel_size, stride, padding):
        x = _chk(x, "maxpool input", 5)
        N, C, D, H, W = x.shape
        k, s, p, osz = max_pool3d_geometry(x.shape, kernel_size, stride, padding)
        out = torch.empty((N, C) + osz, dtype=torch.float32, device=x.device)
        idx = torch.empty(out.shape, dtype=torch.uint8, device=x.device)
        call("dram_maxpool3d_fwd", _p(x), _p(out), _p(idx), N, C, D, H, W, *k, *s, *p, _stream())
        ctx.save_for_backward(idx)
        ctx.geometry = (N, C, D, H, W, *k, *s, *p)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        dout = _chk(dout, "maxpool grad_output", 5)
        dx = torch.empty(ctx.geometry[:5], dtype=torch.float32, device=dout.device)
        call("dram_maxpool3d_bwd", _p(dout), _p(idx), _p(dx), *ctx.geometry, _stream())
        return dx, None, None, None


def max_pool3d(x, kernel_size, stride=None, padding=0):
    return MaxPoolFn.apply(x, kernel_size, stride, padding)


# --------------------------------------------------------------------------- trilinear resize
# workspace cap of the two-stage trilinear backward (the z-reduced intermediate of a group of planes)
TRI_BWD_WS_CAP = 1 << 30
TRI_BWD_ROUTES = ("z+yx4", "z+gather", "gather", "general")


def trilinear_bwd_choice(dy, dx, ws, in_shape):
    """(route, group) of a dram_upsample_trilinear_ac_bwd_ws call with these tensors (ws: the uint8 workspace, or None) --
    asked of the library itself (dram_upsample_trilinear_ac_bwd_choice: the same choice the launch goes through).  route:
    "z+yx4" / "z+gather" = trilinear_bwd_z_kernel into the workspace, then trilinear_bwd_yx4_kernel / trilinear_bwd_kernel,
    `group` planes per round; "gather" = trilinear_bwd_kernel alone; "general" = trilinear_bwd_general_kernel (group 0)."""
    N, C, D, H, W = in_shape
    Do, Ho, Wo = dy.shape[-3:]
    group = ctypes.c_int64(0)
    route = _lib.lib.dram_upsample_trilinear_ac_bwd_choice(
        int(dy.data_ptr() % 16 != 0), int(dx.data_ptr() % 16 != 0), int(ws is not None and ws.data_ptr() % 16 != 0),
        ws.numel() * ws.element_size() if ws is not None else 0, N, C, D, H, W, Do, Ho, Wo, ctypes.byref(group))
    if route < 0:
        raise _lib.DramHipError(f"dram_upsample_trilinear_ac_bwd_choice: {_lib.lib.dram_last_error().decode()}")
    return TRI_BWD_ROUTES[route], int(group.value)


def trilinear_ac_backward(dy, in_shape):
    """Gradient w.r.t. the [N, C, D, H, W] = `in_shape` input of the align_corners=True trilinear upsampling that gave dy."""
    N, C, D, H, W = in_shape
    Do, Ho, Wo = dy.shape[-3:]
    dx = torch.empty(in_shape, dtype=torch.float32, device=dy.device)
    full = _lib.lib.dram_upsample_trilinear_ac_bwd_ws_bytes(N, C, D, H, W, Do, Ho, Wo)
    ws = _ws(min(full, TRI_BWD_WS_CAP), dy.device) if full else None
    call("dram_upsample_trilinear_ac_bwd_ws", _p(dy), _p(dx), _p(ws), ws.numel() if ws is not None else 0,
         N, C, D, H, W, Do, Ho, Wo, _stream())
    return dx


class TrilinearACFn(Function):
    """nn.Upsample(mode='trilinear', align_corners=True) (reference parts.py:149, models.py:146)."""

    @staticmethod
    def forward(ctx, x, size):
        x = _chk(x, "upsample input", 5)
        N, C, D, H, W = x.shape
        Do, Ho, Wo = (int(s) for s in size)
        y = torch.empty((N, C, Do, Ho, Wo), dtype=torch.float32, device=x.device)
        call("dram_upsample_trilinear_ac_fwd", _p(x), _p(y), N, C, D, H, W, Do, Ho, Wo, _stream())
        ctx.in_shape = (N, C, D, H, W)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        return trilinear_ac_backward(_chk(dy, "upsample grad_output", 5), ctx.in_shape), None


def upsample_trilinear_ac(x, size=None, scale_factor=None):
    if size is None:
        if scale_factor is None:
            raise ValueError("either size or scale_factor should be defined")
        sf = scale_factor if isinstance(scale_factor, (tuple, list)) else (scale_factor,) * 3
        # torch: output = floor(input * scale_factor)
        size = tuple(int(math.floor(float(d) * float(s))) for d, s in zip(x.shape[2:], sf))
    elif not isinstance(size, (tuple, list, torch.Size)):
        size = (size,) * 3
    return TrilinearACFn.apply(x, tuple(size))


# --------------------------------------------------------------------------- crop + concat
class CropConcatFn(Function):
    """crop_concat_5d (reference parts.py:37-46)."""

    @staticmethod
    def forward(ctx, t1, t2):
        t1 = _chk(t1, "crop_concat t1", 5)
        t2 = _chk(t2, "crop_concat t2", 5)
        N, C1, D, H, W = t1.shape
        C2, D2, H2, W2 = t2.shape[1:]
        oz, oy, ox = crop_offsets((D, H, W), (D2, H2, W2))
        out = torch.empty((N, C1 + C2, D, H, W), dtype=torch.float32, device=t1.device)
        call("dram_crop_concat_fwd", _p(t1), _p(t2), _p(out), N, C1, C2, D, H, W, D2, H2, W2, oz, oy, ox, _stream())
        ctx.geom = (N, C1, C2, D, H, W, D2, H2, W2, oz, oy, ox)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        N, C1, C2, D, H, W, D2, H2, W2, oz, oy, ox = ctx.geom
        dout = _chk(dout, "crop_concat grad_output", 5)
        dt1 = torch.empty((N, C1, D, H, W), dtype=torch.float32, device=dout.device) if ctx.needs_input_grad[0] else None
        dt2 = torch.empty((N, C2, D2, H2, W2), dtype=torch.float32, device=dout.device) if ctx.needs_input_grad[1] else None
        call("dram_crop_concat_bwd", _p(dout), _p(dt1), _p(dt2), N, C1, C2, D, H, W, D2, H2, W2, oz, oy, ox, _stream())
        return dt1, dt2


def crop_concat(t1, t2):
    return CropConcatFn.apply(t1, t2)


# --------------------------------------------------------------------------- lobe-masked mean
class MaskedMeanFn(Function):
    """sum(x*m)/sum(m) per (n, c) (pooling_dense_features default branch, reference models.py:45-47)."""

    @staticmethod
    def forward(ctx, x, mask):
        x = _chk(x, "masked_mean input", 5)
        mask = _chk(mask, "masked_mean mask", 5)
        N, C = x.shape[:2]
        S = x.numel() // (N * C)
        if mask.shape[0] != N or mask.shape[1] != 1 or mask.numel() != N * S:
            raise ValueError(f"masked_mean: mask {tuple(mask.shape)} does not broadcast over {tuple(x.shape)}")
        out = torch.empty((N, C), dtype=torch.float32, device=x.device)
        msum = torch.empty(N, dtype=torch.float32, device=x.device)
        ws = _ws(_lib.lib.dram_masked_mean_ws_bytes(N, C, S), x.device)
        call("dram_masked_mean_fwd", _p(x), _p(mask), _p(out), _p(msum), _p(ws), ws.numel(), N, C, S, _stream())
        ctx.save_for_backward(mask, msum)
        ctx.shape = tuple(x.shape)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        mask, msum = ctx.saved_tensors
        dout = _chk(dout, "masked_mean grad_output", 2)
        N, C = ctx.shape[:2]
        S = mask.numel() // N
        dx = torch.empty(ctx.shape, dtype=torch.float32, device=dout.device)
        call("dram_masked_mean_bwd", _p(dout), _p(mask), _p(msum), _p(dx), N, C, S, _stream())
        return dx, None


def masked_mean(x, mask):
    return MaskedMeanFn.apply(x, mask)


# --------------------------------------------------------------------------- fused IntRegRefineLoss
class IntRegRefineLossFn(Function):
    """(reg_loss, seg_loss) of IntRegRefineLoss.__call__ (reference dram/metrics.py:360-373): one streaming
    pass for every sum, one for the gradient.  `refined` is the model's second output (None when the
    model returns the same tensor twice, as DC3D does)."""

    @staticmethod
    def forward(ctx, dense, refined, lobes, lesions, keep, targets, weight, smoothing):
        dense = _chk(dense, "loss dense", 5)
        lobes = _chk(lobes, "loss lobes", 5)
        lesions = _chk(lesions, "loss lesions", 5)
        if refined is not None:
            refined = _chk(refined, "loss refined", 5)
        N = dense.shape[0]
        S = dense.numel() // N
        if dense.shape[1] != 1 or lobes.shape != dense.shape or lesions.shape != dense.shape \
                or (refined is not None and refined.shape != dense.shape):
            raise ValueError("IntRegRefineLossFn: dense / refined / lobes / lesions must all be [N,1,D,H,W]")
        keep, targets, weight = _chk(keep, "loss keep").reshape(-1), _chk(targets, "loss targets"), _chk(weight, "loss weight")
        if keep.numel() != N or targets.numel() != 2 * N or weight.numel() != N:
            raise ValueError("IntRegRefineLossFn: keep[N], targets[N,2], weight[N] expected")
        dev = dense.device
        out = torch.empty(2, dtype=torch.float32, device=dev)
        state = torch.empty(_lib.lib.dram_intreg_loss_state_floats(N), dtype=torch.float32, device=dev)
        ws = _ws(_lib.lib.dram_intreg_loss_ws_bytes(N, S), dev)
        call("dram_intreg_loss_fwd", _p(dense), _p(refined), _p(lobes), _p(lesions), _p(keep), _p(targets), _p(weight),
             float(smoothing), _p(out), _p(state), _p(ws), ws.numel(), N, S, _stream())
        ctx.save_for_backward(dense, lobes, lesions, keep, targets, weight, state, *(() if refined is None else (refined,)))
        ctx.smoothing = float(smoothing)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        dense, lobes, lesions, keep, targets, weight, state, *rest = ctx.saved_tensors
        refined = rest[0] if rest else None
        gout = _chk(gout, "loss grad_output", 1)
        N = dense.shape[0]
        S = dense.numel() // N
        ddense = torch.empty_like(dense)
        drefined = torch.empty_like(refined) if refined is not None else None
        call("dram_intreg_loss_bwd", _p(dense), _p(refined), _p(lobes), _p(lesions), _p(keep), _p(targets), _p(weight),
             _p(state), _p(gout), ctx.smoothing, _p(ddense), _p(drefined), N, S, _stream())
        return ddense, drefined, None, None, None, None, None, None


def intreg_refine_loss(dense, lobes, lesions, keep, targets, weight, smoothing=0.1, refined=None):
    """Returns a [2] tensor: (reg_loss, seg_loss)."""
    if refined is dense:
        refined = None
    return IntRegRefineLossFn.apply(dense, refined, lobes, lesions, keep, targets, weight, smoothing)


class IntRegEncLossFn(Function):
    """(reg_loss, enc_loss) of IntRegLoss.__call__ (reference dram/metrics.py:204-210): the interval hinge of
    compute_reg_loss_with_probs (158-177) and the entropy term of compute_enc_loss (154-156) on one logit tensor, one
    streaming pass for the sums and one for the gradient.  `lesions` is part of the call because the loss is a function of
    it, but it acts through `targets` alone (the band Batch derives from the lesion ratio): the kernels read dense and lobes."""

    @staticmethod
    def forward(ctx, dense, lobes, lesions, targets, weight):
        dense = _chk(dense, "loss dense", 5)
        lobes = _chk(lobes, "loss lobes", 5)
        lesions = _chk(lesions, "loss lesions", 5)
        N = dense.shape[0]
        S = dense.numel() // N
        if dense.shape[1] != 1 or lobes.shape != dense.shape or lesions.shape != dense.shape:
            raise ValueError("IntRegEncLossFn: dense / lobes / lesions must all be [N,1,D,H,W]")
        targets, weight = _chk(targets, "loss targets"), _chk(weight, "loss weight")
        if targets.numel() != 2 * N or weight.numel() != N:
            raise ValueError("IntRegEncLossFn: targets[N,2], weight[N] expected")
        dev = dense.device
        out = torch.empty(2, dtype=torch.float32, device=dev)
        state = torch.empty(_lib.lib.dram_intreg_enc_loss_state_floats(N), dtype=torch.float32, device=dev)
        ws = _ws(_lib.lib.dram_intreg_enc_loss_ws_bytes(N, S), dev)
        call("dram_intreg_enc_loss_fwd", _p(dense), _p(lobes), _p(targets), _p(weight), _p(out), _p(state), _p(ws), ws.numel(),
             N, S, _stream())
        ctx.save_for_backward(dense, lobes, targets, weight, state)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        dense, lobes, targets, weight, state = ctx.saved_tensors
        gout = _chk(gout, "loss grad_output", 1)
        N = dense.shape[0]
        S = dense.numel() // N
        ddense = torch.empty_like(dense)
        call("dram_intreg_enc_loss_bwd", _p(dense), _p(lobes), _p(targets), _p(weight), _p(state), _p(gout), _p(ddense), N, S,
             _stream())
        return ddense, None, None, None, None


def intreg_enc_loss(dense, lobes, lesions, targets, weight):
    """Returns a [2] tensor: (reg_loss, enc_loss)."""
    return IntRegEncLossFn.apply(dense, lobes, lesions, targets, weight)


def intreg_targets(lobes, lesions, ctss, freq, band_width):
    """The regression band, class weight and pseudo-label switch of a batch without a host read (csrc/loss.hip,
    dram_intreg_targets): lobes, lesions [N,1,D,H,W] on the device, `ctss` an int32 device tensor of the N CT severity
    scores, `freq` the six class frequencies (a host sequence: they travel with the launch), `band_width` a float.
    Returns (targets[N,2], weight[N], keep[N]).  No gradient: the targets are data."""
    lobes, lesions = _chk(lobes.detach(), "targets lobes", 5), _chk(lesions.detach(), "targets lesions", 5)
    N = lobes.shape[0]
    S = lobes.numel() // max(N, 1)
    if lobes.shape[1] != 1 or lesions.shape != lobes.shape:
        raise ValueError("intreg_targets: lobes / lesions must both be [N,1,D,H,W]")
    if not isinstance(ctss, torch.Tensor) or not ctss.is_cuda or ctss.dtype != torch.int32 or ctss.numel() != N:
        raise TypeError("intreg_targets: ctss must be an int32 device tensor with one score per sample")
    if ctss.device != lobes.device or lesions.device != lobes.device:
        raise RuntimeError("intreg_targets: lobes, lesions and ctss must be on one device")
    freq = [float(f) for f in freq]
    if len(freq) != 6:
        raise ValueError("intreg_targets: six class frequencies expected")
    ctss = ctss.contiguous()
    dev = lobes.device
    targets = torch.empty((N, 2), dtype=torch.float32, device=dev)
    weight = torch.empty(N, dtype=torch.float32, device=dev)
    keep = torch.empty(N, dtype=torch.float32, device=dev)
    ws = _ws(_lib.lib.dram_intreg_targets_ws_bytes(N, S), dev)
    fr = (ctypes.c_float * 6)(*freq)
    call("dram_intreg_targets", _p(lobes), _p(lesions), _p(ctss), ctypes.cast(fr, ctypes.c_void_p), float(band_width),
         _p(targets), _p(weight), _p(keep), _p(ws), ws.numel(), N, S, _stream())
    return targets, weight, keep


class SigmoidFn(Function):
    """F.sigmoid as a differentiable device op (the affine-consistency term compares probabilities,
    reference dram/metrics.py:434,445)."""

    @staticmethod
    def forward(ctx, x):
        x = _chk(x, "sigmoid input")
        y = torch.empty_like(x)
        call("dram_sigmoid_fwd", _p(x), _p(y), x.numel(), _stream())
        ctx.save_for_backward(x)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = _chk(dy, "sigmoid grad_output")
        dx = torch.empty_like(x)
        call("dram_sigmoid_bwd", _p(dy), _p(x), _p(dx), x.numel(), _stream())
        return dx


def sigmoid(x):
    return SigmoidFn.apply(x)


class MaskedSmoothL1Fn(Function):
    """F.smooth_l1_loss(a[m > 0], b[m > 0]) with m [N,1,D,H,W] expanded over the channels of a, b [N,C,D,H,W]
    (reference dram/metrics.py:448-452)."""

    @staticmethod
    def forward(ctx, a, b, mask):
        a, b, mask = _chk(a, "smooth_l1 input", 5), _chk(b, "smooth_l1 target", 5), _chk(mask, "smooth_l1 mask", 5)
        N, C = a.shape[:2]
        S = a.numel() // (N * C)
        if b.shape != a.shape or mask.shape[0] != N or mask.shape[1] != 1 or mask.numel() != N * S:
            raise ValueError(f"masked smooth-L1: shapes {tuple(a.shape)}, {tuple(b.shape)}, mask {tuple(mask.shape)}")
        out = torch.empty(2, dtype=torch.float32, device=a.device)
        ws = _ws(_lib.lib.dram_masked_smooth_l1_ws_bytes(N, C, S), a.device)
        call("dram_masked_smooth_l1_fwd", _p(a), _p(b), _p(mask), _p(out), _p(ws), ws.numel(), N, C, S, _stream())
        ctx.save_for_backward(a, b, mask, out)
        return out[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        a, b, mask, out = ctx.saved_tensors
        N, C = a.shape[:2]
        S = a.numel() // (N * C)
        g = g.reshape(1).contiguous()
        da = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        db = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        if da is not None or db is not None:
            call("dram_masked_smooth_l1_bwd", _p(a), _p(b), _p(mask), _p(out), _p(g), _p(da), _p(db), N, C, S, _stream())
        return da, db, None


def masked_smooth_l1(a, b, mask):
    return MaskedSmoothL1Fn.apply(a, b, mask)


# --------------------------------------------------------------------------- segmentation losses with a given target
SEG_MASK_KINDS = {torch.uint8: 0, torch.float32: 2}     # DRAM_SEG_MASK_U8, DRAM_SEG_MASK_F32 (include/dram_hip.h)


def _seg_mask(t, name, like):
    """A target or volume-of-interest tensor of a segmentation loss: float32, uint8 or bool (read as uint8), on the device,
    of the probabilities' shape.  Returns (contiguous tensor, kind)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: tensor is on {t.device}; the DRAM HIP path only runs on a ROCm device "
                           f"(there is no CPU fallback)")
    if t.dtype == torch.bool:
        t = t.contiguous().view(torch.uint8)
    if t.dtype not in SEG_MASK_KINDS:
        raise TypeError(f"{name}: expected float32, uint8 or bool, got {t.dtype}")
    if t.shape != like.shape:
        raise ValueError(f"{name}: shape {tuple(t.shape)} differs from the probabilities' {tuple(like.shape)}")
    return t.contiguous(), SEG_MASK_KINDS[t.dtype]


def _seg_grad(g, name):
    g = _chk(g, name)
    if g.numel() != 1:
        raise ValueError(f"{name}: expected one element, got shape {tuple(g.shape)}")
    return g


def _seg_buffers(p):
    """(loss, state, workspace) of a segmentation-loss forward; the loss of no elements is NaN (nothing is launched then)."""
    n = p.numel()
    out = torch.full((), float("nan"), dtype=torch.float32, device=p.device) if n == 0 else \
        torch.empty((), dtype=torch.float32, device=p.device)
    state = torch.empty(_lib.lib.dram_seg_loss_state_floats(), dtype=torch.float32, device=p.device)
    ws = torch.empty(max(int(_lib.lib.dram_seg_loss_ws_bytes(n)) // 8, 8), dtype=torch.float64, device=p.device)
    return out, state, ws


def _boot_bce_launch(p, t, kt, voi, kv, smoothing):
    out, state, ws = _seg_buffers(p)
    call("dram_boot_bce_fwd", _p(p), _p(t), _p(voi), kt, kv, p.numel(), float(smoothing), _p(out), _p(state), _p(ws),
         ws.numel() * 8, _stream())
    return out, state, ws


def boot_bce_totals(p, t, voi):
    """The seven fp64 totals of a BootBinCrossEntropy forward, as the finish kernel leaves them at the head of the
    workspace: n_out, sum_out nll, n_in, T, A, B, sum_in nll_hat (a device tensor; for tests and diagnostics)."""
    p = _chk(p, "boot_bce p")
    (t, kt), (voi, kv) = _seg_mask(t, "boot_bce t", p), _seg_mask(voi, "boot_bce voi", p)
    return _boot_bce_launch(p, t, kt, voi, kv, 0.0)[2][:7]


class BootBCEFn(Function):
    """BootBinCrossEntropy.__call__ (reference dram/metrics.py:17-51) for a target that is given: one streaming pass for
    every sum, a one-block finish that takes the reference's `tf.sum() > 0` branch on the device, one streaming pass for the
    gradient.  Nothing is read back in either direction.  An empty tensor gives NaN, as the reference's mean of nothing."""

    @staticmethod
    def forward(ctx, p, t, voi, smoothing):
        p = _chk(p, "boot_bce p")
        t, kt = _seg_mask(t, "boot_bce t", p)
        voi, kv = _seg_mask(voi, "boot_bce voi", p)
        out, state, _ = _boot_bce_launch(p, t, kt, voi, kv, smoothing)
        ctx.save_for_backward(p, t, voi, state)
        ctx.kinds, ctx.smoothing = (kt, kv), float(smoothing)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        p, t, voi, state = ctx.saved_tensors
        g = _seg_grad(g, "boot_bce grad_output")
        dp = torch.empty_like(p)
        call("dram_boot_bce_bwd", _p(p), _p(t), _p(voi), *ctx.kinds, p.numel(), ctx.smoothing, _p(state), _p(g), _p(dp),
             _stream())
        return dp, None, None, None


def boot_bce(p, t, voi, smoothing=0.1):
    """BootBinCrossEntropy(smoothing)(p, t, voi) as a 0-dim tensor; t and voi float32, uint8 or bool."""
    return BootBCEFn.apply(p, t, voi, smoothing)


def _bce_smooth_launch(p, t, kt, smooth):
    out, state, ws = _seg_buffers(p)
    call("dram_bce_smooth_fwd", _p(p), _p(t), kt, p.numel(), float(smooth), _p(out), _p(state), _p(ws), ws.numel() * 8,
         _stream())
    return out, state, ws


def bce_smooth_totals(p, t):
    """The three fp64 totals of a BinaryCrossEntropySmooth forward: T, sum t log pc, sum (1 - t) log(1 - pc)."""
    p = _chk(p, "bce_smooth probs")
    t, kt = _seg_mask(t, "bce_smooth targets", p)
    return _bce_smooth_launch(p, t, kt, 1.0)[2][:3]


class BCESmoothFn(Function):
    """BinaryCrossEntropySmooth.__call__ (reference dram/metrics.py:60-72): the same three launches."""

    @staticmethod
    def forward(ctx, p, t, smooth):
        p = _chk(p, "bce_smooth probs")
        t, kt = _seg_mask(t, "bce_smooth targets", p)
        out, state, _ = _bce_smooth_launch(p, t, kt, smooth)
        ctx.save_for_backward(p, t, state)
        ctx.kind, ctx.smooth = kt, float(smooth)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        p, t, state = ctx.saved_tensors
        g = _seg_grad(g, "bce_smooth grad_output")
        dp = torch.empty_like(p)
        call("dram_bce_smooth_bwd", _p(p), _p(t), ctx.kind, p.numel(), ctx.smooth, _p(state), _p(g), _p(dp), _stream())
        return dp, None, None


def bce_smooth(p, t, smooth):
    """BinaryCrossEntropySmooth(smooth)(p, t) as a 0-dim tensor; t float32, uint8 or bool."""
    return BCESmoothFn.apply(p, t, smooth)


def _seg_overlap_args(logits, target, voi):
    """The checked tensors of a SegOverlap call: (z, t, t kind, voi or None, voi kind, N, S).  The first dimension is the
    sample; a 5-d tensor is [N,1,D,H,W]."""
    z = _chk(logits, "seg_overlap logits")
    if z.dim() < 1 or (z.dim() == 5 and z.shape[1] != 1):
        raise ValueError(f"seg_overlap logits: expected [N, ...] with one channel, got shape {tuple(z.shape)}")
    t, kt = _seg_mask(target, "seg_overlap target", z)
    voi, kv = (None, 0) if voi is None else _seg_mask(voi, "seg_overlap voi", z)
    N = z.shape[0]
    return z, t, kt, voi, kv, N, (z.numel() // N if N else 0)


def _seg_overlap_launch(z, t, kt, voi, kv, N, S, a, b, smooth, alpha, gamma):
    """(out[2], state, fp64 workspace) of a SegOverlap forward; a batch of no elements is (0, 0), nothing is launched."""
    dev = z.device
    out = torch.zeros(2, dtype=torch.float32, device=dev) if N * S == 0 else torch.empty(2, dtype=torch.float32, device=dev)
    state = torch.empty(max(_lib.lib.dram_seg_overlap_state_floats(N), 1), dtype=torch.float32, device=dev)
    ws = torch.empty(max(int(_lib.lib.dram_seg_overlap_ws_bytes(N, S)) // 8, 8), dtype=torch.float64, device=dev)
    call("dram_seg_overlap_fwd", _p(z), _p(t), _p(voi), kt, kv, N, S, float(a), float(b), float(smooth), float(alpha),
         float(gamma), _p(out), _p(state), _p(ws), ws.numel() * 8, _stream())
    return out, state, ws


def seg_overlap_totals(logits, target, voi=None, alpha=.5, gamma=2.0):
    """The fp64 per-sample totals of a SegOverlap forward as the finish kernel leaves them at the head of the workspace, an
    [N, 5] device tensor: TP, SP, ST, M and the sum of the focal terms (for tests and diagnostics)."""
    z, t, kt, voi, kv, N, S = _seg_overlap_args(logits.detach(), target, voi)
    ws = _seg_overlap_launch(z, t, kt, voi, kv, N, S, .5, .5, 1.0, alpha, gamma)[2]
    return ws[:8 * N].view(N, 8)[:, :5] if N * S else torch.zeros((N, 5), dtype=torch.float64, device=z.device)


class SegOverlapFn(Function):
    """(sum_n (1 - TI_n), mean_n F_n): the per-sample Tversky and focal terms of include/dram_hip.h (SegOverlap) on logits
    and a given target.  One streaming pass and a one-block finish forward, one streaming pass backward; what is saved is
    z, t, voi and five floats per sample -- no per-voxel intermediate -- and nothing is read back."""

    @staticmethod
    def forward(ctx, logits, target, voi, a, b, smooth, alpha, gamma):
        z, t, kt, voi, kv, N, S = _seg_overlap_args(logits, target, voi)
        out, state, _ = _seg_overlap_launch(z, t, kt, voi, kv, N, S, a, b, smooth, alpha, gamma)
        ctx.save_for_backward(z, t, state, *(() if voi is None else (voi,)))
        ctx.args = (kt, kv, N, S, float(alpha), float(gamma))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        z, t, state, *rest = ctx.saved_tensors
        voi = rest[0] if rest else None
        gout = _chk(gout, "seg_overlap grad_output", 1)
        if gout.numel() != 2:
            raise ValueError(f"seg_overlap grad_output: expected two elements, got shape {tuple(gout.shape)}")
        kt, kv, N, S, alpha, gamma = ctx.args
        dz = torch.empty_like(z)
        call("dram_seg_overlap_bwd", _p(z), _p(t), _p(voi), kt, kv, N, S, alpha, gamma, _p(state), _p(gout), _p(dz), _stream())
        return dz, None, None, None, None, None, None, None


def seg_overlap(logits, target, voi=None, a=.5, b=.5, smooth=1.0, alpha=.5, gamma=2.0):
    """Returns a [2] tensor: (sum over samples of 1 - Tversky index, mean over samples of the focal term) of the logits
    [N,1,D,H,W] against `target` inside `voi` (float32, uint8 or bool of the logits' shape; voi None: every voxel)."""
    return SegOverlapFn.apply(logits, target, voi, a, b, smooth, alpha, gamma)


# --------------------------------------------------------------------------- PCM local attention
PCM_RELU, PCM_L2NORM = 1, 2
# merge_type -> (flags, scale_mode); reference models.py:259-331 (dot-product family)
PCM_MERGE_MODES = {
    "sm": (0, 0), "scaled_dot_product": (0, 1), "scaled_dot_product_relu": (PCM_RELU, 1), "smrelu": (PCM_RELU, 0),
    "smscaled": (0, 2), "l2sm": (PCM_L2NORM, 0), "l2smrelu": (PCM_RELU | PCM_L2NORM, 0),
}


PCM_MAX_OFFSETS = 128      # the kernels' neighbour-offset table (PCM_MAXE, csrc/pcm.hip)


def _offsets_arg(offsets):
    if not 0 < len(offsets) <= PCM_MAX_OFFSETS:
        raise ValueError(f"PCM: {len(offsets)} neighbour offsets; the device kernels take 1..{PCM_MAX_OFFSETS}")
    flat = [int(v) for o in offsets for v in o]
    return (ctypes.c_int * len(flat))(*flat), len(flat) // 3


class PcmAttentionFn(Function):
    """attn[b,e,i] = softmax over node i's in-grid neighbours e of the merged theta_i . phi_(i+o_e)
    (reference models.py: merge_func 259-331 inside compute_cross_x 365-397)."""

    @staticmethod
    def forward(ctx, theta, phi, offsets, flags, scale_mode, f_relu=None):
        theta, phi = _chk(theta, "pcm theta", 5), _chk(phi, "pcm phi", 5)
        if theta.shape != phi.shape:
            raise ValueError(f"pcm attention: theta {tuple(theta.shape)} and phi {tuple(phi.shape)} differ")
        B, Fd, D, H, W = theta.shape
        f_relu = Fd if f_relu is None else int(f_relu)      # feature planes inside the activation (the rest is added raw)
        arr, E = _offsets_arg(offsets)
        attn = torch.empty((B, E, D, H, W), dtype=torch.float32, device=theta.device)
        call("dram_pcm_attention_split_fwd", _p(theta), _p(phi), arr, E, flags, scale_mode, f_relu, _p(attn), B, Fd, D, H, W,
             _stream())
        ctx.save_for_backward(theta, phi, attn)
        ctx.cfg = (offsets, flags, scale_mode, f_relu)
        return attn

    @staticmethod
    @once_differentiable
    def backward(ctx, dattn):
        theta, phi, attn = ctx.saved_tensors
        offsets, flags, scale_mode, f_relu = ctx.cfg
        dattn = _chk(dattn, "pcm attention grad_output", 5)
        B, Fd, D, H, W = theta.shape
        arr, E = _offsets_arg(offsets)
        ds = torch.empty_like(attn)
        ds2 = torch.empty_like(attn) if (f_relu < Fd and (flags & PCM_RELU)) else None
        dtheta, dphi = torch.empty_like(theta), torch.empty_like(phi)
        call("dram_pcm_attention_split_bwd", _p(theta), _p(phi), _p(attn), _p(dattn), arr, E, flags, scale_mode, f_relu, _p(ds),
             _p(ds2), _p(dtheta), _p(dphi), B, Fd, D, H, W, _stream())
        return dtheta, dphi, None, None, None, None


# merge types normalised by the sum over a node's edges instead of a softmax (reference models.py:300-302, 307-320)
PCM_SUM_MERGES = {"cosine": 0, "heu1": 1, "heu2": 2}


class PcmAttentionSumFn(Function):
    """attn[b,e,i] = v_e / (eps + sum_k v_k) over node i's in-grid neighbours with v = the cosine similarity of
    (theta_i, phi_(i+o_e)) / the heuristic similarity theta.phi / (1 + |theta - phi|_1), masked below 0.03 (heu1: formed
    under no_grad in the reference, so that attention carries no gradient at all) or rectified (heu2)."""

    @staticmethod
    def forward(ctx, theta, phi, offsets, mode):
        theta, phi = _chk(theta, "pcm theta", 5), _chk(phi, "pcm phi", 5)
        if theta.shape != phi.shape:
            raise ValueError(f"pcm attention: theta {tuple(theta.shape)} and phi {tuple(phi.shape)} differ")
        B, Fd, D, H, W = theta.shape
        arr, E = _offsets_arg(offsets)
        attn = torch.empty((B, E, D, H, W), dtype=torch.float32, device=theta.device)
        call("dram_pcm_attention_sum_fwd", _p(theta), _p(phi), arr, E, mode, _p(attn), B, Fd, D, H, W, _stream())
        ctx.save_for_backward(theta, phi, attn)
        ctx.cfg = (offsets, mode)
        return attn

    @staticmethod
    @once_differentiable
    def backward(ctx, dattn):
        theta, phi, attn = ctx.saved_tensors
        offsets, mode = ctx.cfg
        if mode == PCM_SUM_MERGES["heu1"]:
            # reference models.py:311-314: `f = f * mask_f` sits inside `with torch.no_grad():`, so the masked similarities --
            # and the whole heu1 attention -- are constants of the graph: no gradient reaches theta or phi
            return None, None, None, None
        dattn = _chk(dattn, "pcm attention grad_output", 5)
        B, Fd, D, H, W = theta.shape
        arr, E = _offsets_arg(offsets)
        ds = torch.empty_like(attn)
        dtheta, dphi = torch.empty_like(theta), torch.empty_like(phi)
        call("dram_pcm_attention_sum_bwd", _p(theta), _p(phi), _p(attn), _p(dattn), arr, E, mode, _p(ds), _p(dtheta), _p(dphi),
             B, Fd, D, H, W, _stream())
        return dtheta, dphi, None, None


class PcmAggregateFn(Function):
    """out[b,c,i] = sum_e attn[b,e,i] * v[b,c,i+o_e]  (torch.matmul(f_sm, x_g), reference models.py:394)."""

    @staticmethod
    def forward(ctx, attn, v, offsets):
        attn, v = _chk(attn, "pcm attn", 5), _chk(v, "pcm values", 5)
        B, C, D, H, W = v.shape
        arr, E = _offsets_arg(offsets)
        if tuple(attn.shape) != (B, E, D, H, W):
            raise ValueError(f"pcm aggregate: attn {tuple(attn.shape)} does not match values {tuple(v.shape)} x {E} offsets")
        out = torch.empty_like(v)
        call("dram_pcm_aggregate_fwd", _p(attn), _p(v), arr, E, _p(out), B, C, D, H, W, _stream())
        ctx.save_for_backward(attn, v)
        ctx.offsets = offsets
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        attn, v = ctx.saved_tensors
        dout = _chk(dout, "pcm aggregate grad_output", 5)
        B, C, D, H, W = v.shape
        arr, E = _offsets_arg(ctx.offsets)
        dattn, dv = torch.empty_like(attn), torch.empty_like(v)
        call("dram_pcm_aggregate_bwd", _p(attn), _p(v), _p(dout), arr, E, _p(dattn), _p(dv), B, C, D, H, W, _stream())
        return dattn, dv, None


# merge types with a positional-encoding term (reference models.py:287-299): the same kernels on combined feature planes
PCM_GEO_MERGES = ("scaled_dot_product_geo", "scaled_dot_product_geo_relu", "att_is_all")


def pcm_attention(theta, phi, offsets, merge_type, geo_theta=None, geo_phi=None):
    """merge_func (reference models.py:259-331) on the voxel grid.  geo_theta / geo_phi: the projected positional
    encodings [B, geo_f_dim, D, H, W] that the geo merge types add to the appearance term."""
    offsets = tuple(map(tuple, offsets))
    if merge_type in PCM_GEO_MERGES:
        if geo_theta is None or geo_phi is None:
            raise ValueError(f"PCM merge_type {merge_type!r} needs the positional encodings (p_enc_dim > 0)")
        if merge_type == "att_is_all":                  # (theta + geo_theta) . (phi + geo_phi), models.py:297-299
            if theta.shape != geo_theta.shape:
                raise ValueError(f"att_is_all: f_dim {theta.shape[1]} and geo_f_dim {geo_theta.shape[1]} must agree")
            return PcmAttentionFn.apply(theta + geo_theta, phi + geo_phi, offsets, 0, 1)
        th, ph = torch.cat([theta, geo_theta], 1), torch.cat([phi, geo_phi], 1)
        if merge_type == "scaled_dot_product_geo":      # theta.phi + geo_theta.geo_phi: one dot over the stacked planes
            return PcmAttentionFn.apply(th, ph, offsets, 0, 1)
        return PcmAttentionFn.apply(th, ph, offsets, PCM_RELU, 1, theta.shape[1])     # relu(theta.phi) + geo_theta.geo_phi
    if merge_type in PCM_SUM_MERGES:
        return PcmAttentionSumFn.apply(theta, phi, offsets, PCM_SUM_MERGES[merge_type])
    if merge_type == "l2":
        # models.py:262-264: f = exp(-5 (theta - phi)^2), f / f.sum over the edges.  The reference subtracts [.., 1, f_dim] and
        # [.., f_dim, edges] tensors and later reshapes the aggregate to one row per node (models.py:396): both only work for
        # f_dim == 1.  There it is a softmax over the edges of -5 (theta - phi_e)^2 = -5 theta^2 + 10 theta phi_e - 5 phi_e^2,
        # whose first term is common to a node's edges and cancels: the 'sm' kernel on the feature pairs
        # (10 theta, -5) . (phi, phi^2).
        if theta.shape[1] != 1:
            raise ValueError(f"PCM merge_type 'l2' is only defined for f_dim == 1 (got {theta.shape[1]}): the reference "
                             f"broadcasts [.., 1, f_dim] against [.., f_dim, edges] (models.py:263)")
        th2 = torch.cat([10.0 * theta, torch.full_like(theta, -5.0)], 1)
        ph2 = torch.cat([phi, phi * phi], 1)
        return PcmAttentionFn.apply(th2, ph2, offsets, 0, 0)
    if merge_type not in PCM_MERGE_MODES:
        raise NotImplementedError(f"PCM merge_type {merge_type!r}: the dot-product family {sorted(PCM_MERGE_MODES)}, the "
                                  f"geo family {list(PCM_GEO_MERGES)}, {sorted(PCM_SUM_MERGES)} and 'l2' are implemented on the device")
    flags, scale_mode = PCM_MERGE_MODES[merge_type]
    return PcmAttentionFn.apply(theta, phi, offsets, flags, scale_mode)


def pcm_aggregate(attn, v, offsets):
    return PcmAggregateFn.apply(attn, v, tuple(map(tuple, offsets)))


# --------------------------------------------------------------------------- OneShot transforms
class ResizeTrilinearFn(Function):
    """F.interpolate(x, size / scale_factor, mode='trilinear') with align_corners=False
    (Rescale3DOneShot on "#image" tensors, reference data_transforms.py:1202-1239)."""

    @staticmethod
    def forward(ctx, x, size, scales):
        x = _chk(x, "resize input", 5)
        N, C, D, H, W = x.shape
        Do, Ho, Wo = (int(v) for v in size)
        y = torch.empty((N, C, Do, Ho, Wo), dtype=torch.float32, device=x.device)
        call("dram_resize_trilinear_fwd", _p(x), _p(y), N, C, D, H, W, Do, Ho, Wo, *scales, _stream())
        ctx.geom = (N, C, D, H, W, Do, Ho, Wo, scales)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        N, C, D, H, W, Do, Ho, Wo, scales = ctx.geom
        dy = _chk(dy, "resize grad_output", 5)
        dx = torch.empty((N, C, D, H, W), dtype=torch.float32, device=dy.device)
        call("dram_resize_trilinear_bwd", _p(dy), _p(dx), N, C, D, H, W, Do, Ho, Wo, *scales, _stream())
        return dx, None, None


def _resize_geometry(x, size, scale_factor):
    """Output size and the per-axis source scale ATen uses (0 = the default in/out)."""
    if (size is None) == (scale_factor is None):
        raise ValueError("only one of size or scale_factor should be defined")
    if size is not None:
        size = tuple(int(v) for v in (size if isinstance(size, (tuple, list, torch.Size)) else (size,) * 3))
        return size, (0.0, 0.0, 0.0)
    sf = tuple(float(v) for v in (scale_factor if isinstance(scale_factor, (tuple, list)) else (scale_factor,) * 3))
    size = tuple(int(math.floor(float(d) * s)) for d, s in zip(x.shape[2:], sf))
    return size, tuple(1.0 / s for s in sf)      # recompute_scale_factor=None: the given factor maps coordinates


def interpolate_trilinear(x, size=None, scale_factor=None):
    size, scales = _resize_geometry(x, size, scale_factor)
    return ResizeTrilinearFn.apply(x, size, scales)


def interpolate_nearest(x, size=None, scale_factor=None):
    """F.interpolate(mode='nearest'); label maps: no gradient."""
    size, scales = _resize_geometry(x, size, scale_factor)
    xc = _chk(x.detach(), "nearest input", 5)
    N, C, D, H, W = xc.shape
    y = torch.empty((N, C) + size, dtype=torch.float32, device=xc.device)
    call("dram_resize_nearest", _p(xc), _p(y), N, C, D, H, W, *size, *scales, _stream())
    return y


class AffineSampleFn(Function):
    """F.grid_sample(x, F.affine_grid(theta, x.size())) for one [3,4] theta shared by the batch
    (Rotate3DXOneShot, reference data_transforms.py:1186-1208)."""

    @staticmethod
    def forward(ctx, x, theta):
        x = _chk(x, "affine sample input", 5)
        N, C, D, H, W = x.shape
        arr = (ctypes.c_float * 12)(*[float(v) for v in theta])
        y = torch.empty_like(x)
        call("dram_affine_sample_fwd", _p(x), _p(y), arr, N, C, D, H, W, _stream())
        ctx.theta = tuple(float(v) for v in theta)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        dy = _chk(dy, "affine sample grad_output", 5)
        N, C, D, H, W = dy.shape
        arr = (ctypes.c_float * 12)(*ctx.theta)
        dx = torch.empty_like(dy)
        call("dram_affine_sample_bwd", _p(dy), _p(dx), arr, N, C, D, H, W, _stream())
        return dx, None


def affine_sample(x, theta12):
    return AffineSampleFn.apply(x, tuple(theta12))


class SpatialPermuteFlipFn(Function):
    """A signed permutation of the spatial axes of [N,C,D,H,W] (torch.flip / torch.rot90 / transpose chains)."""

    @staticmethod
    def forward(ctx, x, perm, flip):
        x = _chk(x, "permute/flip input", 5)
        N, C, D, H, W = x.shape
        ind = (D, H, W)
        y = torch.empty((N, C) + tuple(ind[p] for p in perm), dtype=torch.float32, device=x.device)
        call("dram_spatial_permute_flip", _p(x), _p(y), N, C, D, H, W, (ctypes.c_int * 3)(*perm), (ctypes.c_int * 3)(*flip),
             _stream())
        ctx.pf = (perm, flip)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        perm, flip = ctx.pf
        dy = _chk(dy, "permute/flip grad_output", 5)
        inv_perm, inv_flip = [0, 0, 0], [0, 0, 0]
        for k in range(3):                      # output axis k came from input axis perm[k] (flipped or not)
            inv_perm[perm[k]], inv_flip[perm[k]] = k, flip[k]
        N, C, D, H, W = dy.shape
        ind = (D, H, W)
        dx = torch.empty((N, C) + tuple(ind[p] for p in inv_perm), dtype=torch.float32, device=dy.device)
        call("dram_spatial_permute_flip", _p(dy), _p(dx), N, C, D, H, W, (ctypes.c_int * 3)(*inv_perm),
             (ctypes.c_int * 3)(*inv_flip), _stream())
        return dx, None, None


def signed_permutation(ops):
    """Compose torch-style ops on the spatial axes into (perm, flip): ("flip", dims) and ("transpose", a, b)
    with dims in 5-D numbering (2, 3, 4), applied in order."""
    perm, flip = [0, 1, 2], [0, 0, 0]
    for op in ops:
        if op[0] == "flip":
            for d in op[1]:
                flip[d - 2] ^= 1
        else:
            a, b = op[1] - 2, op[2] - 2
            perm[a], perm[b] = perm[b], perm[a]
            flip[a], flip[b] = flip[b], flip[a]
    return tuple(perm), tuple(flip)


def rot90_ops(k, dims):
    """torch.rot90(x, k, dims) as flips and a transpose."""
    a, b = dims
    k %= 4
    if k == 0:
        return []
    if k == 1:
        return [("flip", (b,)), ("transpose", a, b)]
    if k == 2:
        return [("flip", (a, b))]
    return [("flip", (a,)), ("transpose", a, b)]


def spatial_permute_flip(x, perm, flip):
    if tuple(perm) == (0, 1, 2) and not any(flip):
        return x
    return SpatialPermuteFlipFn.apply(x, tuple(perm), tuple(flip))
