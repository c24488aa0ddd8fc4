"""Device optimisers: `Adam`, `AdamW`, `SGD`, `RAdam` and `AdaBound` whose update is one HIP launch per parameter group
(csrc/optim.hip) in place of ATen's dozen foreach launches over every tensor of the group.

The reference trains with `torch.optim.Adam(lr=1e-4)` under `ExponentialLR(gamma=0.9)` (st_dram_ref.py; an SGD-with-momentum
block is commented out beside it) and `job_runner.py` saves and reloads `optimizer.state_dict()` with every checkpoint.  The
classes here derive from torch's own and replace `step()` alone: constructor arguments, their validation, `param_groups`, the
per-parameter state (keys, dtypes, devices; `step` stays torch's fp32 scalar on the host) and so `state_dict()` /
`load_state_dict()` are torch's, and a checkpoint written by either loads into the other.  `lr` is read from `param_groups`
at every step, so LR schedulers work unchanged.  `RAdam` (the settings file's engine.models.optimizer.RAdam line) derives
from torch.optim.RAdam in the same way.  `AdaBound` (its adabound.AdaBound line) has no torch counterpart: it is a
torch.optim.Optimizer with the constructor, state keys and arithmetic of the `adabound` package.

`step()` builds a host table of (p, grad, exp_avg, exp_avg_sq[, max_exp_avg_sq]) pointers and the per-parameter bias
corrections -- the gradient pointers change every step under `zero_grad(set_to_none=True)` -- and hands it to
`dram_optim_adam` / `dram_optim_sgd` / `dram_optim_radam` / `dram_optim_adabound` in chunks of `TABLE_CAPACITY` tensors,
on the current stream.  It never synchronises with the device and reads no device value; the table travels in the kernel arguments, so there is no buffer to copy or keep
alive.  (A captured graph would replay one step's pointers and bias corrections: graph-captured steps are not supported.)
Like every op of this package there is no fallback: parameters and gradients must be dense fp32 on a ROCm device.

Global-norm gradient clipping runs on the same tables.  `clip_grad_norm_` is torch.nn.utils.clip_grad_norm_ (2-norm and
inf-norm) as a norm launch per table, one finishing block and an in-place scale per table.  `set_grad_clip` on an optimiser
folds the clipping into `step()`: the norm over the gradients of all groups, the finishing block, and the update kernels
multiply the coefficient -- a device scalar -- into every gradient element as they read it, so the gradients are neither
read nor written a second time.  Neither reads a device value on the host.
"""
import math
import struct

import torch

from ._lib import call, lib

__all__ = ["Adam", "AdamW", "SGD", "RAdam", "AdaBound", "TABLE_CAPACITY", "clip_grad_norm_"]

TABLE_CAPACITY = int(lib.dram_optim_table_capacity())   # tensors per launch (the table is a kernel argument)

_ENTRY = struct.Struct("@5Pqff")                        # dram_optim_tensor of include/dram_hip.h
assert _ENTRY.size == 56


def _no_tensor_lr(lr):
    if isinstance(lr, torch.Tensor):
        raise TypeError("dram_amd.optim: lr must be a Python number, got a tensor (a tensor lr lives on the device and "
                        "step() reads no device value)")


def _chk_param(p, name):
    """The parameter and its gradient as the kernel needs them (the style of functional._chk); returns the gradient,
    made contiguous."""
    g = p.grad
    if not p.is_cuda:
        raise RuntimeError(f"{name}: parameter is on {p.device}; the DRAM HIP path only runs on a ROCm device "
                           f"(there is no CPU fallback)")
    if g.is_sparse:
        raise RuntimeError(f"{name}: sparse gradients are not supported")
    if p.dtype != torch.float32 or g.dtype != torch.float32:
        raise TypeError(f"{name}: expected float32 parameter and gradient, got {p.dtype} and {g.dtype}")
    if g.device != p.device:
        raise RuntimeError(f"{name}: gradient is on {g.device}, parameter on {p.device}")
    if not p.is_contiguous():
        raise ValueError(f"{name}: parameter of shape {tuple(p.shape)} is not contiguous (it is updated in place)")
    return g.contiguous()


def _with_grad(group, name):
    """(parameter, contiguous gradient) of the group's parameters that have one, all checked before any state changes; a
    parameter whose .grad is None is skipped as torch skips it (its step count does not advance)."""
    return [(p, _chk_param(p, name)) for p in group["params"] if p.grad is not None]


def _chk_state(t, p, name):
    if t.dtype != torch.float32 or t.device != p.device or t.shape != p.shape or not t.is_contiguous():
        raise RuntimeError(f"{name}: state tensor {tuple(t.shape)} {t.dtype} on {t.device} does not match its parameter "
                           f"{tuple(p.shape)} {p.dtype} on {p.device}")
    return t


def _host_step(state, name):
    s = state["step"]
    if not torch.is_tensor(s):
        s = state["step"] = torch.tensor(float(s), dtype=torch.float32)
    if s.is_cuda:
        raise RuntimeError(f"{name}: the step count is a device tensor (capturable or fused state); reload the state "
                           f"through load_state_dict, which moves it to the host")
    return s


def _launch(entry, rows, *scalars, gscale=None):
    """rows: (device, p, g, m, v, vmax, s0, s1) with tensors or None; one launch per device and TABLE_CAPACITY rows.
    The rows' tensors stay referenced by the caller's lists until the launches are issued.  gscale: None, or the one-element
    device tensor every gradient is multiplied by as it is read (the `_scaled` entry points)."""
    by_dev = {}
    for r in rows:
        if r[1].numel() > 0:
            by_dev.setdefault(r[0], []).append(r)
    for dev, rs in by_dev.items():
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            for lo in range(0, len(rs), TABLE_CAPACITY):
                part = rs[lo:lo + TABLE_CAPACITY]
                buf = bytearray(_ENTRY.size * len(part))
                for i, (_, p, g, m, v, vmax, s0, s1) in enumerate(part):
                    _ENTRY.pack_into(buf, i * _ENTRY.size, p.data_ptr(), g.data_ptr(), 0 if m is None else m.data_ptr(),
                                     0 if v is None else v.data_ptr(), 0 if vmax is None else vmax.data_ptr(), p.numel(),
                                     s0, s1)
                if gscale is None:
                    call(entry, bytes(buf), len(part), *scalars, stream)
                else:
                    call(entry + "_scaled", bytes(buf), len(part), *scalars, gscale.data_ptr(), stream)


_NORM_KINDS = {2.0: 2, math.inf: 0}                     # DRAM_OPTIM_NORM_2, DRAM_OPTIM_NORM_INF of include/dram_hip.h


def _norm_kind(norm_type):
    kind = _NORM_KINDS.get(float(norm_type))
    if kind is None:
        raise NotImplementedError(f"dram_amd.optim: norm_type={norm_type!r}; the device gradient norm supports 2.0 and inf")
    return kind


def _grad_tables(grads):
    """The host tables (bytes, tensor count) over `grads`, TABLE_CAPACITY tensors each: only g and n are filled in."""
    tables = []
    for lo in range(0, len(grads), TABLE_CAPACITY):
        part = grads[lo:lo + TABLE_CAPACITY]
        buf = bytearray(_ENTRY.size * len(part))
        for i, g in enumerate(part):
            _ENTRY.pack_into(buf, i * _ENTRY.size, 0, g.data_ptr(), 0, 0, 0, g.numel(), 0.0, 0.0)
        tables.append((bytes(buf), len(part)))
    return tables


def _one_device(grads, name):
    devs = {g.device for g in grads}
    if len(devs) > 1:
        raise NotImplementedError(f"{name}: gradients on {len(devs)} devices ({', '.join(sorted(map(str, devs)))}); the global "
                                  f"norm is computed on one device")
    return next(iter(devs))


def _grad_norm(grads, tables, kind, max_norm):
    """The norm launches and the finish over non-empty contiguous fp32 gradients on one device (the current stream); returns
    the device tensor [total_norm, clip_coef]."""
    dev = grads[0].device
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        counts = [int(lib.dram_optim_grad_norm_partials(buf, n)) for buf, n in tables]
        partials = torch.empty(sum(counts), dtype=torch.float64, device=dev)
        out = torch.empty(2, dtype=torch.float32, device=dev)
        off = 0
        for (buf, n), c in zip(tables, counts):
            call("dram_optim_grad_norm", buf, n, kind, partials.data_ptr(), off, stream)
            off += c
        call("dram_optim_grad_norm_finish", partials.data_ptr(), off, kind, float(max_norm), out.data_ptr(), stream)
    return out


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """torch.nn.utils.clip_grad_norm_ on csrc/optim.hip: the gradients of `parameters` are scaled in place by
    min(1, max_norm / (total_norm + 1e-6)) and the norm before clipping comes back as a 0-dim fp32 device tensor.  norm_type
    2.0 or inf.  Nothing is read back to the host unless error_if_nonfinite, which reads the norm and raises torch's
    RuntimeError before any gradient is scaled.  `foreach` is accepted and ignored.  Parameters without a gradient and empty
    tensors are skipped; without any gradient the result is a zero tensor."""
    name = "dram_amd.optim.clip_grad_norm_"
    kind = _norm_kind(norm_type)
    max_norm = float(max_norm)
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    pairs = [(p, _chk_param(p, name)) for p in parameters if p.grad is not None]
    pairs = [(p, g) for p, g in pairs if g.numel() > 0]
    if not pairs:
        return torch.tensor(0.0)
    grads = [g for _, g in pairs]
    dev = _one_device(grads, name)
    tables = _grad_tables(grads)
    out = _grad_norm(grads, tables, kind, max_norm)
    if error_if_nonfinite and not math.isfinite(float(out[0])):
        raise RuntimeError(f"The total norm of order {float(norm_type)} for gradients from `parameters` is non-finite, so it "
                           f"cannot be clipped. To disable this error and scale the gradients by the non-finite norm anyway, "
                           f"set `error_if_nonfinite=False`")
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        for buf, n in tables:
            call("dram_optim_grad_scale", buf, n, out.data_ptr() + 4, stream)
    for p, g in pairs:
        if g.data_ptr() != p.grad.data_ptr():          # _chk_param made a contiguous copy: the scaled values go back
            p.grad.copy_(g)
    return out[0]


class _GradClip:
    """set_grad_clip() of the optimisers below: global-norm clipping inside step()."""

    _clip = None                                       # (max_norm, norm kind) or None; not part of state_dict()
    last_grad_norm = None                              # 0-dim device tensor: the norm before clipping at the last clipped step
    last_clip_coef = None                              # ... and the coefficient that step multiplied into the gradients

    def set_grad_clip(self, max_norm, norm_type=2.0):
        """Clip the global gradient norm (over all parameter groups together, what clip_grad_norm_(model.parameters(),
        max_norm, norm_type) sees) inside every later step(); None turns it off, which is the default.  The clipped step
        computes what clip_grad_norm_ followed by step() computes, bit for bit, with ONE difference: `.grad` is left
        unscaled (the coefficient is multiplied into each gradient element as the update kernel reads it).  The norm before
        clipping is `last_grad_norm` after the step and the coefficient `last_clip_coef`, both 0-dim device tensors that
        nothing reads on the host.  An attribute of this object, not a param_groups key and not in
        state_dict(): checkpoints stay torch's."""
        self._clip = None if max_norm is None else (float(max_norm), _norm_kind(norm_type))

    def _clip_pairs(self, name):
        """Clipping off: (None, None).  On: every group's (parameter, gradient) pairs, all checked, and the one-element
        device tensor of the clip coefficient (None without any gradient)."""
        if self._clip is None:
            return None, None
        for group in self.param_groups:
            _no_tensor_lr(group["lr"])
        pairs = [_with_grad(group, name) for group in self.param_groups]
        grads = [g for ps in pairs for _, g in ps if g.numel() > 0]
        if not grads:
            self.last_grad_norm, self.last_clip_coef = torch.tensor(0.0), torch.tensor(1.0)
            return pairs, None
        _one_device(grads, name)
        out = _grad_norm(grads, _grad_tables(grads), self._clip[1], self._clip[0])
        self.last_grad_norm, self.last_clip_coef = out[0], out[1]
        return pairs, out[1:]


class _AdamStep(_GradClip):
    """step() of Adam and AdamW (torch.optim.AdamW is torch.optim.Adam with decoupled_weight_decay=True)."""

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:                # a checkpoint of a capturable / fused torch optimiser
            group["foreach"], group["capturable"], group["fused"], group["differentiable"] = None, False, None, False
            for p in group["params"]:
                s = self.state.get(p, {}).get("step")
                if torch.is_tensor(s) and s.is_cuda:
                    self.state[p]["step"] = s.detach().to("cpu", torch.float32)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        name = f"dram_amd.optim.{type(self).__name__}"
        pairs, gscale = self._clip_pairs(name)
        for gi, group in enumerate(self.param_groups):
            lr = group["lr"]
            _no_tensor_lr(lr)
            beta1, beta2 = (float(b) for b in group["betas"])
            amsgrad = bool(group["amsgrad"])
            rows = []
            for p, g in (_with_grad(group, name) if pairs is None else pairs[gi]):
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    if amsgrad:
                        state["max_exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                step = _host_step(state, name)
                step += 1
                t = float(step)
                rows.append((p.device, p, g, _chk_state(state["exp_avg"], p, name), _chk_state(state["exp_avg_sq"], p, name),
                             _chk_state(state["max_exp_avg_sq"], p, name) if amsgrad else None,
                             float(lr) / (1.0 - beta1 ** t), math.sqrt(1.0 - beta2 ** t)))
            _launch("dram_optim_adam", rows, float(lr), beta1, beta2, float(group["eps"]), float(group["weight_decay"]),
                    int(bool(group["decoupled_weight_decay"])), int(amsgrad), int(bool(group["maximize"])), gscale=gscale)
        return loss


class Adam(_AdamStep, torch.optim.Adam):
    """torch.optim.Adam (arguments, validation, state and state dict) with the update on csrc/optim.hip."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, maximize=False,
                 decoupled_weight_decay=False):
        _no_tensor_lr(lr)
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, maximize=maximize,
                         decoupled_weight_decay=decoupled_weight_decay)


class AdamW(_AdamStep, torch.optim.AdamW):
    """torch.optim.AdamW (arguments, validation, state and state dict) with the update on csrc/optim.hip."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False):
        _no_tensor_lr(lr)
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, maximize=maximize)


class RAdam(_GradClip, torch.optim.RAdam):
    """torch.optim.RAdam (arguments, validation, state and state dict) with the update on csrc/optim.hip.  Whether a tensor
    takes the rectified update depends on its step count alone: the host decides per tensor and hands the kernel one step
    factor."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, decoupled_weight_decay=False, *,
                 maximize=False):
        _no_tensor_lr(lr)
        super().__init__(params, lr, betas, eps, weight_decay, decoupled_weight_decay, maximize=maximize)

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:                # a checkpoint of a capturable torch optimiser
            group["foreach"], group["capturable"], group["differentiable"] = None, False, False
            for p in group["params"]:
                s = self.state.get(p, {}).get("step")
                if torch.is_tensor(s) and s.is_cuda:
                    self.state[p]["step"] = s.detach().to("cpu", torch.float32)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        name = "dram_amd.optim.RAdam"
        pairs, gscale = self._clip_pairs(name)
        for gi, group in enumerate(self.param_groups):
            lr = group["lr"]
            _no_tensor_lr(lr)
            beta1, beta2 = (float(b) for b in group["betas"])
            rho_inf = 2.0 / (1.0 - beta2) - 1.0
            rows = []
            for p, g in (_with_grad(group, name) if pairs is None else pairs[gi]):
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                step = _host_step(state, name)
                step += 1
                t = float(step)
                bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
                rho_t = rho_inf - 2.0 * t * beta2 ** t / bc2
                if rho_t > 5.0:
                    rect = math.sqrt((rho_t - 4.0) * (rho_t - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t))
                    s0, s1 = float(lr) * rect * math.sqrt(bc2) / bc1, 1.0
                else:
                    s0, s1 = float(lr) / bc1, 0.0
                rows.append((p.device, p, g, _chk_state(state["exp_avg"], p, name), _chk_state(state["exp_avg_sq"], p, name),
                             None, s0, s1))
            _launch("dram_optim_radam", rows, float(lr), beta1, beta2, float(group["eps"]), float(group["weight_decay"]),
                    int(bool(group["decoupled_weight_decay"])), int(bool(group["maximize"])), gscale=gscale)
        return loss


class AdaBound(_GradClip, torch.optim.Optimizer):
    """AdaBound (Luo et al. 2019) with the constructor, the state and the arithmetic of the `adabound` package (0.0.5), the
    update on csrc/optim.hip:

        g' = g + wd p;  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2;  vuse = amsbound ? (vmax = max(vmax, v)) : v
        p -= clamp(lr sqrt(bc2) / bc1 / (sqrt(vuse) + eps), lower, upper) * m
        lower = final (1 - 1 / (gamma t + 1)),  upper = final (1 + 1 / (gamma t)),  final = final_lr * lr / base_lr

    `base_lrs` holds every group's lr at construction (an attribute, not in state_dict(), as in the package), so an LR
    scheduler scales the bounds with the rate.  State per parameter: `step` (a host fp32 scalar tensor; an int from a
    checkpoint the package wrote is taken over), `exp_avg`, `exp_avg_sq` and, with amsbound, `max_exp_avg_sq`.  The bounds
    depend on the step count and are launch scalars: a group whose parameters all have the same count -- the ordinary case
    -- is one launch, and every further distinct count one more."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), final_lr=0.1, gamma=1e-3, eps=1e-8, weight_decay=0,
                 amsbound=False):
        _no_tensor_lr(lr)
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= final_lr:
            raise ValueError(f"Invalid final learning rate: {final_lr}")
        if not 0.0 <= gamma < 1.0:
            raise ValueError(f"Invalid gamma parameter: {gamma}")
        defaults = dict(lr=lr, betas=betas, final_lr=final_lr, gamma=gamma, eps=eps, weight_decay=weight_decay,
                        amsbound=amsbound)
        super().__init__(params, defaults)
        self.base_lrs = [group["lr"] for group in self.param_groups]

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            group.setdefault("amsbound", False)

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if hasattr(self, "base_lrs"):                  # a group added after construction: its lr then is its base
            self.base_lrs.append(self.param_groups[-1]["lr"])

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        name = "dram_amd.optim.AdaBound"
        pairs, gscale = self._clip_pairs(name)
        for gi, (group, base_lr) in enumerate(zip(self.param_groups, self.base_lrs)):
            lr = group["lr"]
            _no_tensor_lr(lr)
            beta1, beta2 = (float(b) for b in group["betas"])
            amsbound = bool(group["amsbound"])
            gamma = float(group["gamma"])
            final = float(group["final_lr"]) * float(lr) / float(base_lr)
            by_step = {}
            for p, g in (_with_grad(group, name) if pairs is None else pairs[gi]):
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    if amsbound:
                        state["max_exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                step = _host_step(state, name)
                step += 1
                t = float(step)
                by_step.setdefault(t, []).append(
                    (p.device, p, g, _chk_state(state["exp_avg"], p, name), _chk_state(state["exp_avg_sq"], p, name),
                     _chk_state(state["max_exp_avg_sq"], p, name) if amsbound else None,
                     float(lr) * math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t), 0.0))
            for t, rows in by_step.items():
                lower = final * (1.0 - 1.0 / (gamma * t + 1.0))
                upper = final * (1.0 + 1.0 / (gamma * t)) if gamma != 0.0 else math.inf
                _launch("dram_optim_adabound", rows, beta1, beta2, float(group["eps"]), float(group["weight_decay"]),
                        int(amsbound), lower, upper, gscale=gscale)
        return loss


class SGD(_GradClip, torch.optim.SGD):
    """torch.optim.SGD (arguments, validation, state and state dict) with the update on csrc/optim.hip."""

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False):
        _no_tensor_lr(lr)
        if isinstance(weight_decay, torch.Tensor):
            raise TypeError("dram_amd.optim: weight_decay must be a Python number, got a tensor")
        super().__init__(params, lr, momentum, dampening, weight_decay, nesterov, maximize=maximize)

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            group["foreach"], group["fused"], group["differentiable"] = None, None, False

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        name = "dram_amd.optim.SGD"
        pairs, gscale = self._clip_pairs(name)
        for gi, group in enumerate(self.param_groups):
            lr = group["lr"]
            _no_tensor_lr(lr)
            momentum = float(group["momentum"])
            rows = []
            for p, g in (_with_grad(group, name) if pairs is None else pairs[gi]):
                buf, first = None, 0.0
                if momentum != 0:
                    state = self.state[p]
                    buf = state.get("momentum_buffer")
                    if buf is None:                    # torch: buf = clone(g'); here the kernel writes g' into it
                        buf = state["momentum_buffer"] = torch.empty_like(p, memory_format=torch.preserve_format)
                        first = 1.0
                    _chk_state(buf, p, name)
                rows.append((p.device, p, g, buf, None, None, first, 0.0))
            _launch("dram_optim_sgd", rows, float(lr), momentum, float(group["dampening"]), float(group["weight_decay"]),
                    int(bool(group["nesterov"])), int(bool(group["maximize"])), gscale=gscale)
        return loss
