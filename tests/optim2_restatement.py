"""numpy fp64 restatement of the RAdam and AdaBound updates of csrc/optim.hip, and the bound on what an fp32 evaluation of
the same update may differ from it by.  The companion of tests/optim_restatement.py (Adam, AdamW, SGD), whose unit roundoff,
`within` and derivation of the terms g', m and v this module takes over unchanged.

Definitions (per element; t = the parameter's own step count after increment, bc1 = 1 - b1^t, bc2 = 1 - b2^t):
  RAdam      g' = maximize ? -g : g;  decoupled weight decay: p *= 1 - lr wd;  otherwise g' += wd p
             m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2
             rho_inf = 2 / (1 - b2) - 1;  rho_t = rho_inf - 2 t b2^t / bc2
             rho_t > 5:   p -= lr rect sqrt(bc2) / bc1 * m / (sqrt(v) + eps)
                          rect = sqrt((rho_t - 4)(rho_t - 2) rho_inf / ((rho_inf - 4)(rho_inf - 2) rho_t))
             otherwise:   p -= lr / bc1 * m
  AdaBound   g' = g + wd p;  m, v as above;  vuse = amsbound ? (vmax = max(vmax, v)) : v
             final = final_lr lr / base_lr;  lower = final (1 - 1 / (gamma t + 1));  upper = final (1 + 1 / (gamma t))
             p -= clamp(lr sqrt(bc2) / bc1 / (sqrt(vuse) + eps), lower, upper) * m
In both, eps joins the raw root sqrt(v): not Adam's sqrt(v) / sqrt(bc2) + eps.
tests/test_optim2_cpu.py holds RAdamRun against torch.optim.RAdam in fp64.  AdaBound is not part of torch; where the `adabound`
package can be imported that test holds AdaBoundRun against it, and elsewhere the definition above, which is the package's
0.0.5 step() term by term, is the pin, and the test holds AdaBoundRun against a plain torch transcription of it.
"""
import math

import numpy as np

import optim_restatement as R1
from optim_restatement import TINY, U, UE, f64, within  # noqa: F401  (re-exported for the tests)

BOUND_DERIVATION = """
Bound derivation, in the manner of optim_restatement.BOUND_DERIVATION, which it continues: one relative error <= u per fp32
operation and per scalar rounded to fp32, written on the magnitudes of the OPERANDS; E* absolute, elementwise, carried from
step to step; for every term the larger count of the kernel's operation order and of the fp32 order it is compared with on
the CPU (torch.optim.RAdam; the adabound package's step()) is taken.

  g', the AdamW-style decay, m, v, vmax:  exactly optim_restatement's Eg, Ep (decay), Em, Ev, Evmax -- the kernel forms them by
      the same operations as the Adam kernel, torch.optim.RAdam by the same as torch.optim.Adam (lerp; mul, addcmul), and the
      package's m.mul_(b1).add_(1 - b1, g') is 3 roundings on either term, inside the 4 taken there.
  den = sqrt(vuse) + eps.  Carried: Es = min(Evuse / sqrt(vuse), sqrt(Evuse)) as there.  Local: the root (1) on sqrt(vuse), eps
      rounded (1) on eps, the sum (1) on den:  <= sqrt(vuse) + eps + den = 2 den.
      Eden = Es + 2u den;     den' = max(den - Eden, eps (1 - 2u)) is the smallest den the fp32 run can hold.

  RAdam, rectified:  upd = S m / den with the host scalar S = lr rect sqrt(bc2) / bc1.
      Kernel: quotient (1), S rounded (1), the product fused into the final sum (0) = 2.  torch: m / bc1 as a product with
      the rounded reciprocal (scalar, reciprocal, product: 3), times lr (scalar, product: 2), sqrt(bc2) / den as
      reciprocal times scalar (3), the product of the two (1), times rect (scalar, product: 2) = 11.  Taken: 12.
      Carried: S (Em / den' + |m| Eden / (den den')).  The final sum (1) is relative to |p| + |upd|:
      Ep <- Ep + S (Em / den' + |m| Eden / (den den')) + 12u |upd| + u (|p| + |upd|).
  RAdam, not rectified:  upd = (lr / bc1) m.  Kernel: scalar (1), fused product (0).  torch: m / bc1 (3), times lr (2) = 5:
      Ep <- Ep + (lr / bc1) Em + 5u |upd| + u (|p| + |upd|).
      v does not enter p in this branch, but it is updated, and Ev carried, all the same.

  AdaBound:  q = s / den with the host scalar s = lr sqrt(bc2) / bc1: s rounded (1), quotient (1), the same in the package
      (full_like, div_):      Eq = s Eden / (den den') + 2u q.
      r = clamp(q, lower, upper) = min(max(q, lower), upper).  The fp32 run clamps its own q~ (|q~ - q| <= Eq) at the ROUNDED
      bounds lower~ = lower (1 + d1), upper~ = upper (1 + d2), |d| <= u.  Take r* = clamp(q~, lower, upper): max and min are
      1-Lipschitz in each argument, so |r* - r| <= Eq WHICHEVER side of a bound q and q~ lie on -- an element that is clamped
      in one run and free in the other costs nothing extra.  And |r~ - r*| <= u r* (1 + 2u): where r~ = q~ the unrounded
      bounds move it by at most lower~ - lower or upper - upper~, onto that bound; where r~ = lower~, r* is lower or a q~
      between lower and lower~; where r~ = upper~, r* is upper or a q~ in (upper~, upper) >= upper (1 - u).  So the error
      of a bound is relative to the CLAMPED value, never to a bound that does not bind (upper is 1e11 in one test):
      Er = Eq + u (r + Eq).
      upd = r m: the kernel fuses the product into the final sum (0), the package rounds it (1); the final sum (1):
      Ep <- Ep + (r + Er) Em + |m| Er + u |upd| + u (|p| + |upd|).
Underflow: 2^-126 once per operation counted, as there.
"""


def rectification(t, b2):
    """(rho_t, rect or None) of RAdam at step t: a function of t and beta2 alone, evaluated in double."""
    rho_inf = 2.0 / (1.0 - b2) - 1.0
    rho_t = rho_inf - 2.0 * t * b2 ** t / (1.0 - b2 ** t)
    if rho_t > 5.0:
        return rho_t, math.sqrt((rho_t - 4.0) * (rho_t - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t))
    return rho_t, None


class _MomentRun:
    """p, m, v[, vmax], the step count and the bounds Ep, Em, Ev[, Evmax] of one tensor; `_moments` is the part of the step the
    two rules share with Adam (optim_restatement.AdamRun.step, the same expressions)."""

    def __init__(self, p, betas, eps, weight_decay, use_vmax, m, v, vmax, step):
        self.p = f64(p).copy()
        self.m = np.zeros_like(self.p) if m is None else f64(m).copy()
        self.v = np.zeros_like(self.p) if v is None else f64(v).copy()
        self.vmax = (np.zeros_like(self.p) if vmax is None else f64(vmax).copy()) if use_vmax else None
        self.t = int(step)
        self.b1, self.b2 = float(betas[0]), float(betas[1])
        assert self.b1 >= 0.5, "the bound on m covers torch's lerp form for beta1 >= 1/2 only (optim_restatement)"
        self.eps, self.wd = float(eps), float(weight_decay)
        self.Ep, self.Em, self.Ev = (np.zeros_like(self.p) for _ in range(3))
        self.Evmax = np.zeros_like(self.p) if use_vmax else None
        self.amsgrad = use_vmax                      # the name test_gpu_optim's checks read

    def _moments(self, g, lr, maximize=False, decoupled=False):
        b1, b2, wd = self.b1, self.b2, self.wd
        g = f64(g).reshape(self.p.shape)
        g = -g if maximize else g
        Eg = np.zeros_like(g)
        if wd != 0.0 and decoupled:
            self.Ep = abs(1.0 - lr * wd) * self.Ep + 2 * UE * np.abs(self.p) + TINY
            self.p = self.p * (1.0 - lr * wd)
        elif wd != 0.0:
            Eg = wd * self.Ep + 3 * UE * (np.abs(g) + wd * np.abs(self.p)) + 2 * TINY
            g = g + wd * self.p
        self.t += 1
        self.Em = b1 * self.Em + (1 - b1) * Eg + 4 * UE * (b1 * np.abs(self.m) + (1 - b1) * np.abs(g)) + 4 * TINY
        self.m = b1 * self.m + (1 - b1) * g
        self.Ev = b2 * self.Ev + (1 - b2) * (2 * np.abs(g) * Eg + Eg * Eg) + 4 * UE * (b2 * self.v + (1 - b2) * g * g) + 4 * TINY
        self.v = b2 * self.v + (1 - b2) * g * g

    def _den(self, vuse, Evuse):
        """den = sqrt(vuse) + eps, its bound Eden and den', the smallest value an fp32 run can hold for it."""
        s = np.sqrt(vuse)
        Es = np.minimum(np.sqrt(Evuse), np.where(s > 0, Evuse / np.where(s > 0, s, 1.0), np.inf))
        den = s + self.eps
        Eden = Es + 2 * UE * den
        return den, Eden, np.maximum(den - Eden, self.eps * (1 - 2 * UE))


class RAdamRun(_MomentRun):
    """One tensor under torch.optim.RAdam's rule.  `step(g, lr)`; g None: no gradient this step, nothing changes.
    `rectified` lists, step by step, whether the step took the rectified branch."""

    def __init__(self, p, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled_weight_decay=False, maximize=False,
                 m=None, v=None, step=0):
        super().__init__(p, betas, eps, weight_decay, False, m, v, None, step)
        self.decoupled, self.maximize = decoupled_weight_decay, maximize
        self.rectified = []

    def step(self, g, lr):
        if g is None:
            return self
        self._moments(g, lr, self.maximize, self.decoupled)
        bc1, bc2 = 1.0 - self.b1 ** self.t, 1.0 - self.b2 ** self.t
        _, rect = rectification(self.t, self.b2)
        self.rectified.append(rect is not None)
        with np.errstate(divide="ignore", invalid="ignore"):
            if rect is not None:
                S = lr * rect * math.sqrt(bc2) / bc1
                den, Eden, den_lo = self._den(self.v, self.Ev)
                upd = S * self.m / den
                self.Ep = (self.Ep + S * (self.Em / den_lo + np.abs(self.m) * Eden / (den * den_lo)) + 12 * UE * np.abs(upd)
                           + UE * (np.abs(self.p) + np.abs(upd)) + 8 * TINY)
            else:
                upd = (lr / bc1) * self.m
                self.Ep = self.Ep + (lr / bc1) * self.Em + 5 * UE * np.abs(upd) + UE * (np.abs(self.p) + np.abs(upd)) + 4 * TINY
        self.p = self.p - upd
        return self


class AdaBoundRun(_MomentRun):
    """One tensor under AdaBound.  `step(g, lr)` takes the group's current lr; `base_lr` is the group's lr at construction.
    `regimes` lists, step by step, the fractions of elements (clamped at lower, unclamped, clamped at upper), and
    `bounds` the (lower, upper) of the step."""

    def __init__(self, p, base_lr, betas=(0.9, 0.999), final_lr=0.1, gamma=1e-3, eps=1e-8, weight_decay=0.0, amsbound=False,
                 m=None, v=None, vmax=None, step=0):
        super().__init__(p, betas, eps, weight_decay, amsbound, m, v, vmax, step)
        self.base_lr, self.final_lr, self.gamma = float(base_lr), float(final_lr), float(gamma)
        self.regimes, self.bounds = [], []

    def step(self, g, lr):
        if g is None:
            return self
        self._moments(g, lr)
        vuse, Evuse = self.v, self.Ev
        if self.vmax is not None:
            self.Evmax = np.maximum(self.Evmax, self.Ev)
            self.vmax = np.maximum(self.vmax, self.v)
            vuse, Evuse = self.vmax, self.Evmax
        s = lr * math.sqrt(1.0 - self.b2 ** self.t) / (1.0 - self.b1 ** self.t)
        final = self.final_lr * lr / self.base_lr
        lower = final * (1.0 - 1.0 / (self.gamma * self.t + 1.0))
        upper = final * (1.0 + 1.0 / (self.gamma * self.t))
        with np.errstate(divide="ignore", invalid="ignore"):
            den, Eden, den_lo = self._den(vuse, Evuse)
            q = s / den
            Eq = s * Eden / (den * den_lo) + 2 * UE * q + 2 * TINY
            r = np.clip(q, lower, upper)
            Er = Eq + UE * (r + Eq) + TINY
            upd = r * self.m
            self.Ep = (self.Ep + (r + Er) * self.Em + np.abs(self.m) * Er + UE * np.abs(upd)
                       + UE * (np.abs(self.p) + np.abs(upd)) + 2 * TINY)
        n = max(q.size, 1)
        self.regimes.append((float((q < lower).sum()) / n, float(((q >= lower) & (q <= upper)).sum()) / n,
                             float((q > upper).sum()) / n))
        self.bounds.append((lower, upper))
        self.p = self.p - upd
        return self


# the option combinations of the tests: name -> (kind, constructor keywords beyond lr)
RADAM_CASES = {
    "radam": ("radam", {}),
    "radam_wd": ("radam", {"weight_decay": 0.05}),
    "radam_decoupled": ("radam", {"weight_decay": 0.1, "decoupled_weight_decay": True}),
    "radam_maximize": ("radam", {"maximize": True}),
    "radam_betas_eps": ("radam", {"betas": (0.8, 0.95), "eps": 1e-6}),
    "radam_all": ("radam", {"weight_decay": 0.05, "maximize": True, "betas": (0.8, 0.95), "eps": 1e-6}),
}
# gamma = 0.5 draws the bounds in within a few steps (lower 0.033 / 0.05 / 0.06, upper 0.3 / 0.2 / 0.167 at steps 1 / 2 / 3 for
# final_lr 0.1), so that make_inputs' gradients leave elements on both bounds and between them
ADABOUND_CASES = {
    "adabound": ("adabound", {"gamma": 0.5}),
    "adabound_wd": ("adabound", {"gamma": 0.5, "weight_decay": 0.05}),
    "adabound_amsbound": ("adabound", {"gamma": 0.5, "amsbound": True}),
    "adabound_betas_eps": ("adabound", {"gamma": 0.5, "betas": (0.8, 0.95), "eps": 1e-6, "final_lr": 0.05}),
    "adabound_all": ("adabound", {"gamma": 0.25, "weight_decay": 0.05, "amsbound": True, "final_lr": 0.2}),
    "adabound_default_gamma": ("adabound", {}),
}
CASES = {**RADAM_CASES, **ADABOUND_CASES}
LR = {"radam": 1e-2, "adabound": 1e-3}
STEPS = 8                       # RAdam with the default betas is first rectified at step 6


def make_run(kind, kw, p, base_lr=None, **state):
    if kind == "radam":
        return RAdamRun(p, **kw, **state)
    return AdaBoundRun(p, LR["adabound"] if base_lr is None else base_lr, **kw, **state)


def make_inputs(n, seed, steps=STEPS):
    """fp32 parameter ~ 0.1 N(0,1) and `steps` gradients whose magnitude is spread per element over 10^-3 .. 10^0.5 (a fixed
    per-element scale times N(0,1) about a common offset, so that m does not average to nothing): with lr 1e-3 the first
    step's rate 0.01 / |g| lies below AdaBound's lower bound for the large elements, above its upper bound for the small ones
    and between them for the rest.  Fixed by the seed, exactly representable in fp32."""
    rng = np.random.default_rng(seed)
    p = (0.1 * rng.standard_normal(n)).astype(np.float32)
    scale = 10.0 ** rng.uniform(-3.0, 0.5, n)
    off = 0.5 * rng.standard_normal(n)
    gs = [(scale * (off + rng.standard_normal(n))).astype(np.float32) for _ in range(steps)]
    return p, gs


def inputs(kind, n, seed, steps=STEPS):
    """RAdam: optim_restatement's inputs (|g| ~ 0.01), `steps` of them; AdaBound: the spread ones above."""
    return R1.make_inputs(n, seed, steps) if kind == "radam" else make_inputs(n, seed, steps)
