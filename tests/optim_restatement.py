"""numpy fp64 restatement of the optimiser update of csrc/optim.hip (Adam, AdamW, SGD as torch defines them), and the bound
on what an fp32 evaluation of the same update may differ from it by.

Definitions (per element; t = the parameter's own step count after increment):
  Adam / AdamW   g' = maximize ? -g : g
                 Adam with weight_decay: g' += wd p        AdamW: p *= 1 - lr wd
                 m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2;  vuse = amsgrad ? (vmax = max(vmax, v)) : v
                 den = sqrt(vuse) / sqrt(1 - b2^t) + eps;  p -= lr / (1 - b1^t) * m / den
  SGD            g' = maximize ? -g : g;  g' += wd p;  buf = g' on the first step, then mu buf + (1 - dampening) g'
                 g' = nesterov ? g' + mu buf : buf (with momentum);  p -= lr g'
tests/test_optim_cpu.py holds these against torch's own optimisers in fp64.

`AdamRun` / `SgdRun` carry one tensor through its steps in fp64 and, beside p, m, v (buf), the bounds Ep, Em, Ev: see
`Bound derivation` below.
"""
import math

import numpy as np

U = 2.0 ** -24                    # unit roundoff of fp32 (round to nearest)
UE = U * (1.0 + 2.0 ** -10)       # ... with room for the second-order terms the first-order analysis below drops
TINY = 2.0 ** -126                # smallest normal fp32 number: the absolute error of an operation that underflows

BOUND_DERIVATION = """
Bound derivation.  An fp32 evaluation differs from the fp64 one by (a) the error its inputs already carry, propagated, and
(b) one relative error <= u = 2^-24 per fp32 operation (IEEE add, multiply, fma, divide and square root are correctly
rounded) and per scalar hyper-parameter, which is rounded to fp32 once.  fp64's own error (2^-53) is ignored.  Every local
term is written on the MAGNITUDES OF THE OPERANDS, not on the result: m = b1 m + (1 - b1) g' cancels when m and g' differ in
sign, and the rounding errors do not shrink with it.  E* are absolute, elementwise, and carried from step to step.  The
counts cover the kernel's operation order AND the order torch's fp32 optimisers use (which the CPU test holds to the same
bound): the larger count of the two is taken, term by term.

  g' (weight decay, Adam and SGD):  g + wd p.  wd rounded (1), product (1; 0 when fused), sum (1):
      Eg = wd Ep + 3u (|g| + wd |p|).        Without weight decay g' = +-g exactly and Eg = 0.
  AdamW decay:  p (1 - lr wd): the factor rounded (1), product (1):   Ep <- |1 - lr wd| Ep + 2u |p|.
  m:  kernel fma(b1, m, (1-b1) g'):  on the m term b1 rounded + final rounding = 2, on the g' term (1-b1) rounded + product +
      final = 3.  torch: m + (1-b1)(g' - m) (lerp): difference (1), weight rounded (1), product (1) -- each relative to
      (1-b1)(|g'| + |m|) -- and the final sum (1) relative to b1 |m| + (1-b1) |g'|: 4 (1-b1) |g'| + (b1 + 3 (1-b1)) |m|, which
      is within 4 (b1 |m| + (1-b1) |g'|) whenever b1 >= 1/2 (asserted).  So
      Em <- b1 Em + (1-b1) Eg + 4u (b1 |m| + (1-b1) |g'|).
  v:  g'^2 (1), (1-b2) rounded (1), product (1), final (1) = 4 on the g' term; b2 rounded, [product,] final <= 3 on the v term:
      Ev <- b2 Ev + (1-b2) (2 |g'| Eg + Eg^2) + 4u (b2 v + (1-b2) g'^2).
  vmax = max(vmax, v) is exact and max is 1-Lipschitz in each argument:  Evmax <- max(Evmax, Ev).
  den = sqrt(vuse) / sqrt(bc2) + eps.  |sqrt(a) - sqrt(b)| = |a - b| / (sqrt(a) + sqrt(b)) <= |a - b| / sqrt(a), so the carried
      error is Es = min(Evuse / sqrt(vuse), sqrt(Evuse)) (also |sqrt(a) - sqrt(b)| <= sqrt(|a - b|), the smaller one where
      weight decay made g' cancel and vuse is no larger than its error).  Local: root (1), sqrt(bc2) rounded (1), quotient (1) on
      sqrt(vuse)/sqrt(bc2); eps rounded (1) on eps; the sum (1) on den: <= 3 (den - eps) + eps + den <= 4 den:
      Eden = Es / sqrt(bc2) + 4u den.
  p:  upd = (lr / bc1) (m / den): quotient (1), lr / bc1 rounded (1), product (1; 0 when fused into the sum): 3u |upd| local,
      plus the carried Em / den' + |m| Eden / (den den') with den' = max(den - Eden, eps (1 - 2u)) the smallest den the fp32 run can hold (its root is >= 0);
      the final sum (1) is relative to |p - upd| <= |p| + |upd|:
      Ep <- Ep + (lr / bc1) (Em / den' + |m| Eden / (den den')) + 3u |upd| + u (|p| + |upd|).
  SGD buf:  kernel fma(mu, buf, (1-d) g') 2 / 3 roundings, torch buf.mul_(mu).add_(g', alpha=1-d) 3 / 3:
      Eb <- mu Eb + |1-d| Eg + 3u (mu |buf| + |1-d| |g'|);  the first step copies g':  Eb = Eg.
  SGD nesterov:  g'' = g' + mu buf: mu rounded, [product,] sum:  Eg'' = Eg + mu Eb + 3u (|g'| + mu |buf|);  else g'' = buf, Eb.
  SGD p:  p - lr g'': lr rounded (1), product (1; 0 when fused), sum (1):
      Ep <- Ep + lr Eg'' + 2u lr |g''| + u (|p| + lr |g''|).
Underflow: an operation whose result falls below the smallest normal number 2^-126 keeps fewer bits (gradual underflow) or none
(flush to zero); either way its absolute error is <= 2^-126, which every E above takes once per operation counted (g'^2 of
a gradient below 1e-19 is such a result; the term is far below u times any operand that matters).
u is taken as 2^-24 (1 + 2^-10): every dropped second-order term is a product of two of the terms above, i.e. at most a few
u times a first-order term.
"""


def f64(a):
    return np.asarray(a, dtype=np.float64)


class AdamRun:
    """One tensor under Adam (decoupled=False) or AdamW (decoupled=True).  `step(g, lr)` advances p, m, v[, vmax], the step count
    and the bounds; g None: the parameter has no gradient this step and nothing changes."""

    def __init__(self, p, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, maximize=False, decoupled=False,
                 m=None, v=None, vmax=None, step=0):
        self.p = f64(p).copy()
        self.m = np.zeros_like(self.p) if m is None else f64(m).copy()
        self.v = np.zeros_like(self.p) if v is None else f64(v).copy()
        self.vmax = (np.zeros_like(self.p) if vmax is None else f64(vmax).copy()) if amsgrad else None
        self.t = int(step)
        self.b1, self.b2 = float(betas[0]), float(betas[1])
        assert self.b1 >= 0.5, "the bound on m covers torch's lerp form for beta1 >= 1/2 only (see BOUND_DERIVATION)"
        self.eps, self.wd, self.amsgrad, self.maximize, self.decoupled = float(eps), float(weight_decay), amsgrad, maximize, decoupled
        self.Ep, self.Em, self.Ev = (np.zeros_like(self.p) for _ in range(3))
        self.Evmax = np.zeros_like(self.p) if amsgrad else None

    def step(self, g, lr):
        if g is None:
            return self
        b1, b2, wd = self.b1, self.b2, self.wd
        g = f64(g).reshape(self.p.shape)
        g = -g if self.maximize else g
        Eg = np.zeros_like(g)
        if wd != 0.0 and self.decoupled:
            self.Ep = abs(1.0 - lr * wd) * self.Ep + 2 * UE * np.abs(self.p) + TINY
            self.p = self.p * (1.0 - lr * wd)
        elif wd != 0.0:
            Eg = wd * self.Ep + 3 * UE * (np.abs(g) + wd * np.abs(self.p)) + 2 * TINY
            g = g + wd * self.p
        self.t += 1
        bc1, bc2s = 1.0 - b1 ** self.t, math.sqrt(1.0 - b2 ** self.t)
        self.Em = b1 * self.Em + (1 - b1) * Eg + 4 * UE * (b1 * np.abs(self.m) + (1 - b1) * np.abs(g)) + 4 * TINY
        self.m = b1 * self.m + (1 - b1) * g
        self.Ev = b2 * self.Ev + (1 - b2) * (2 * np.abs(g) * Eg + Eg * Eg) + 4 * UE * (b2 * self.v + (1 - b2) * g * g) + 4 * TINY
        self.v = b2 * self.v + (1 - b2) * g * g
        vuse, Evuse = self.v, self.Ev
        if self.amsgrad:
            self.Evmax = np.maximum(self.Evmax, self.Ev)
            self.vmax = np.maximum(self.vmax, self.v)
            vuse, Evuse = self.vmax, self.Evmax
        s = np.sqrt(vuse)
        Es = np.minimum(np.sqrt(Evuse), np.where(s > 0, Evuse / np.where(s > 0, s, 1.0), np.inf))
        den = s / bc2s + self.eps
        Eden = Es / bc2s + 4 * UE * den
        den_lo = np.maximum(den - Eden, self.eps * (1 - 2 * UE))
        upd = (lr / bc1) * self.m / den
        self.Ep = (self.Ep + (lr / bc1) * (self.Em / den_lo + np.abs(self.m) * Eden / (den * den_lo)) + 3 * UE * np.abs(upd)
                   + UE * (np.abs(self.p) + np.abs(upd)) + 4 * TINY)
        self.p = self.p - upd
        return self


class SgdRun:
    """One tensor under torch's SGD rule; `buf` None until the first step with a gradient (momentum != 0)."""

    def __init__(self, p, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, maximize=False, buf=None):
        self.p = f64(p).copy()
        self.buf = None if buf is None else f64(buf).copy()
        self.mu, self.damp, self.wd, self.nesterov, self.maximize = float(momentum), float(dampening), float(weight_decay), nesterov, maximize
        self.Ep = np.zeros_like(self.p)
        self.Eb = np.zeros_like(self.p)

    def step(self, g, lr):
        if g is None:
            return self
        mu, wd, omd = self.mu, self.wd, 1.0 - self.damp
        g = f64(g).reshape(self.p.shape)
        g = -g if self.maximize else g
        Eg = np.zeros_like(g)
        if wd != 0.0:
            Eg = wd * self.Ep + 3 * UE * (np.abs(g) + wd * np.abs(self.p)) + 2 * TINY
            g = g + wd * self.p
        if mu != 0.0:
            if self.buf is None:
                self.buf, self.Eb = g.copy(), Eg.copy()
            else:
                self.Eb = mu * self.Eb + abs(omd) * Eg + 3 * UE * (mu * np.abs(self.buf) + abs(omd) * np.abs(g)) + 3 * TINY
                self.buf = mu * self.buf + omd * g
            if self.nesterov:
                Eg = Eg + mu * self.Eb + 3 * UE * (np.abs(g) + mu * np.abs(self.buf)) + 2 * TINY
                g = g + mu * self.buf
            else:
                g, Eg = self.buf, self.Eb
        self.Ep = self.Ep + lr * Eg + 2 * UE * lr * np.abs(g) + UE * (np.abs(self.p) + lr * np.abs(g)) + 2 * TINY
        self.p = self.p - lr * g
        return self


def within(got, want, bound):
    """(ok, worst ratio |got - want| / bound over the elements; 0 / 0 counts as 0)."""
    d = np.abs(f64(got).reshape(want.shape) - want)
    ok = bool((d <= bound).all())
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d > 0, d / bound, 0.0)
    return ok, float(r.max()) if r.size else 0.0


# the option combinations of the tests: name -> (kind, constructor keywords beyond lr)
ADAM_CASES = {
    "adam": ("adam", {}),
    "adam_wd": ("adam", {"weight_decay": 0.05}),
    "adam_amsgrad": ("adam", {"amsgrad": True}),
    "adam_maximize": ("adam", {"maximize": True}),
    "adam_betas_eps": ("adam", {"betas": (0.8, 0.95), "eps": 1e-6}),
    "adam_all": ("adam", {"weight_decay": 0.05, "amsgrad": True, "maximize": True}),
    "adamw": ("adamw", {}),
    "adamw_wd_amsgrad": ("adamw", {"weight_decay": 0.1, "amsgrad": True}),
}
SGD_CASES = {
    "sgd": ("sgd", {}),
    "sgd_wd": ("sgd", {"weight_decay": 0.05}),
    "sgd_momentum": ("sgd", {"momentum": 0.9}),
    "sgd_dampening": ("sgd", {"momentum": 0.9, "dampening": 0.3}),
    "sgd_nesterov": ("sgd", {"momentum": 0.9, "nesterov": True}),
    "sgd_maximize": ("sgd", {"momentum": 0.8, "maximize": True, "weight_decay": 0.01}),
}
CASES = {**ADAM_CASES, **SGD_CASES}
LR = 1e-2


def make_run(kind, kw, p, **state):
    if kind == "sgd":
        return SgdRun(p, **kw, **state)
    kw = dict(kw)
    if kind == "adamw":
        kw.setdefault("weight_decay", 1e-2)
    return AdamRun(p, decoupled=kind == "adamw", **kw, **state)


def make_inputs(n, seed, steps=5):
    """fp32 parameter ~ 0.1 N(0,1) and `steps` gradients ~ 0.01 N(0,1) with a common per-element offset (so that m does not
    average to nothing) -- fixed by the seed, exactly representable in fp32."""
    rng = np.random.default_rng(seed)
    p = (0.1 * rng.standard_normal(n)).astype(np.float32)
    off = 0.005 * rng.standard_normal(n)
    gs = [(off + 0.01 * rng.standard_normal(n)).astype(np.float32) for _ in range(steps)]
    return p, gs
