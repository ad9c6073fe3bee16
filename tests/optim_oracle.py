"""fp64 restatement of the optimizer guards ("Optimizer guards"): the gradient
norm and clip coefficient of torch.nn.utils.clip_grad_norm_, a clipped Adam step (the Adam part is
tests/adam_closure.py's reference / bars / check_step), the EMA lerp with its warm-up, and the
learning-rate schedules' closed forms.  numpy and Python floats only; tests/test_optim_oracle.py
holds it against torch on the CPU, tests/test_gpu_optim.py holds the library against it.

Bars, from the number formats alone (u = 2^-24, the fp32 unit roundoff):

  norm   NORM_BAR = 2^-22 relative.  The device squares in fp64 (exact: 24 + 24 bits) and adds n
         non-negative fp64 terms in some order: at most n 2^-53 relative, 1.5e-9 at the largest n
         used, 2^27; the square root adds 2^-53 and the rounding of the result to fp32 2^-24.
         2^-24 (1 + 0.02) with a margin of 4 is 2^-22.
  coef   the same: min(1, max_norm / (norm + 1e-6)) is evaluated in fp64 from the fp64 norm
         (relative error as above, without the fp32 rounding) and rounded to fp32 once.
  ema    e' = e + c (p - e), c = fl(1 - fl(decay)) as the kernel forms it: the subtraction
         rounds by at most u |p - e| <= u (|p| + |e|), which the product scales by c <= 1; the
         product rounds by u c |p - e| <= u (|p| + |e|); the sum rounds by u |e'|, and e' lies
         between e and p, so |e'| <= |p| + |e|.  Three roundings of at most u (|p| + |e|) each
         (a contraction only removes one): EMA_BAR = 3 u (|p| + |e|), times (1 + 2^-20) for the
         second-order terms.
"""
import math

import numpy as np

import adam_closure as ac

U = ac.U
NORM_BAR = 2.0 ** -22
CLIP_EPS = 1e-6  # clip_grad_norm_'s


def norm(g) -> float:
    """The L2 norm of the flat gradient, squares and sum in fp64 (math.fsum: exactly rounded)."""
    g = np.asarray(g, dtype=np.float64).reshape(-1)
    return math.sqrt(math.fsum(g * g))


def clip_coef(nrm: float, max_norm: float) -> float:
    """clip_grad_norm_: min(1, max_norm / (norm + 1e-6)); max_norm = inf never clips."""
    return min(1.0, max_norm / (nrm + CLIP_EPS))


def ctl_record(g, max_norm=math.inf, skipped=0.0):
    """What srmi_grad_norm leaves in ctl[4], as Python doubles (ctl[0], ctl[1] before their
    rounding to fp32): (norm, coefficient, finite, skipped count)."""
    nrm = norm(g)
    with np.errstate(over="ignore"):
        finite = math.isfinite(float(np.float32(nrm)))  # of the fp32 number that is reported
    return (nrm, clip_coef(nrm, max_norm) if finite else 0.0, 1.0 if finite else 0.0,
            skipped + (0.0 if finite else 1.0))


def clipped(g, coef):
    """g' = fl(g * coef) in fp32, the gradient the guarded step runs Adam on (coef: the fp32
    number in ctl[1])."""
    import torch
    g = torch.as_tensor(g).detach().cpu().float()
    out = (g.double() * float(np.float32(coef))).float()  # one rounding of the exact fp64 product
    return out


def clipped_adam(p, g, m, v, step, hp, coef):
    """One fp64 Adam step on the clipped gradient: adam_closure.reference on (p, g', m, v)."""
    return ac.reference(p, clipped(g, coef), m, v, step, hp)


def check_clipped_step(pre, post, step, hp, coef, table=None):
    """adam_closure.check_step over (p, g', m, v), at its own bars."""
    p, g, m, v = pre
    return ac.check_step((p, clipped(g, coef), m, v), post, step, hp, table)


def ema_decay_at(decay: float, warmup: bool, t: int) -> float:
    """The decay of Adam step t (1-based): min(decay, (1 + t) / (10 + t)) under warm-up."""
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


def ema_lerp(ema, p_new, decay):
    """ema + c (p_new - ema) in fp64, c = fl(1 - fl(decay)): the kernel's own coefficient."""
    c = float(np.float32(1.0) - np.float32(decay))
    e, p = np.asarray(ema, dtype=np.float64), np.asarray(p_new, dtype=np.float64)
    return e + c * (p - e)


def ema_bar(ema, p_new):
    e, p = np.abs(np.asarray(ema, dtype=np.float64)), np.abs(np.asarray(p_new, dtype=np.float64))
    return 3.0 * U * (e + p) * (1.0 + 2.0 ** -20)


def check_ema(ema0, p_new, decay, ema1):
    """-> (worst error / bar, failing elements)."""
    err = np.abs(np.asarray(ema1, dtype=np.float64) - ema_lerp(ema0, p_new, decay))
    bar = ema_bar(ema0, p_new)
    ok = np.isfinite(np.asarray(ema1, dtype=np.float64))
    ra = np.where(err == 0, 0.0, err / np.maximum(bar, 1e-300))
    ra = np.where(ok, ra, np.inf)
    return float(ra.max()), int((ra > 1.0).sum())


# ----------------------------------------------------------------------------- schedules
def lr_constant(lr, t0):
    return lr


def lr_step(lr, t0, step_size, gamma):
    return lr * gamma ** (t0 // step_size)


def lr_cosine(lr, t0, t_max, eta_min=0.0):
    if t0 >= t_max:
        return eta_min
    return eta_min + (lr - eta_min) * (1.0 + math.cos(math.pi * t0 / t_max)) / 2.0


def lr_warmup(lr, t0, W, s, main):
    """lr (s + (1 - s) t0 / W) for t0 < W, then main(t0 - W)."""
    if t0 < W:
        return lr * (s + (1.0 - s) * t0 / W)
    return main(t0 - W)


def schedule(cfg, lr, t0):
    """The rate of a FusedTrainer lr_schedule dict at t0 (Adam step t uses t0 = t - 1)."""
    kind = cfg["kind"]
    if kind == "constant":
        main = lambda x: lr_constant(lr, x)  # noqa: E731
    elif kind == "step":
        main = lambda x: lr_step(lr, x, cfg["step_size"], cfg["gamma"])  # noqa: E731
    elif kind == "cosine":
        main = lambda x: lr_cosine(lr, x, cfg["t_max"], cfg.get("eta_min", 0.0))  # noqa: E731
    else:
        raise ValueError(kind)
    return lr_warmup(lr, t0, cfg.get("warmup", 0), cfg.get("warmup_start", 0.0), main)


# ----------------------------------------------------------------------------- inputs
def wide_gradient(n, seed=0):
    """fp32 values with magnitudes from 1e-30 to 1e+25, signs mixed: their squares overflow (and
    underflow) fp32 but not fp64, so an fp32 accumulator shows up as inf.  Element 0 is the
    largest in magnitude class (1e25), so n = 1 has a norm whose square overflows fp32 too."""
    rng = np.random.default_rng(7919 * seed + n % 104729)
    mag = 10.0 ** rng.uniform(-30.0, 25.0, size=n)
    g = (mag * rng.choice([-1.0, 1.0], size=n)).astype(np.float32)
    g[0] = np.float32(-3.7e24)
    return g
