"""Closure checks of the optimizer half of the training step: one Adam step (adam_kernel through
srmi_adam_step) and the micro-batch gradient sum (scale_add_kernel through srmi_axpy), against fp64
from the kernel's own operands.  Pure functions of CPU tensors: tests/test_gpu_update.py feeds them
the library's outputs, tests/test_adam_closure_checks.py an op-by-op fp32 restatement and the ways
the kernel could be subtly wrong (MUTATIONS).

Reference (reference()).  One step of torch.optim.Adam's L2 form in fp64 from the PRE-step
p, g, m, v (fp32 values widened) and `step`, with the hyper-parameters as the entry point receives
them -- C floats: float64(float32(lr)), and so beta1, beta2, eps, weight_decay -- and bc1, bc2
from pow in double, as srmi_adam_step forms them:

    g' = g + wd p            m' = m + c1 (g' - m)         v' = beta2 v + c2 g'^2
    den = sqrt(v') / sqrt(bc2) + eps      q = m' / den     ss = lr / bc1      p' = p - ss q

c1 = 1 - beta1 and c2 = 1 - beta2 are exact in fp32 for a float beta in [0.5, 1] (Sterbenz), so the
kernel's `1.f - b` is the reference's number (reference() refuses other betas).  Nothing compounds
from step to step: every step is checked from its own operands.

Bars (bars()), from the number formats alone; u = 2^-24, the fp32 unit roundoff.  They hold
whether or not the compiler contracts the multiply-adds (a contraction removes a rounding).

    dg' = 2u (|g| + |wd p|)                        two roundings: wd p, the sum; 0 when wd = 0
    dm  = c1 dg' + 3u (|m| + c1 (|g'| + |m|))      g' - m, c1 (.), m + (.)
    dv  = 4u v' + 2 c2 |g'| dg'                    beta2 v, c2 g', (.) g', the sum
    dden = (dv / (2 v') + 3u) den                  sqrtf, the division by fl(sqrt(bc2)), that
                                                   number's own rounding, + eps; dv / v' = 0 at v' = 0
    dq  = dm / den + |q| (dden / den + u/2)
    dp  = ss dq + 1.5u |ss q| + u |p'|             fl(ss), ss q, the subtraction

The one-u figure for sqrtf (and for the division) is an assumption about the device's math
library: tests/test_gpu_update.py measures fl(x / fl(sqrt(v))) against fp64 on the kernel's own v'
once and holds it to 2u (DESIGN.md section 4 records the figure).

"Moved": at least 99 % of the elements with g != 0 have v_new != v_old -- that the moments were
written at all.  It is a condition on the inputs (make_inputs), which the restatement meets.

Against the real torch.optim.Adam (torch_bars()).  The ABI's floats make the library a
self-consistent Adam with beta = float32(beta) and lr = float32(lr); torch holds the doubles.  With
db = float32(beta) - beta and the same pre-step state, to first order in db:

    m':   |db1| |g' - m|                                        (c1 changes by -db1)
    v':   |db2| (v + g'^2)                                      (beta2 by db2, c2 by -db2)
    bc:   |bf^t - b^t| <= t max(bf, b)^(t-1) |db|  (mean value theorem), so
          rel(bc2) = t bmax2^(t-1) |db2| / min(bc2),  rel(ss) = t bmax1^(t-1) |db1| / min(bc1) + |dlr| / lr

For t <= 3, bc2 ~ t c2 and rel(bc2) ~ |db2| / c2 = 1.3e-5 (beta2 = 0.999): the same size as v''s
own relative change, and sqrt halves both in the update.  The term grows like t |db| / b while
b^t ~ 1 and vanishes with b^t: at t = 20001 it is 20001 * 0.999^20000 * 1.3e-8 / 1 = 5e-13 and what
is left is v''s and m''s own change.  These, and a difference (ep, em, ev) of the pre-step
states (torch's second step starts from torch's first), go through the step linearly
(response()): dg' = wd ep; dm = beta1 em + c1 dg' + (m' term); dv = beta2 ev + 2 c2 |g'| dg' +
c2 dg'^2 + (v' term); the root sqrt(v') / sqrt(bc2) changes by dv / (2 sqrt(v')) (by sqrt(dv) at
v' = 0) over sqrt(bc2) plus rel(bc2) / 2 of itself; dq = dm / den + |q| droot / den;
dp = ep + ss dq + |ss q| rel(ss).  torch's own fp32 arithmetic obeys the closure bars about ITS
fp64 Adam (lerp_, mul_ + addcmul_, sqrt / bc2_sqrt + eps, addcdiv_: the same operations), and its
double scalars are rounded to fp32 inside those kernels (u relative each on c1, beta2, c2 and the
step size), which enters as |g' - m| c1 u, v' u and u on ss.  So

    bar(torch) = closure bar (the library's) + closure bar (torch's) + response(float-beta term
                 + scalar roundings + the previous step's bar)

each piece derived, none measured.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
CLASSES = ("m", "v", "p", "moved")
GRID_SPAN = 8192 * 256      # srmi_adam_step's grid cap in elements: the loop's second trip starts here
AXPY_SPAN = 4096 * 256      # srmi_axpy's
MOVED_MIN = 0.99


def f32(x):
    return float(np.float32(x))


def hyper(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, wd=0.0):
    """The hyper-parameters as srmi_adam_step receives them (C floats), as Python doubles."""
    return dict(lr=f32(lr), b1=f32(betas[0]), b2=f32(betas[1]), eps=f32(eps), wd=f32(wd))


def _t64(x):
    return torch.as_tensor(x).detach().to("cpu", torch.float64).reshape(-1)


def bias_corrections(hp, step):
    """bc1, bc2, and the two floats the kernel gets: step_size and bc2_sqrt."""
    bc1 = 1.0 - math.pow(hp["b1"], step)
    bc2 = 1.0 - math.pow(hp["b2"], step)
    return bc1, bc2, f32(hp["lr"] / bc1), f32(math.sqrt(bc2))


def reference(p, g, m, v, step, hp):
    """The fp64 step and its intermediates from the pre-step state."""
    if step < 1:
        raise ValueError("step < 1")
    if not (0.5 <= hp["b1"] <= 1.0 and 0.5 <= hp["b2"] <= 1.0):
        raise ValueError("1 - beta is exact in fp32 only for beta in [0.5, 1]")
    p, g, m, v = _t64(p), _t64(g), _t64(m), _t64(v)
    c1, c2 = 1.0 - hp["b1"], 1.0 - hp["b2"]
    bc1, bc2, _, _ = bias_corrections(hp, step)
    wp = hp["wd"] * p
    g1 = g + wp if hp["wd"] != 0.0 else g
    m1 = m + c1 * (g1 - m)
    v1 = hp["b2"] * v + c2 * g1 * g1
    den = v1.sqrt() / math.sqrt(bc2) + hp["eps"]
    q = m1 / den
    ss = hp["lr"] / bc1
    return dict(p0=p, g=g, m0=m, v0=v, wp=wp, g1=g1, m=m1, v=v1, den=den, q=q, ss=ss, dpu=ss * q, p=p - ss * q,
                c1=c1, c2=c2, bc1=bc1, bc2=bc2, hp=hp, step=step)


def bars(r):
    """dm, dv, dp of the module docstring, elementwise, from reference()'s dict."""
    c1, c2 = r["c1"], r["c2"]
    dg = 2 * U * (r["g"].abs() + r["wp"].abs()) if r["hp"]["wd"] != 0.0 else torch.zeros_like(r["g"])
    dm = c1 * dg + 3 * U * (r["m0"].abs() + c1 * (r["g1"].abs() + r["m0"].abs()))
    dv = 4 * U * r["v"] + 2 * c2 * r["g1"].abs() * dg
    rv = torch.where(r["v"] > 0, dv / r["v"].clamp_min(1e-300), torch.zeros_like(dv))
    dden = (0.5 * rv + 3 * U) * r["den"]
    dq = dm / r["den"] + r["q"].abs() * (dden / r["den"] + 0.5 * U)
    dp = r["ss"] * dq + 1.5 * U * r["dpu"].abs() + U * r["p"].abs()
    return dict(m=dm, v=dv, p=dp)


class Report:
    """rows: (class, worst error / bar, index of the worst, failing elements, first failing index,
    the tensor the worst lies in (a failing row: "worst's; first's") or None, ok).  The "moved" row
    holds the moved fraction in place of the ratio and the unmoved count in place of the index."""

    def __init__(self):
        self.rows = []

    def add(self, cls, ratio, index, nfail, first, name, ok):
        self.rows.append((cls, float(ratio), int(index), int(nfail), first, name, bool(ok)))

    def failures(self, cls):
        return [r for r in self.rows if r[0] == cls and not r[6]]

    def failed(self):
        return {r[0] for r in self.rows if not r[6]}

    def worst(self, cls):
        return max((r[1] for r in self.rows if r[0] == cls), default=0.0)

    def lines(self):
        out = []
        for c, ra, i, nf, fi, nm, ok in self.rows:
            if c == "moved":
                out.append(f"  moved fraction of the elements with g != 0 whose v changed: {ra:.4f} ({i} unmoved; "
                           f"needs >= {MOVED_MIN}){'' if ok else '  FAILS'}")
                continue
            out.append(f"  {c:5s} worst/bar {ra:9.3e} at {i}{'' if nm is None else ' (' + nm + ')'}"
                       f"{'' if ok else f'  FAILS: {nf} elements, first {fi}'}")
        return out


def _name_of(table, index):
    if table is None:
        return None
    for name, off, n, _ in table:
        if off <= index < off + n:
            return name
    return None


def ratio(err, bar):
    """err / bar with 0 / 0 = 0 and x / 0 = inf."""
    out = err / bar.clamp_min(1e-300)
    out = torch.where((bar == 0) & (err > 0), torch.full_like(out, math.inf), out)
    return torch.where(err == 0, torch.zeros_like(out), out)


def _row(rep, cls, got, want, bar, table):
    got = _t64(got)
    assert got.numel() == want.numel(), (cls, got.numel(), want.numel())
    ra = ratio((got - want).abs(), bar)
    ra = torch.where(torch.isfinite(got), ra, torch.full_like(ra, math.inf))
    bad = ra > 1.0
    nfail = int(bad.sum())
    i = int(ra.argmax())
    first = int(bad.nonzero()[0]) if nfail else None
    name = _name_of(table, i)
    if nfail and table is not None:
        name = f"{name}; first in {_name_of(table, first)}"
    rep.add(cls, ra[i], i, nfail, first, name, nfail == 0)


def check_step(pre, post, step, hp, table=None):
    """pre = (p, g, m, v) before the step, post = (p, m, v) after it -> Report over the classes
    m, v, p (against reference() within bars()) and "moved" (no element with g != 0: met, 1.0).
    table (an Engine's): failures and the worst element are named by tensor."""
    r = reference(*pre, step, hp)
    b = bars(r)
    rep = Report()
    for cls, got in (("m", post[1]), ("v", post[2]), ("p", post[0])):
        _row(rep, cls, got, r[cls], b[cls], table)
    nz = r["g"] != 0
    n_nz = int(nz.sum())
    moved = int(((_t64(post[2]) != r["v0"]) & nz).sum())
    frac = moved / n_nz if n_nz else 1.0
    rep.add("moved", frac, n_nz - moved, n_nz - moved, None, None, frac >= MOVED_MIN)
    return rep


# ----------------------------------------------------------------------------- inputs
def make_inputs(n, step, seed=0):
    """p ~ 0.05 N(0,1); g, m ~ N(0,1) 10^U(-10,0), v the square of such a draw, so that elements with
    sqrt(v) near eps exist; every seventh element of g, m, v exactly 0 (staggered: g at i % 7 = 1, m at
    3, v at 5, so that zeros meet non-zeros and element 0 -- all of n = 1 -- has none); m = v = 0 at step 1; no 0 < |g| < 1e-10, which keeps
    fp32 denormals out of g^2.  fp32 CPU tensors."""
    gen = torch.Generator(device="cpu").manual_seed(1000003 * seed + 7919 * (step % 1009) + n % 104729)

    def draw():
        return (torch.randn(n, generator=gen, dtype=torch.float64)
                * 10.0 ** (-10.0 * torch.rand(n, generator=gen, dtype=torch.float64)))

    i = torch.arange(n)
    p = (0.05 * torch.randn(n, generator=gen, dtype=torch.float64)).float()
    g = draw()
    g = torch.where(g.abs() < 1e-10, torch.copysign(torch.full_like(g, 1e-10), g), g)
    g = torch.where(i % 7 == 1, torch.zeros_like(g), g).float()
    if step == 1:
        m, v = torch.zeros(n), torch.zeros(n)
    else:
        m = torch.where(i % 7 == 3, torch.zeros(n, dtype=torch.float64), draw()).float()
        v = torch.where(i % 7 == 5, torch.zeros(n, dtype=torch.float64), draw() ** 2).float()
    return p, g, m, v


# ----------------------------------------------------------------------------- restatement
MUTATIONS = {
    0: "the kernel, op by op in fp32",
    1: "decoupled decay: p -= lr wd p, g untouched",
    2: "eps inside the bias-corrected root: (sqrt(v) + eps) / sqrt(bc2)",
    3: "bc2 of step + 1",
    4: "bc1 of step - 1 (step >= 2)",
    5: "(1 - beta2) g in place of (1 - beta2) g^2",
    6: "m updated from g instead of g' (wd != 0)",
    7: "the elements from 8192 * 256 on left untouched",
    8: "v not written back",
}


def restate_fp32(p, g, m, v, step, hp, mut=0):
    """adam_kernel with srmi_adam_step's two floats, every operation rounded to fp32 (no
    contraction) -> (p, m, v) fp32.  mut: a key of MUTATIONS."""
    p, g, m, v = (x.detach().cpu().float().reshape(-1) for x in (p, g, m, v))
    b1, b2, eps, wd = hp["b1"], hp["b2"], hp["eps"], hp["wd"]
    c1, c2 = f32(np.float32(1) - np.float32(b1)), f32(np.float32(1) - np.float32(b2))
    bc1 = 1.0 - math.pow(b1, step - 1 if mut == 4 else step)
    bc2 = 1.0 - math.pow(b2, step + 1 if mut == 3 else step)
    ss, bs = f32(hp["lr"] / bc1), f32(math.sqrt(bc2))
    gi = g
    if wd != 0.0 and mut != 1:
        gi = g + wd * p
    gm = g if mut == 6 else gi
    mi = m + c1 * (gm - m)
    vi = b2 * v + (c2 * gi if mut == 5 else c2 * gi * gi)
    den = (vi.sqrt() + eps) / bs if mut == 2 else vi.sqrt() / bs + eps
    pn = p - ss * (mi / den)
    if mut == 1 and wd != 0.0:
        pn = pn - f32(hp["lr"] * wd) * p
    vo = v.clone() if mut == 8 else vi
    if mut == 7:
        pn[GRID_SPAN:], mi[GRID_SPAN:], vo[GRID_SPAN:] = p[GRID_SPAN:], m[GRID_SPAN:], v[GRID_SPAN:]
    assert pn.dtype == mi.dtype == vo.dtype == torch.float32
    return pn, mi, vo


# ----------------------------------------------------------------------------- axpy
def check_axpy(y0, x, a, y1):
    """y1 = y0 + a x within u (|y'| + |a x|): the product's rounding and the sum's (one rounding
    of the exact y0 + a x if contracted).  a as the entry point receives it.  -> (worst / bar,
    failing elements, first failing index)."""
    a = f32(a)
    y0, x, y1 = _t64(y0), _t64(x), _t64(y1)
    want = y0 + a * x
    ra = ratio((y1 - want).abs(), U * (want.abs() + (a * x).abs()))
    ra = torch.where(torch.isfinite(y1), ra, torch.full_like(ra, math.inf))
    bad = ra > 1.0
    n = int(bad.sum())
    return float(ra.max()), n, (int(bad.nonzero()[0]) if n else None)


# ----------------------------------------------------------------------------- torch.optim.Adam
def response(r, ep, em, ev, dm_x, dv_x, rel_bc2, rel_ss):
    """First-order change of (p', m', v') of reference() r under a pre-state difference (ep, em, ev),
    additional changes dm_x of m' and dv_x of v', and relative changes of bc2 and of ss."""
    hp, c1, c2 = r["hp"], r["c1"], r["c2"]
    dg = abs(hp["wd"]) * ep
    dm = hp["b1"] * em + c1 * dg + dm_x
    dv = hp["b2"] * ev + 2 * c2 * r["g1"].abs() * dg + c2 * dg * dg + dv_x
    sv = r["v"].sqrt()
    droot = torch.where(sv > 0, 0.5 * dv / sv.clamp_min(1e-300), dv.sqrt()) / math.sqrt(r["bc2"])
    droot = droot + 0.5 * rel_bc2 * sv / math.sqrt(r["bc2"])
    dq = dm / r["den"] + r["q"].abs() * droot / r["den"]
    dp = ep + r["ss"] * dq + r["dpu"].abs() * rel_ss
    return dict(p=dp, m=dm, v=dv)


def float_beta_rel(bf, b, t):
    """Bound on |bf^t - b^t| / min(1 - bf^t, 1 - b^t): the relative change of a bias correction when
    beta is the float bf instead of b (mean value theorem; any t >= 1)."""
    d = abs(bf - b) * t * math.pow(max(bf, b), t - 1)
    return d / min(1.0 - math.pow(bf, t), 1.0 - math.pow(b, t))


def torch_bars(pre, step, hp, lr, betas, prev=None):
    """The bar of the library's step against torch.optim.Adam(lr, betas: Python doubles) from the
    pre-step state `pre` (the library's), torch's own differing from it by at most `prev` (the
    previous step's torch_bars; None: the same state).  -> dict p, m, v (module docstring)."""
    r = reference(*pre, step, hp)
    b = bars(r)
    z = torch.zeros_like(r["g"])
    ep, em, ev = (prev[k] for k in ("p", "m", "v")) if prev is not None else (z, z, z)
    db1, db2 = abs(hp["b1"] - betas[0]), abs(hp["b2"] - betas[1])
    gm = (r["g1"] - r["m0"]).abs()
    g2 = r["g1"] * r["g1"]
    dm_x = db1 * gm + U * r["c1"] * gm                      # float beta1; torch's c1 rounded to fp32
    dv_x = db2 * (r["v0"] + g2) + U * r["v"]                # float beta2; torch's beta2, c2 rounded
    rel_bc2 = float_beta_rel(hp["b2"], betas[1], step)
    rel_ss = float_beta_rel(hp["b1"], betas[0], step) + abs(hp["lr"] - lr) / lr + U
    x = response(r, ep, em, ev, dm_x, dv_x, rel_bc2, rel_ss)
    return {k: 2 * b[k] + x[k] for k in ("p", "m", "v")}


def torch_adam(table, state, opt_sd):
    """A CPU torch.optim.Adam over per-tensor fp32 parameters (the model state dict's values, in
    table order) loaded from a checkpoint's optimizer state dict.  -> (optimizer, parameters)."""
    ps = [torch.nn.Parameter(state[name].detach().clone().float()) for name, _, _, _ in table]
    g = opt_sd["param_groups"][0]
    opt = torch.optim.Adam(ps, lr=g["lr"], betas=tuple(g["betas"]), eps=g["eps"], weight_decay=g["weight_decay"])
    opt.load_state_dict(opt_sd)
    return opt, ps


def torch_adam_step(opt, ps, table, grads):
    """One step with the flat gradient `grads` -> flat (p, m, v) after it."""
    gh = grads.detach().cpu().float()
    for prm, (_, off, n, shape) in zip(ps, table):
        prm.grad = gh[off:off + n].view(shape).clone()
    opt.step()
    flat = lambda xs: torch.cat([x.detach().reshape(-1) for x in xs])  # noqa: E731
    return (flat(ps), flat([opt.state[q]["exp_avg"] for q in ps]), flat([opt.state[q]["exp_avg_sq"] for q in ps]))


def compare(got, want, bar, table=None):
    """-> (worst / bar, failing elements, first failing index, tensor of the worst)."""
    got = _t64(got)
    ra = ratio((got - _t64(want)).abs(), bar)
    ra = torch.where(torch.isfinite(got), ra, torch.full_like(ra, math.inf))
    bad = ra > 1.0
    n = int(bad.sum())
    i = int(bad.nonzero()[0]) if n else int(ra.argmax())
    return float(ra.max()), n, (i if n else None), _name_of(table, i)


def rel_size(got, want, bar, ref):
    """The deviation and its bar relative to |ref|, over the elements with ref != 0 ->
    (largest deviation, the bar at that element, median deviation, median bar).  For figures
    that are reported; nothing is asserted on them."""
    got, want, ref = _t64(got), _t64(want), _t64(ref).abs()
    ok = ref > 0
    d, b = (got - want).abs()[ok] / ref[ok], bar[ok] / ref[ok]
    i = int(d.argmax())
    return float(d[i]), float(b[i]), float(d.median()), float(b.median())
