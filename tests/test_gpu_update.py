"""The optimizer half of the training step against fp64 Adam (tests/adam_closure.py; what each
check catches is shown on the CPU in tests/test_adam_closure_checks.py):

 a. srmi_adam_step (adam_kernel): p, m and v against the fp64 step from the kernel's own operands,
    bars from the number formats; n = 1, 255, 256, 257 and 8192 * 256 + 777 (the grid-stride
    loop's second trip with a ragged tail), steps 1, 2, 3, 1000, 100000, weight_decay 0 and 1e-2,
    lr 1e-3 and 5e-5, a non-default (beta1, beta2, eps) once per n; two calls bit-identical; the
    zero step leaves p bit-unchanged; step < 1 refused; the device's sqrtf and division measured
    once against the one-u-each figure the bars assume.
 b. srmi_axpy (scale_add_kernel) against fp64, n = 1, 257, 4096 * 256 + 777, a = 1 and -0.37.
 c. The update through FusedTrainer (small RCAN, B = 4, micro 1 and 2, weight_decay 1e-2, 3
    steps): the checkers over the whole flat buffer from (p0, grads, m0, v0, t), and after every
    step every engine's forward bit-identical to a fresh Engine packed with the new weights.
 d. Steps 2 and 3 against a real CPU torch.optim.Adam loaded from the checkpoint after step 1 and
    fed the engine's gradients, within adam_closure.torch_bars (the closure bars plus the
    float-beta term, derived there).
 e. The checkpoint's steps edited to 20000, loaded into a second trainer: one more step, the closure
    bar at t = 20001 and torch_bars against torch.optim.Adam loaded from the same dict.
"""
import functools
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

import adam_closure as ac  # noqa: E402

NS = [1, 255, 256, 257, ac.GRID_SPAN + 777]
STEPS = [1, 2, 3, 1000, 100000]
WDS = [0.0, 1e-2]
LRS = [1e-3, 5e-5]
OTHER = (0.8, 0.99, 1e-6)   # beta1, beta2, eps


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _inputs(n, step):
    return ac.make_inputs(n, step)


def _adam(pre, step, lr, betas, eps, wd):
    """One srmi_adam_step on copies of the CPU pre-state -> (p, m, v) on the CPU."""
    from srmi.engine import adam_step
    p, g, m, v = (x.to(dev()).clone() for x in pre)
    adam_step(p, g, m, v, step, lr, betas, eps, wd)
    torch.cuda.synchronize()
    assert torch.equal(g.cpu(), pre[1])  # the gradient is read only
    return p.cpu(), m.cpu(), v.cpu()


# ---------------------------------------------------------------------------------- a
@pytest.mark.parametrize("n", NS)
def test_adam_step_closes(n):
    worst = {c: 0.0 for c in ac.CLASSES[:3]}
    cases = [(s, w, l, (0.9, 0.999), 1e-8) for s, w, l in itertools.product(STEPS, WDS, LRS)]
    cases.append((3, 1e-2, 1e-3, OTHER[:2], OTHER[2]))
    bad = []
    for step, wd, lr, betas, eps in cases:
        pre = _inputs(n, step)
        assert bool(pre[1][0] != 0) and (step == 1 or bool((pre[2][0] != 0) & (pre[3][0] != 0)))  # n = 1 too
        post = _adam(pre, step, lr, betas, eps, wd)
        rep = ac.check_step(pre, post, step, ac.hyper(lr, betas, eps, wd))
        for c in worst:
            worst[c] = max(worst[c], rep.worst(c))
        if rep.failed():
            bad.append((step, wd, lr, betas, eps, rep.lines()))
    print(f"\nadam n {n}: worst error / bar over {len(cases)} cases: "
          + " ".join(f"{c} {x:.4f}" for c, x in worst.items()))
    assert not bad, bad


@pytest.mark.parametrize("n", [257, ac.GRID_SPAN + 777])
def test_adam_step_is_deterministic(n):
    pre = _inputs(n, 3)
    a = _adam(pre, 3, 1e-3, (0.9, 0.999), 1e-8, 1e-2)
    b = _adam(pre, 3, 1e-3, (0.9, 0.999), 1e-8, 1e-2)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("n", [257, ac.GRID_SPAN + 777])
def test_zero_step_leaves_p_unchanged(n):
    """g = 0, m = v = 0, wd = 0: p' = p - ss * (0 / (0 + eps)) = p, bit for bit."""
    p = _inputs(n, 1)[0]
    z = torch.zeros(n)
    pn, mn, vn = _adam((p, z, z, z), 1, 1e-3, (0.9, 0.999), 1e-8, 0.0)
    assert torch.equal(pn, p) and not mn.any() and not vn.any()


def test_step_below_one_is_refused():
    from srmi._lib import SrmiError
    from srmi.engine import adam_step
    pre = [x.to(dev()).clone() for x in _inputs(257, 3)]
    for step in (0, -1):
        with pytest.raises(SrmiError):
            adam_step(*pre, step, 1e-3)
    torch.cuda.synchronize()
    assert all(torch.equal(x.cpu(), y) for x, y in zip(pre, _inputs(257, 3)))


def test_device_sqrt_and_division_are_within_one_u_each():
    """The bars take sqrtf and the division at one u each.  Measured on the kernel's own v': with
    step = 100000 (bc1 = bc2 = 1 in double), lr = 1, eps = 0, p = 0 and g = m = x a power of two,
    m' = x exactly and p' = -fl(x / fl(sqrt(v'))): the composite's error against fp64 x / sqrt(v')
    is sqrtf's plus the division's, held to 2u (DESIGN.md section 4 records the figure)."""
    n = 100_000
    gen = torch.Generator().manual_seed(5)
    x = 2.0 ** -(torch.arange(n) % 30).float()
    v = ((torch.randn(n, generator=gen, dtype=torch.float64)
          * 10.0 ** (-8.0 * torch.rand(n, generator=gen, dtype=torch.float64))) ** 2).float()
    pn, mn, vn = _adam((torch.zeros(n), x, x.clone(), v), 100000, 1.0, (0.9, 0.999), 0.0, 0.0)
    assert torch.equal(mn, x)
    want = -x.double() / vn.double().sqrt()
    rel = ((pn.double() - want) / want).abs() / ac.U
    print(f"\nfl(x / fl(sqrt(v'))) against fp64: worst {float(rel.max()):.3f} u, mean {float(rel.mean()):.3f} u")
    assert float(rel.max()) <= 2.0


# ---------------------------------------------------------------------------------- b
@pytest.mark.parametrize("a", [1.0, -0.37])
@pytest.mark.parametrize("n", [1, 257, ac.AXPY_SPAN + 777])
def test_axpy_closes(n, a):
    """x ~ N(0,1) and y ~ 0.05 N(0,1) of their own draw (gradient sums have no exact zeros): at
    every n, n = 1 included, the first element's sum differs from y by far more than the bar, so a
    kernel that wrote nothing fails the check."""
    from srmi.engine import axpy
    gen = torch.Generator().manual_seed(4099 + n)
    y0, x0 = 0.05 * torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    assert bool(x0[0].abs() > 1e-3) and bool(y0[0] != 0)  # a condition on the inputs: a x[0] >> u |y[0]|
    y, x = y0.to(dev()).clone(), x0.to(dev()).clone()
    axpy(y, x, a)
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), x0)
    worst, nfail, first = ac.check_axpy(y0, x0, a, y.cpu())
    print(f"\naxpy n {n} a {a}: worst error / bar {worst:.3f}")
    assert nfail == 0, (worst, nfail, first)
    assert bool(y.cpu()[0] != y0[0])  # follows from the two above; said outright for n = 1
    if a == 1.0:  # one rounding of an exact sum: the trainer's gradient sum is torch's
        assert torch.equal(y.cpu(), y0 + x0)


# ---------------------------------------------------------------------------- c, d, e
B, LR, BETAS, EPS, WD = 4, 1e-3, (0.9, 0.999), 1e-8, 1e-2
CONFIGS = [((4, 48), 1), ((4, 48), 2), ((8, 32), 1), ((8, 32), 2)]
TRAINERS = [pytest.param(c, id=f"{c[0][0]}x{c[0][1]}-micro{c[1]}") for c in CONFIGS]


def _spec():
    from srmi.engine import NetSpec
    return NetSpec(arch="rcan", nchannels_in=2, nchannels_out=2, nfeatures=64, nlayers=2, nblocks=2, scale=4)


def _trainer(tile, micro):
    from srmi.trainer import FusedTrainer
    return FusedTrainer(_spec(), B, tile, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, interp_loss=False,
                        device=dev(), seed=3, micro=micro)


def _packs_are_current(tr, lrfix):
    """Every engine's forward of lrfix equals, bit for bit, that of a fresh Engine of the same
    capacity and cu_budget packed with tr.params -> the engines that differ."""
    from srmi.engine import Engine
    stale = []
    for k, eng in enumerate(tr.engines):
        got = eng.forward(tr.params, lrfix).clone()
        fresh = Engine(tr.spec, eng.batch, (eng.lr_h, eng.lr_w), train=True, device=tr.device,
                       cu_budget=eng._cfg.cu_budget)
        fresh.pack(tr.params)
        want = fresh.forward(tr.params, lrfix)
        torch.cuda.synchronize()
        if not torch.equal(got, want):
            stale.append((k, float((got - want).abs().max())))
    return stale


def _snap(tr):
    torch.cuda.synchronize()
    return tr.params.cpu().clone(), tr.m.cpu().clone(), tr.v.cpu().clone()


def _against(got, want, bar, table, p0):
    """The library's (p, m, v) against torch's within `bar` -> {class: compare()'s tuple}, and
    under "rel" the deviation of v and of the update p' - p0 in relative terms (reported only)."""
    out = {c: ac.compare(x, y, bar[c], table) for c, x, y in zip("pmv", got, want)}
    out["rel"] = (ac.rel_size(got[2], want[2], bar["v"], want[2]),
                  ac.rel_size(got[0], want[0], bar["p"], want[0].double() - p0.double()))
    return out


@functools.lru_cache(maxsize=None)
def _run(tile, micro):
    tr = _trainer(tile, micro)
    table, hp = tr.eng.table, ac.hyper(LR, BETAS, EPS, WD)
    gen = torch.Generator().manual_seed(17 + tile[0])
    s = tr.spec.scale
    hr = torch.randn(B, 2, tile[0] * s, tile[1] * s, generator=gen).to(dev())
    lrfix = torch.randn(B // micro, 2, *tile, generator=gen).to(dev())
    out = dict(table=table, closure=[], stale=[], torch=[])
    opt = ps = prev = None
    for t in (1, 2, 3):
        p0, m0, v0 = _snap(tr)
        tr.step(hr)
        post = _snap(tr)
        g = tr.grads.cpu().clone()
        pre = (p0, g, m0, v0)
        out["closure"].append(ac.check_step(pre, post, t, hp, table))
        out["stale"].append(_packs_are_current(tr, lrfix))
        if opt is not None:  # d: torch from the checkpoint after step 1, the engine's own gradients
            prev = ac.torch_bars(pre, t, hp, LR, BETAS, prev)
            out["torch"].append(_against(post, ac.torch_adam_step(opt, ps, table, g), prev, table, p0))
        if t == 1:
            ck = tr.checkpoint()
            opt, ps = ac.torch_adam(table, ck["model_state_dict"], ck["optimizer_state_dict"])
    # e: resume at step 20000
    ck = tr.checkpoint()
    for st in ck["optimizer_state_dict"]["state"].values():
        st["step"] = (torch.full_like(st["step"], 20000) if torch.is_tensor(st["step"])
                      else type(st["step"])(20000))
    tr2 = _trainer(tile, micro)
    tr2.load_checkpoint(ck)
    opt, ps = ac.torch_adam(table, ck["model_state_dict"], ck["optimizer_state_dict"])
    p0, m0, v0 = _snap(tr2)
    assert all(torch.equal(x, y) for x, y in zip((p0, m0, v0), post)) and tr2.t == 20000
    tr2.step(hr)
    post = _snap(tr2)
    g = tr2.grads.cpu().clone()
    pre = (p0, g, m0, v0)
    out["resume_t"] = tr2.t
    out["resume_closure"] = ac.check_step(pre, post, 20001, hp, table)
    out["resume_stale"] = _packs_are_current(tr2, lrfix)
    out["resume_torch"] = _against(post, ac.torch_adam_step(opt, ps, table, g),
                                   ac.torch_bars(pre, 20001, hp, LR, BETAS), table, p0)
    print(f"\ntrainer {tile} micro {micro}: {tr.eng.n_params} parameters")
    for t, rep in enumerate(out["closure"] + [out["resume_closure"]], start=1):
        print(f" closure step {t if t < 4 else 20001}\n" + "\n".join(rep.lines()))
    for t, w in zip((2, 3, 20001), out["torch"] + [out["resume_torch"]]):
        (vm, vb, vmed, vbmed), (um, ub, umed, ubmed) = w["rel"]
        print(f" against torch.optim.Adam step {t}: "
              + " ".join(f"{c} {w[c][0]:.3f} ({w[c][3]})" for c in "pmv")
              + f"\n  v relative: worst {vm:.2e} (bar there {vb:.2e}), median {vmed:.2e} (bar {vbmed:.2e});"
              + f" update relative: median {umed:.2e} (bar {ubmed:.2e})")
    return out


@pytest.mark.parametrize("c", TRAINERS)
def test_trainer_update_closes(c):
    """(c) Every step's (params, m, v) from (p0, tr.grads, m0, v0, t), the worst tensor by name."""
    out = _run(*c)
    assert len(out["closure"]) == 3
    for t, rep in enumerate(out["closure"], start=1):
        assert not rep.failed(), (t, rep.lines())


@pytest.mark.parametrize("c", TRAINERS)
def test_every_engine_repacks_the_new_weights(c):
    """(c) After every step (and after the resumed one) every engine's packs are the packs of the
    new master weights: its forward equals a fresh engine's bit for bit."""
    out = _run(*c)
    assert out["stale"] == [[], [], []] and out["resume_stale"] == [], (out["stale"], out["resume_stale"])


@pytest.mark.parametrize("c", TRAINERS)
def test_trainer_against_torch_adam(c):
    """(d) Steps 2 and 3 against torch.optim.Adam(weight_decay=1e-2) loaded from the checkpoint
    after step 1 and fed the engine's own gradients.  The bar (adam_closure.torch_bars; its module
    docstring has the derivation in full): the library is an Adam with beta = float32(beta), so with
    db = float32(beta) - beta, from the same pre-step state and to first order, m' differs from
    torch's by |db1| |g' - m|, v' by |db2| (v + g'^2), bc2 by t bmax^(t-1) |db2| / bc2 relative
    (mean value theorem) = |db2| / (1 - beta2) = 1.3e-5 for t <= 3, and ss = lr / bc1 likewise by
    |db1| / (1 - beta1) = 2.4e-7 plus lr's own float rounding.  These go through the step linearly:
    the root sqrt(v' / bc2) takes half the relative change of v' and of bc2, q = m' / den takes
    dm / den + |q| dden / den, p takes ss dq + |ss q| rel(ss).  Added to them: the closure bar twice
    (the library's fp32 arithmetic and torch's, which performs the same operations), torch's double
    scalars rounded to fp32 inside its kernels (u each), and at step 3 the bar of step 2 carried
    through the same linear response (torch's step 3 starts from torch's step 2).  Nothing in it is
    fitted: v sits near 0.9 of it because the float-beta offset is systematic."""
    out = _run(*c)
    assert len(out["torch"]) == 2
    for w in out["torch"]:
        assert all(w[c][1] == 0 for c in "pmv"), w


@pytest.mark.parametrize("c", TRAINERS)
def test_resume_at_a_large_step(c):
    """(e) One step from a checkpoint at step 20000: the closure bar, and torch_bars against
    torch.optim.Adam loaded from the same dict, the float-beta term taken at t = 20001.  There the
    bias corrections' share, t bmax^(t-1) |db| / bc -- which grows like t |db| / beta while
    beta^t ~ 1 and peaks near t = 1 / (1 - beta) -- has vanished with beta^t (0.999^20000 = 2e-9:
    5e-13 relative in bc2, 0 in bc1), and what is left of the term is the one-step change of the
    moments themselves, |db1| |g' - m| and |db2| (v + g'^2), through the same linear response."""
    out = _run(*c)
    assert out["resume_t"] == 20001
    assert not out["resume_closure"].failed(), out["resume_closure"].lines()
    assert all(out["resume_torch"][c][1] == 0 for c in "pmv"), out["resume_torch"]
