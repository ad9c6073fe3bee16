"""The checkers of tests/adam_closure.py, fed from the CPU (no GPU): the op-by-op fp32 restatement
of adam_kernel sits inside every bar, close to the bar of p (its last half ulp is reached); each way
the update could be subtly wrong (adam_closure.MUTATIONS) fails exactly the classes named, by a
clear margin; and the derived bar against the real torch.optim.Adam holds for the restatement over
compounding steps, from step 1 and from a resumed step of 20000.

A mutation that corrupts m' or v' inside the kernel fails p as well: the kernel forms p from its
own m' and v', and p is checked from the pre-step operands like the moments."""
import functools

import pytest
import torch

import adam_closure as ac

N = 200_000
STEPS = [1, 2, 3, 1000, 100000]
WDS = [0.0, 1e-2]


@functools.lru_cache(maxsize=None)
def _inputs(n, step):
    return ac.make_inputs(n, step)


@functools.lru_cache(maxsize=None)
def _report(n, step, wd, mut=0, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
    hp = ac.hyper(lr, betas, eps, wd)
    pre = _inputs(n, step)
    return ac.check_step(pre, ac.restate_fp32(*pre, step, hp, mut), step, hp)


@pytest.mark.parametrize("wd", WDS)
@pytest.mark.parametrize("step", STEPS)
def test_restatement_sits_inside_every_bar(step, wd):
    rep = _report(N, step, wd)
    print(f"\nstep {step} wd {wd}\n" + "\n".join(rep.lines()))
    assert not rep.failed()
    # the inputs reach what they are for: elements whose root is comparable to eps (without decay:
    # wd p ~ 5e-4 lifts every g' far above eps), and exact zeros
    r = ac.reference(*_inputs(N, step), step, ac.hyper(wd=wd))
    root = r["den"] - r["hp"]["eps"]
    if wd == 0.0:
        assert int(((root > 0.1 * r["hp"]["eps"]) & (root < 10 * r["hp"]["eps"])).sum()) > N // 100
    assert int((r["g"] == 0).sum()) >= N // 7
    assert not bool(((r["g"] != 0) & (r["g"].abs() < 1e-10)).any())


def test_restatement_reaches_the_bar_of_p():
    """A bar nobody comes near checks nothing: over the cases the worst p error is above 0.8 of its
    bar (the final half ulp of p), m and v above a third of theirs."""
    reps = [_report(N, s, w) for s in STEPS for w in WDS]
    worst = {c: max(r.worst(c) for r in reps) for c in ("m", "v", "p")}
    print(worst)
    assert worst["p"] > 0.8 and worst["m"] > 1 / 3 and worst["v"] > 1 / 3


def test_non_default_hyper_parameters():
    rep = _report(N, 3, 1e-2, 0, 5e-5, (0.8, 0.99), 1e-6)
    print("\n".join(rep.lines()))
    assert not rep.failed()


#   mutation, step, wd, n, the classes that must fail (no other may)
BIG = ac.GRID_SPAN + 777
MUTANTS = [
    (1, 1, 1e-2, N, {"m", "v", "p"}),
    (1, 1000, 1e-2, N, {"m", "v", "p"}),
    (2, 1, 0.0, N, {"p"}),
    (2, 3, 1e-2, N, {"p"}),
    (2, 1000, 0.0, N, {"p"}),
    (3, 1, 0.0, N, {"p"}),
    (3, 3, 1e-2, N, {"p"}),
    (3, 1000, 0.0, N, {"p"}),
    (4, 2, 0.0, N, {"p"}),
    (4, 3, 1e-2, N, {"p"}),
    (5, 1, 0.0, N, {"v", "p"}),      # p is formed from the kernel's own v'
    (5, 1000, 1e-2, N, {"v", "p"}),
    (6, 1, 1e-2, N, {"m", "p"}),     # and from its own m'
    (6, 1000, 1e-2, N, {"m", "p"}),
    (7, 3, 1e-2, BIG, {"m", "v", "p"}),
    (8, 3, 0.0, N, {"v", "moved"}),  # p and m are right: only the store of v is missing
    (8, 1, 1e-2, N, {"v", "moved"}),
]


@pytest.mark.parametrize("mut,step,wd,n,classes", MUTANTS,
                         ids=[f"m{m}-t{s}-wd{w:g}-n{n}" for m, s, w, n, _ in MUTANTS])
def test_mutation_fails_its_classes(mut, step, wd, n, classes):
    rep = _report(n, step, wd, mut)
    print(ac.MUTATIONS[mut], "->", sorted(rep.failed()))
    print("\n".join(rep.lines()))
    assert rep.failed() == classes
    for cls in classes - {"moved"}:
        (row,) = rep.failures(cls)
        assert row[1] > 100.0, row          # a clear margin: two orders past the bar
        if mut == 7:                        # named by index: exactly the loop's second trip
            assert row[3] > 700 and row[4] >= ac.GRID_SPAN, row
    if mut == 8:
        assert rep.worst("moved") == 0.0


def test_compare_fails_a_non_finite_value():
    want = torch.ones(8)
    got = want.clone()
    got[5] = float("nan")
    worst, nfail, first, _ = ac.compare(got, want, torch.full((8,), 1e-3, dtype=torch.float64))
    assert (nfail, first) == (1, 5) and worst == float("inf")


def test_the_first_element_is_never_a_zero():
    """n = 1 is element 0 alone: g, and past step 1 m and v, are non-zero there."""
    for step in (1, 2, 3, 1000, 100000):
        p, g, m, v = ac.make_inputs(1, step)
        assert bool(p[0] != 0) and bool(g[0] != 0)
        assert step == 1 or (bool(m[0] != 0) and bool(v[0] != 0))


def test_the_zero_step_is_exact():
    """g = 0, m = v = 0, wd = 0: every bar but p's half ulp is 0 and the restatement meets them."""
    n = 1000
    p = ac.make_inputs(n, 1)[0]
    z = torch.zeros(n)
    hp = ac.hyper()
    pn, mn, vn = ac.restate_fp32(p, z, z, z, 1, hp)
    assert torch.equal(pn, p) and not mn.any() and not vn.any()
    rep = ac.check_step((p, z, z, z), (pn, mn, vn), 1, hp)
    assert not rep.failed()


def test_axpy_checker():
    g = torch.Generator().manual_seed(3)
    y0, x = torch.randn(5000, generator=g), torch.randn(5000, generator=g)
    for a in (1.0, -0.37):
        y1 = y0 + ac.f32(a) * x
        worst, nfail, _ = ac.check_axpy(y0, x, a, y1)
        assert nfail == 0 and worst <= 1.0
        y1[4321] += 4e-7 * max(1.0, float(y1[4321].abs()))
        worst, nfail, first = ac.check_axpy(y0, x, a, y1)
        assert (nfail, first) == (1, 4321)


# ------------------------------------------------------------------- torch.optim.Adam
TABLE = [("a.weight", 0, 3000, (30, 100)), ("a.bias", 3000, 30, (30,)), ("b.weight", 3030, 970, (970,))]
LR, BETAS, EPS, WD = 1e-3, (0.9, 0.999), 1e-8, 1e-2


def _opt_sd(m, v, step):
    from srmi import checkpoint as ckpt
    return ckpt.adam_state_dict(TABLE, m, v, step, LR, BETAS, EPS, WD)


def _state(p):
    return {name: p[off:off + n].view(shape) for name, off, n, shape in TABLE}


@pytest.mark.parametrize("t0", [1, 20000])
def test_torch_bar_holds_and_is_not_slack(t0):
    """From a state at step t0 (as a checkpoint holds it) the restatement and a real CPU
    torch.optim.Adam take the same gradients for two steps; the restatement stays inside
    torch_bars (compounding through `prev`), and v's deviation -- the float beta2 -- is a fixed
    fraction of its bar, not rounding noise below it."""
    n = 4000
    p, _, m, v = ac.make_inputs(n, 5, seed=11)
    hp = ac.hyper(LR, BETAS, EPS, WD)
    opt, ps = ac.torch_adam(TABLE, _state(p), _opt_sd(m, v, t0))
    prev = None
    for k in (1, 2):
        g = ac.make_inputs(n, 5, seed=20 + k)[1]
        pre = (p, g, m, v)
        bar = ac.torch_bars(pre, t0 + k, hp, LR, BETAS, prev)
        p, m, v = ac.restate_fp32(*pre, t0 + k, hp)
        tp, tm, tv = ac.torch_adam_step(opt, ps, TABLE, g)
        worst = {c: ac.compare(x, y, bar[c], TABLE) for c, x, y in (("p", p, tp), ("m", m, tm), ("v", v, tv))}
        print(t0 + k, {c: (f"{w[0]:.3f}", w[1]) for c, w in worst.items()})
        assert all(w[1] == 0 for w in worst.values()), worst
        if k == 1:
            assert worst["v"][0] > 0.2
        prev = bar


def test_float_beta_term_sizes():
    """The sizes the derivation states: |db2| / c2 = 1.3e-5 at t <= 3, vanishing at t = 20001."""
    hp = ac.hyper()
    for t in (1, 2, 3):
        assert 1.2e-5 < ac.float_beta_rel(hp["b2"], 0.999, t) < 1.4e-5
        assert ac.float_beta_rel(hp["b1"], 0.9, t) < 3e-7
    assert ac.float_beta_rel(hp["b2"], 0.999, 20001) < 1e-12
    assert ac.float_beta_rel(hp["b1"], 0.9, 20001) == 0.0
    # the largest the term gets, near t = 1 / (1 - beta): t db / b in size
    t = 1000
    assert 0.5 * t * 1.3e-8 / 0.999 * 0.999 ** t / (1 - 0.999 ** t) < ac.float_beta_rel(hp["b2"], 0.999, t) < 2e-5
