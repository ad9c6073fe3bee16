"""The optimizer guards on the device ("Optimizer guards") against
tests/optim_oracle.py, every bar derived there or in tests/adam_closure.py:

 1. srmi_grad_norm: the norm of gradients whose squares overflow fp32, within 2^-22 of fp64, at
    n = 1, 255, 256, 257, 1027 and 8192 * 256 * 4 + 3 (the grid-stride loop wraps and leaves an
    unaligned tail), from a slice that starts 1 and 3 elements off a 16-byte boundary, the same
    bits on a second run.
 2. The clip coefficient within 2^-22 of the fp64 formula, exactly 1 when norm + 1e-6 <= max_norm
    and at max_norm = inf.
 3. One NaN, one +inf, at the first, a middle and the last element: the finite flag clears, the
    count runs across calls, srmi_adam_step_guarded leaves p, m, v, ema bit for bit; max_norm 0,
    negative or NaN is SRMI_ERR_ARG and nothing is launched.
 4. The guarded step closes through adam_closure.check_step on g' = fl(g ctl[1]) with the device's
    own coefficient, steps 1, 2, 1000, weight_decay 0 and 1e-2; at ctl[1] = 1 without an average
    it is srmi_adam_step bit for bit.
 5. The average closes against the fp64 lerp from the device's own new p within three fp32
    roundings of |ema| + |p| (optim_oracle.EMA bar), decay 0, 0.9, 0.999 and the warm-up's.
 6. FusedTrainer: clip_norm = 1e30 is the default trainer bit for bit; a clipped step closes from
    the trainer's own grads and ctl; a NaN HR pixel skips the step (everything bit-unchanged, the
    count 1) and the next clean step is Adam's step 3; a step schedule's third step closes at
    lr / 2; an EDSR and a land=True trainer (norm and skip); a one-rank data-parallel group under
    both reducer settings.
 7. A checkpoint saved and loaded into a fresh trainer steps bit-identically, the average and the
    skipped count included.
 8. train_timeslices over two tiny time slices, one holding a NaN tile.
"""
import functools
import io
import math
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import adam_closure as ac  # noqa: E402
import optim_oracle as oo  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 8192 * 256 * 4 + 3
NS = [1, 255, 256, 257, 1027, BIG]
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same(a, b):
    return torch.equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def _wide(n):
    """(the gradient on the host, its fp64 norm): computed once, never written."""
    g = oo.wide_gradient(n)
    g.setflags(write=False)
    return g, oo.norm(g)


def _norm(g_dev, max_norm=math.inf, ctl=None):
    """One srmi_grad_norm -> ctl on the host (fp32 numpy), after a synchronize."""
    from srmi.engine import grad_norm
    if ctl is None:
        ctl = torch.zeros(4, device=dev())
    grad_norm(g_dev, ctl, max_norm)
    torch.cuda.synchronize()
    return ctl.cpu().numpy()


# ---------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("n", NS)
def test_norm_closes_and_is_deterministic(n):
    g, want = _wide(n)
    with np.errstate(over="ignore"):
        assert not np.isfinite(np.float32(g[0]) * np.float32(g[0]))  # an fp32 square overflows
    gd = torch.from_numpy(g.copy()).to(dev())
    a, b = _norm(gd), _norm(gd)
    rel = abs(float(a[0]) - want) / want
    print(f"\nnorm n {n}: {float(a[0]):.9e} against {want:.9e}, relative {rel:.3e} (bar {oo.NORM_BAR:.3e})")
    assert math.isfinite(float(a[0])) and rel <= oo.NORM_BAR
    assert a[2] == 1.0 and a[3] == 0.0
    assert a.tobytes() == b.tobytes()
    assert torch.equal(gd.cpu(), torch.from_numpy(g.copy()))  # the gradient is read only


@pytest.mark.parametrize("off", [1, 3])
@pytest.mark.parametrize("n", [2, 1027, 70001])
def test_norm_from_a_slice_off_the_16_byte_boundary(n, off):
    g, want = _wide(n)
    buf = torch.full((n + 8,), float("nan"), device=dev())  # what lies around the slice must not be read
    assert buf.data_ptr() % 16 == 0
    buf[off:off + n] = torch.from_numpy(g.copy()).to(dev())
    a = _norm(buf[off:off + n])
    assert a[2] == 1.0 and abs(float(a[0]) - want) / want <= oo.NORM_BAR, (a, want)


# ---------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("n", [257, 1027])
def test_clip_coefficient(n):
    g, nrm = _wide(n)
    gd = torch.from_numpy(g.copy()).to(dev())
    for factor in (1e-30, 0.37, 0.999999):
        mx = float(np.float32(factor * nrm))
        a = _norm(gd, mx)
        want = oo.clip_coef(nrm, mx)
        assert want < 1.0 and abs(float(a[1]) - want) / want <= oo.NORM_BAR, (factor, a, want)
    for mx in (float(np.float32(nrm * 1.000001)), 3e38, math.inf):  # norm + 1e-6 <= max_norm
        assert nrm + 1e-6 <= mx
        a = _norm(gd, mx)
        assert a[1] == 1.0 and a[2] == 1.0, (mx, a)


# ---------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("n", [1027, BIG])
def test_a_non_finite_element_skips_the_step(n):
    from srmi.engine import adam_step_guarded
    g, _ = _wide(n)
    gd = torch.from_numpy(g.copy()).to(dev())
    gen = torch.Generator().manual_seed(n)
    state0 = [torch.randn(n, generator=gen).to(dev()) for _ in range(4)]  # p, m, v (its sign is never looked at), ema
    state = [x.clone() for x in state0]
    ctl = torch.zeros(4, device=dev())
    calls = 0
    for bad in (math.nan, math.inf):
        for where in (0, n // 2, n - 1):
            keep = gd[where].clone()
            gd[where] = bad
            a = _norm(gd, 1.0, ctl)
            calls += 1
            assert a[2] == 0.0 and a[3] == float(calls) and not math.isfinite(float(a[0])), (bad, where, a)
            adam_step_guarded(state[0], gd, state[1], state[2], ctl, 3, LR, BETAS, EPS, 1e-2, ema=state[3],
                              ema_decay=0.9)
            adam_step_guarded(state[0], gd, state[1], state[2], ctl, 3, LR, BETAS, EPS, 0.0)
            torch.cuda.synchronize()
            assert all(same(x, y) for x, y in zip(state, state0)), (bad, where)
            gd[where] = keep
    a = _norm(gd, 1.0, ctl)  # a clean gradient: the flag comes back, the count stays
    assert a[2] == 1.0 and a[3] == float(calls)


@pytest.mark.parametrize("max_norm", [0.0, -1.0, math.nan, -math.inf])
def test_a_bad_max_norm_is_refused_and_nothing_is_launched(max_norm):
    from srmi._lib import SrmiError
    from srmi.engine import grad_norm
    gd = torch.from_numpy(_wide(1027)[0].copy()).to(dev())
    ctl = torch.tensor([5.0, 6.0, 7.0, 8.0], device=dev())
    with pytest.raises(SrmiError, match="SRMI_ERR_ARG"):
        grad_norm(gd, ctl, max_norm)
    torch.cuda.synchronize()
    assert ctl.tolist() == [5.0, 6.0, 7.0, 8.0]


# ---------------------------------------------------------------------------------- 4
def _guarded(pre, ctl, step, wd, ema=None, decay=0.0):
    from srmi.engine import adam_step_guarded
    p, g, m, v = (x.to(dev()).clone() for x in pre)
    e = None if ema is None else ema.to(dev()).clone()
    adam_step_guarded(p, g, m, v, ctl, step, LR, BETAS, EPS, wd, ema=e, ema_decay=decay)
    torch.cuda.synchronize()
    assert torch.equal(g.cpu(), pre[1])
    return (p.cpu(), m.cpu(), v.cpu()) + (() if e is None else (e.cpu(),))


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("step", [1, 2, 1000])
def test_guarded_step_closes_on_the_clipped_gradient(step, wd):
    pre = ac.make_inputs(1027, step)
    gd = pre[1].to(dev())
    nrm = oo.norm(pre[1].numpy())
    ctl = torch.zeros(4, device=dev())
    a = _norm(gd, float(np.float32(0.37 * nrm)), ctl)
    coef = float(a[1])
    assert 0.36 < coef < 0.38 and a[2] == 1.0
    post = _guarded(pre, ctl, step, wd)
    rep = oo.check_clipped_step(pre, post, step, ac.hyper(LR, BETAS, EPS, wd), coef)
    print(f"\nguarded step {step} wd {wd} coef {coef:.8f}\n" + "\n".join(rep.lines()))
    assert not rep.failed(), rep.lines()
    # the unclipped gradient does not close: the coefficient was applied
    assert ac.check_step(pre, post, step, ac.hyper(LR, BETAS, EPS, wd)).failed()


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("n,step", [(1027, 1), (1027, 2), (1027, 1000), (ac.GRID_SPAN + 777, 3)])
def test_guarded_step_at_coefficient_one_is_adam_step_bit_for_bit(n, step, wd):
    from srmi.engine import adam_step
    pre = ac.make_inputs(n, step)
    ctl = torch.tensor([1.0, 1.0, 1.0, 0.0], device=dev())
    got = _guarded(pre, ctl, step, wd)
    p, g, m, v = (x.to(dev()).clone() for x in pre)
    adam_step(p, g, m, v, step, LR, BETAS, EPS, wd)
    torch.cuda.synchronize()
    assert all(same(x, y.cpu()) for x, y in zip(got, (p, m, v)))
    assert not same(got[0], pre[0])


# ---------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("decay", [0.0, 0.9, 0.999] + [oo.ema_decay_at(0.999, True, t) for t in (1, 2, 3)])
@pytest.mark.parametrize("n", [1027, ac.GRID_SPAN + 777])
def test_ema_closes(n, decay):
    """Bar (optim_oracle's docstring): e' = e + c (p' - e) with c = fl(1 - fl(decay)) takes three
    fp32 roundings -- the difference, the product, the sum -- each at most u (|e| + |p'|), since
    c <= 1 and e' lies between e and p'; a contraction removes one.  3 u (|e| + |p'|)."""
    pre = ac.make_inputs(n, 3)
    gen = torch.Generator().manual_seed(n + 1)
    ema0 = (pre[0].double() + 0.01 * torch.randn(n, generator=gen, dtype=torch.float64)).float()
    ctl = torch.tensor([1.0, 1.0, 1.0, 0.0], device=dev())
    p, m, v, e = _guarded(pre, ctl, 3, 1e-2, ema=ema0, decay=decay)
    plain = _guarded(pre, ctl, 3, 1e-2)
    assert all(same(x, y) for x, y in zip((p, m, v), plain))  # the average changes nothing else
    worst, nfail = oo.check_ema(ema0.numpy(), p.numpy(), decay, e.numpy())
    print(f"\nema n {n} decay {decay:.6f}: worst error / bar {worst:.3f}")
    assert nfail == 0, (worst, nfail)
    assert oo.check_ema(ema0.numpy(), p.numpy(), decay, ema0.numpy())[1] > 0  # an unmoved average fails


# ---------------------------------------------------------------------------------- 6
B, TILE, WD = 4, (48, 48), 1e-2


def _spec(arch="rcan"):
    from srmi.engine import NetSpec
    if arch == "edsr":
        return NetSpec(arch="edsr", nchannels_in=2, nchannels_out=2, nfeatures=64, nlayers=2, nblocks=0, scale=4)
    return NetSpec(arch="rcan", nchannels_in=2, nchannels_out=2, nfeatures=64, nlayers=2, nblocks=2, scale=4)


def _trainer(micro=1, arch="rcan", wd=WD, **kw):
    from srmi.trainer import FusedTrainer
    return FusedTrainer(_spec(arch), B, TILE, lr=LR, betas=BETAS, eps=EPS, weight_decay=wd, interp_loss=False,
                        device=dev(), seed=3, micro=micro, **kw)


@functools.lru_cache(maxsize=None)
def _tiles(seed=17):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(B, 2, TILE[0] * 4, TILE[1] * 4, generator=gen).to(dev())


def _snap(tr):
    torch.cuda.synchronize()
    out = [tr.params.cpu().clone(), tr.m.cpu().clone(), tr.v.cpu().clone()]
    if tr.ema is not None:
        out.append(tr.ema.cpu().clone())
    return out


def _norm_of_grads(tr, out):
    """out["grad_norm"] against the fp64 norm of the trainer's own grads, at the case-1 bar."""
    torch.cuda.synchronize()
    want = oo.norm(tr.grads.cpu().numpy())
    got = float(out["grad_norm"])
    assert got == float(tr.ctl[0]) and abs(got - want) <= oo.NORM_BAR * want, (got, want)
    return want


@pytest.mark.parametrize("micro", [1, 2])
def test_a_huge_clip_norm_is_the_default_trainer_bit_for_bit(micro):
    a, b = _trainer(micro), _trainer(micro, clip_norm=1e30)
    assert a.ctl is None and a.ema is None and b.guard and b.ema is None
    for t in range(3):
        oa, ob = a.step(_tiles(17 + t)), b.step(_tiles(17 + t))
        assert "grad_norm" not in oa and set(ob) == set(oa) | {"grad_norm", "step_skipped"}
        assert float(ob["step_skipped"]) == 1.0 and float(b.ctl[1]) == 1.0
        assert same(oa["loss"], ob["loss"])
    assert all(same(x, y) for x, y in zip(_snap(a), _snap(b)))
    assert b.skipped_steps() == 0 and a.skipped_steps() == 0


@functools.lru_cache(maxsize=None)
def _measured_norm(micro):
    tr = _trainer(micro, guard=True)
    out = tr.step(_tiles())
    nrm = _norm_of_grads(tr, out)
    assert float(out["step_skipped"]) == 1.0 and float(tr.ctl[1]) == 1.0  # guard alone never clips
    return nrm


@pytest.mark.parametrize("micro", [1, 2])
def test_trainer_clips_skips_and_counts_the_skipped_step(micro):
    nrm = _measured_norm(micro)
    tr = _trainer(micro, clip_norm=0.5 * nrm, ema=dict(decay=0.999, warmup=True))
    hp, table = ac.hyper(LR, BETAS, EPS, WD), tr.eng.table
    assert same(tr.ema, tr.params) and tr.ema.data_ptr() != tr.params.data_ptr()
    assert tr.eval_params() is tr.params and tr.eval_params(ema=True) is tr.ema
    # step 1: clipped, closes from the trainer's own grads and ctl
    pre = _snap(tr)
    out = tr.step(_tiles())
    post = _snap(tr)
    _norm_of_grads(tr, out)
    coef = float(tr.ctl[1])
    assert abs(coef - 0.5) < 1e-3 and float(out["step_skipped"]) == 1.0
    g = tr.grads.cpu().clone()
    rep = oo.check_clipped_step((pre[0], g, pre[1], pre[2]), post[:3], 1, hp, coef, table)
    assert not rep.failed(), rep.lines()
    assert oo.check_ema(pre[3].numpy(), post[0].numpy(), oo.ema_decay_at(0.999, True, 1), post[3].numpy())[1] == 0
    # step 2: a NaN in one HR pixel
    hr = _tiles(18).clone()
    hr[1, 0, 100, 7] = float("nan")
    out = tr.step(hr)
    torch.cuda.synchronize()
    assert float(out["step_skipped"]) == 0.0 and not math.isfinite(float(out["grad_norm"]))
    assert all(same(x, y) for x, y in zip(_snap(tr), post))
    assert tr.skipped_steps() == 1 and tr.t == 2
    # step 3: clean; the skipped step consumed its number
    pre = post
    out = tr.step(_tiles(19))
    post = _snap(tr)
    coef = float(tr.ctl[1])
    g = tr.grads.cpu().clone()
    assert float(out["step_skipped"]) == 1.0 and tr.skipped_steps() == 1 and tr.t == 3
    rep = oo.check_clipped_step((pre[0], g, pre[1], pre[2]), post[:3], 3, hp, coef, table)
    assert not rep.failed(), rep.lines()
    assert oo.check_clipped_step((pre[0], g, pre[1], pre[2]), post[:3], 2, hp, coef, table).failed()
    assert oo.check_ema(pre[3].numpy(), post[0].numpy(), oo.ema_decay_at(0.999, True, 3), post[3].numpy())[1] == 0
    sd = tr.ema_state_dict()
    assert list(sd) == list(tr.state_dict()) and same(torch.cat([x.reshape(-1) for x in sd.values()]), post[3])


@pytest.mark.parametrize("guard", [None, True])
def test_step_schedule_third_step_runs_at_half_the_rate(guard):
    tr = _trainer(1, lr_schedule=dict(kind="step", step_size=2, gamma=0.5), guard=guard)
    table = tr.eng.table
    rates = []
    for t in (1, 2, 3):
        rates.append(tr.current_lr())
        pre = _snap(tr)
        tr.step(_tiles(17 + t))
        post = _snap(tr)
        g = tr.grads.cpu().clone()
        rep = ac.check_step((pre[0], g, pre[1], pre[2]), post[:3], t, ac.hyper(rates[-1], BETAS, EPS, WD), table)
        assert not rep.failed(), (t, rep.lines())
        if t == 3:  # and not at the base rate
            assert ac.check_step((pre[0], g, pre[1], pre[2]), post[:3], t, ac.hyper(LR, BETAS, EPS, WD), table).failed()
    assert rates == [LR, LR, LR / 2] and tr.current_lr() == LR / 2
    assert tr.checkpoint()["optimizer_state_dict"]["param_groups"][0]["lr"] == LR  # the BASE rate


def test_edsr_norm_and_skip():
    tr = _trainer(1, arch="edsr", guard=True)
    out = tr.step(_tiles())
    _norm_of_grads(tr, out)
    assert float(out["step_skipped"]) == 1.0
    post = _snap(tr)
    hr = _tiles(18).clone()
    hr[3, 1, 0, 0] = float("nan")
    out = tr.step(hr)
    torch.cuda.synchronize()
    assert float(out["step_skipped"]) == 0.0 and tr.skipped_steps() == 1
    assert all(same(x, y) for x, y in zip(_snap(tr), post))


def test_land_norm_and_skip():
    """land=True: NaN pixels are the mask, not a fault -- a coastal batch steps, and its norm is
    the fp64 norm of its gradient; so does a batch that is dry throughout (its upstream gradient
    is zero everywhere, and so is the step's: nothing to guard against).  What the mask cannot
    hide is a weight that has become NaN: every feature map is NaN, the filter gradients are
    NaN * 0, and the step is skipped instead of spreading it into m and v."""
    tr = _trainer(1, guard=True, land=True)
    hr = _tiles().clone()
    hr[:, :, :40, :56] = float("nan")
    pre = _snap(tr)
    out = tr.step(hr)
    _norm_of_grads(tr, out)
    post = _snap(tr)
    assert float(out["step_skipped"]) == 1.0 and tr.skipped_steps() == 0 and not same(post[0], pre[0])
    out = tr.step(torch.full_like(hr, float("nan")))
    _norm_of_grads(tr, out)
    assert float(out["step_skipped"]) == 1.0 and tr.skipped_steps() == 0
    tr.params[0] = float("nan")  # (the head conv's first filter tap)
    for e in tr.engines:
        e.pack(tr.params)
    post = _snap(tr)
    out = tr.step(hr)
    torch.cuda.synchronize()
    assert float(out["step_skipped"]) == 0.0 and tr.skipped_steps() == 1
    assert all(same(x, y) for x, y in zip(_snap(tr), post))


def _dp_worker(port, q, reducer_stream, clip):
    import sys
    sys.path[:0] = [os.path.join(ROOT, "super-resolution-climate_amd"), ROOT, os.path.join(ROOT, "tests")]
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        os.environ.pop(k, None)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    from srmi.dist import init_from_env
    info = init_from_env("nccl", force=True)
    assert info.enabled
    dp = _trainer(2, clip_norm=clip, info=info, dp_reducer_stream=reducer_stream)
    ref = _trainer(2, clip_norm=clip)
    pre = _snap(dp)
    a, b = dp.step(_tiles()), ref.step(_tiles())
    post = _snap(dp)
    want = oo.norm(dp.grads.cpu().numpy())
    coef = float(dp.ctl[1])
    rep = oo.check_clipped_step((pre[0], dp.grads.cpu(), pre[1], pre[2]), post[:3], 1, ac.hyper(LR, BETAS, EPS, WD), coef)
    q.put(dict(norm=float(a["grad_norm"]), want=want, coef=coef, kept=float(a["step_skipped"]),
               ctl_equal=same(dp.ctl, ref.ctl), state_equal=all(same(x, y) for x, y in zip(post, _snap(ref))),
               failed=sorted(rep.failed()), lines=rep.lines()))
    dist.destroy_process_group()


@pytest.mark.parametrize("reducer_stream", [False, True])
def test_one_rank_data_parallel_group_norm_and_clipped_step(reducer_stream):
    """The norm is taken after the bucket all-reduces have been waited for (both schedules): at
    one rank the all-reduce is the identity, so ctl and the state equal the non-DP trainer's bit
    for bit, and the step closes from the rank's own grads and ctl."""
    import multiprocessing as mp
    clip = 0.5 * _measured_norm(2)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_dp_worker, args=(35000 + random.randint(0, 2000), q, reducer_stream, clip))
    p.start()
    r = q.get(timeout=240)
    p.join(timeout=60)
    assert p.exitcode == 0
    assert abs(r["norm"] - r["want"]) <= oo.NORM_BAR * r["want"] and abs(r["coef"] - 0.5) < 1e-3 and r["kept"] == 1.0
    assert r["ctl_equal"] and r["state_equal"] and not r["failed"], r


# ---------------------------------------------------------------------------------- 7
def test_checkpoint_round_trip_steps_bit_identically():
    kw = dict(clip_norm=0.5 * _measured_norm(1), ema=dict(decay=0.9, warmup=False),
              lr_schedule=dict(kind="cosine", t_max=10, warmup=2, warmup_start=0.5))
    a = _trainer(1, **kw)
    a.step(_tiles())
    hr = _tiles(18).clone()
    hr[0, 0, 0, 0] = float("nan")
    a.step(hr)  # skipped
    a.step(_tiles(19))
    state = a.checkpoint(epoch=1, itime=0, loss=0.5)
    assert state["srmi_optimizer"] == dict(skipped=1, ema_decay=0.9, ema_warmup=False)
    assert state["optimizer_state_dict"]["param_groups"][0]["lr"] == LR
    buf = io.BytesIO()
    torch.save(state, buf)
    buf.seek(0)
    b = _trainer(1, **kw)
    b.load_checkpoint(torch.load(buf, map_location="cpu", weights_only=True))
    assert b.t == a.t == 3 and b.skipped_steps() == 1 and b.current_lr() == a.current_lr()
    assert all(same(x, y) for x, y in zip(_snap(a), _snap(b))) and not same(a.ema, a.params)
    oa, ob = a.step(_tiles(20)), b.step(_tiles(20))
    sa, sb = _snap(a), _snap(b)
    assert len(sa) == 4 and all(same(x, y) for x, y in zip(sa, sb))
    assert same(oa["loss"], ob["loss"]) and same(a.ctl, b.ctl) and b.skipped_steps() == 1
    # a file without the keys: the average starts at the loaded params, the count at 0
    for k in ("srmi_optimizer", "ema_state_dict"):
        state.pop(k)
    c = _trainer(1, **kw)
    c.load_checkpoint(state)
    assert same(c.ema, c.params) and c.skipped_steps() == 0 and c.t == 3
    # a trainer without an average ignores the key, and a bad record changes nothing
    d = _trainer(1)
    before = _snap(d)
    with pytest.raises(ValueError):
        d.load_checkpoint(dict(a.checkpoint(), srmi_optimizer=dict(skipped=-1)))
    assert all(same(x, y) for x, y in zip(_snap(d), before)) and d.t == 0
    d.load_checkpoint(a.checkpoint())
    assert d.ema is None and same(d.params, a.params)


# ---------------------------------------------------------------------------------- 8
def test_train_timeslices_skips_the_nan_batch(tmp_path):
    from srmi.harness import CheckpointStore, LossRecords, train_timeslices
    tr = _trainer(1, wd=0.0, guard=True)
    p0 = tr.params.clone()
    clean = torch.cat([_tiles(30), _tiles(31)])     # 8 tiles: two batches of 4
    dirty = torch.cat([_tiles(32), _tiles(33)]).clone()
    dirty[5, 1, 17, 33] = float("nan")              # one tile of the second batch
    store = CheckpointStore(str(tmp_path / "res"), "v1")
    recs = LossRecords(str(tmp_path / "rec"), "ds", "t", "m")
    out = train_timeslices(tr, [lambda: clean, lambda: dirty], 2, B, store=store, records=recs, refresh_state=True,
                           rng=random.Random(3))
    torch.cuda.synchronize()
    assert out["skipped"] == 1 and math.isfinite(out["prediction"]) and tr.t == 4
    ck = torch.load(store.path("train"), map_location="cpu", weights_only=True)
    assert all(bool(torch.isfinite(x).all()) for x in ck["model_state_dict"].values())
    assert ck["srmi_optimizer"]["skipped"] == 1 and math.isfinite(ck["loss"])
    assert not same(tr.params, p0) and bool(torch.isfinite(tr.params).all())
    rows = recs.load_results()
    assert len(rows) == 2 and len(rows[0]) == 4 and rows[1][4:] == ["skipped=1"]
    # the guard off: the result dict is what it was
    plain = train_timeslices(_trainer(1, wd=0.0), [lambda: clean], 2, B, refresh_state=True, rng=random.Random(3))
    assert set(plain) == {"prediction", "interpolated"}
