"""The optimizer guards on the CPU (no GPU): tests/optim_oracle.py against torch in fp64
(clip_grad_norm_, torch.optim.Adam on the clipped gradients, Tensor.lerp_, StepLR /
CosineAnnealingLR / LinearLR), srmi.optim's schedules against the oracle's closed forms, the
checkpoint's two extra keys on the host, the argument checks, and the new symbols' binding."""
import io
import math
import os

import numpy as np
import pytest
import torch

import adam_closure as ac
import optim_oracle as oo
from conftest import ROOT

NEW_SYMBOLS = ("srmi_grad_norm_workspace", "srmi_grad_norm", "srmi_adam_step_guarded")


def _tensors(seed=0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=gen, dtype=torch.float64) * sc
            for s, sc in (((7, 3), 1.0), ((5,), 1e-3), ((2, 2, 3, 3), 10.0), ((1,), 0.5), ((64,), 1e-6))]


# ----------------------------------------------------------------------------- norm, coefficient
@pytest.mark.parametrize("max_norm", [1e-3, 1.0, 25.0, 1e6, math.inf])
def test_norm_and_coefficient_against_clip_grad_norm(max_norm):
    """1e6 and inf lie above the norm (~ 60): the coefficient clamps to exactly 1 and the
    gradients stay bit for bit."""
    ts = _tensors()
    flat = torch.cat([t.reshape(-1) for t in ts]).numpy()
    ps = [torch.nn.Parameter(torch.zeros_like(t)) for t in ts]
    for p, t in zip(ps, ts):
        p.grad = t.clone()
    total = float(torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False))
    nrm, coef, finite, skipped = oo.ctl_record(flat, max_norm)
    assert finite == 1.0 and skipped == 0.0
    assert abs(nrm - total) <= 1e-14 * total
    got = torch.cat([p.grad.reshape(-1) for p in ps]).numpy()
    assert np.allclose(got, flat * coef, rtol=1e-14, atol=0.0)
    if max_norm >= 1e6:
        assert coef == 1.0 and np.array_equal(got, flat)
    else:
        assert coef < 1.0 and abs(oo.norm(got) - max_norm) <= 1e-6 * max_norm + 1e-6


def test_norm_does_not_overflow_where_fp32_would():
    g = oo.wide_gradient(1027)
    with np.errstate(over="ignore"):
        assert not np.isfinite(np.sqrt(np.sum(g * g, dtype=np.float32)))
    nrm = oo.norm(g)
    assert math.isfinite(nrm) and nrm >= abs(float(g[0]))
    assert abs(nrm - float(torch.linalg.vector_norm(torch.tensor(g, dtype=torch.float64)))) <= 1e-14 * nrm


@pytest.mark.parametrize("bad", [math.nan, math.inf, -math.inf])
@pytest.mark.parametrize("where", [0, 500, 1026])
def test_a_non_finite_element_clears_the_flag_and_counts(bad, where):
    g = oo.wide_gradient(1027)
    g[where] = bad
    nrm, coef, finite, skipped = oo.ctl_record(g, 1.0, skipped=2.0)
    assert not math.isfinite(nrm) and (coef, finite, skipped) == (0.0, 0.0, 3.0)


# ----------------------------------------------------------------------------- clipped Adam
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_clipped_adam_against_torch_adam_in_fp64(wd):
    """Three steps of torch.optim.Adam (fp64 parameters) behind clip_grad_norm_ against the
    oracle's clipped step chained on its own state.  The oracle runs Adam on g' = fl32(g coef)
    with coef rounded to fp32 (what the device multiplies by), torch on g coef in fp64: the
    gradients differ by 2 u relative, which the fp32 closure bars of the same step cover."""
    n, lr, betas, eps, max_norm = 301, 1e-3, (0.9, 0.999), 1e-8, 0.5
    hp = ac.hyper(lr, betas, eps, wd)
    p0, g, _, _ = ac.make_inputs(n, 1, seed=3)
    prm = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.Adam([prm], lr=hp["lr"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"], weight_decay=hp["wd"])
    p, m, v = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for t in (1, 2, 3):
        gt = ac.make_inputs(n, 1, seed=3 + t)[1] * 10.0 ** t   # a norm far above max_norm
        prm.grad = gt.double().clone()
        torch.nn.utils.clip_grad_norm_([prm], max_norm)
        opt.step()
        coef = float(np.float32(oo.ctl_record(gt.numpy(), max_norm)[1]))
        assert 0.0 < coef < 1.0
        r = oo.clipped_adam(p, gt, m, v, t, hp, coef)
        b = ac.bars(r)
        st = opt.state[prm]
        for cls, got in (("p", prm.detach()), ("m", st["exp_avg"]), ("v", st["exp_avg_sq"])):
            worst = float(ac.ratio((got - r[cls]).abs(), b[cls]).max())
            assert worst <= 1.0, (t, cls, worst)
        assert float((r["p"] - p).abs().max()) > 0
        p, m, v = prm.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()


# ----------------------------------------------------------------------------- EMA
@pytest.mark.parametrize("decay,warmup,t", [(0.0, False, 1), (0.9, False, 5), (0.999, False, 5), (0.999, True, 1),
                                            (0.999, True, 2), (0.999, True, 3), (0.5, True, 100)])
def test_ema_against_lerp(decay, warmup, t):
    from srmi.optim import check_ema, ema_decay_at
    d = oo.ema_decay_at(decay, warmup, t)
    assert d == ema_decay_at(check_ema(dict(decay=decay, warmup=warmup)), t)
    if warmup and t <= 3:
        assert d == (1.0 + t) / (10.0 + t) < decay
    gen = torch.Generator().manual_seed(t)
    e, p = torch.randn(257, generator=gen, dtype=torch.float64), torch.randn(257, generator=gen, dtype=torch.float64)
    c = float(np.float32(1.0) - np.float32(d))  # the kernel's coefficient
    want = e.clone().lerp_(p, c)
    got = oo.ema_lerp(e.numpy(), p.numpy(), d)
    # (lerp_ evaluates p - (p - e) (1 - c) for c >= 0.5: a few fp64 roundings of |e| + |p| apart)
    assert (np.abs(got - want.numpy()) <= 8 * 2.0 ** -53 * (e.abs() + p.abs()).numpy()).all()
    assert abs(c - (1.0 - d)) <= 2.0 ** -24
    # the fp32 lerp itself closes at the oracle's bar
    e32, p32 = e.float(), p.float()
    worst, nfail = oo.check_ema(e32.numpy(), p32.numpy(), d, (e32 + np.float32(c) * (p32 - e32)).numpy())
    assert nfail == 0 and worst <= 1.0
    assert oo.check_ema(e32.numpy(), p32.numpy(), d, e32.numpy())[1] > 0  # an average left unmoved fails


# ----------------------------------------------------------------------------- schedules
def _torch_rates(make, steps, lr=1e-3):
    prm = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([prm], lr=lr)
    sched = make(opt)
    out = []
    for _ in range(steps):
        out.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    return out


@pytest.mark.parametrize("cfg,make", [
    (dict(kind="step", step_size=7, gamma=0.5), lambda o: torch.optim.lr_scheduler.StepLR(o, 7, 0.5)),
    (dict(kind="cosine", t_max=49, eta_min=1e-5),
     lambda o: torch.optim.lr_scheduler.CosineAnnealingLR(o, 49, eta_min=1e-5)),
    (dict(kind="cosine", t_max=49), lambda o: torch.optim.lr_scheduler.CosineAnnealingLR(o, 49)),
    (dict(kind="constant", warmup=20, warmup_start=0.1),
     lambda o: torch.optim.lr_scheduler.LinearLR(o, start_factor=0.1, end_factor=1.0, total_iters=20)),
], ids=["StepLR", "CosineAnnealingLR", "CosineAnnealingLR-eta0", "LinearLR"])
def test_schedules_against_torch(cfg, make):
    """50 steps: the optimizer step numbered t (1-based) runs at torch's rate after t - 1
    scheduler steps = schedule(t - 1).  (torch's cosine is recursive: 1e-12 relative.)"""
    from srmi.optim import make_lr_schedule
    lr = 1e-3
    want = _torch_rates(make, 50, lr)
    f = make_lr_schedule(cfg, lr)
    for t0, w in enumerate(want):
        assert abs(oo.schedule(cfg, lr, t0) - w) <= 1e-12 * lr, (t0, w)
        assert f(t0) == oo.schedule(cfg, lr, t0)


@pytest.mark.parametrize("cfg", [dict(kind="step", step_size=3, gamma=0.1, warmup=5, warmup_start=0.25),
                                 dict(kind="cosine", t_max=10, eta_min=1e-6, warmup=4),
                                 dict(kind="constant")])
def test_warmup_then_main_is_the_closed_form(cfg):
    from srmi.optim import make_lr_schedule
    lr = 3e-4
    f = make_lr_schedule(cfg, lr)
    W, s = cfg.get("warmup", 0), cfg.get("warmup_start", 0.0)
    for t0 in range(40):
        want = oo.schedule(cfg, lr, t0)
        assert f(t0) == want
        if t0 < W:
            assert want == lr * (s + (1 - s) * t0 / W)
        elif cfg["kind"] == "step":
            assert want == lr * 0.1 ** ((t0 - W) // 3)
        elif cfg["kind"] == "cosine":
            assert want == (1e-6 if t0 - W >= 10 else 1e-6 + (lr - 1e-6) * (1 + math.cos(math.pi * (t0 - W) / 10)) / 2)
        else:
            assert want == lr
    assert make_lr_schedule(None, lr) is None
    g = lambda t0: 1.0 / (1 + t0)  # noqa: E731
    assert make_lr_schedule(g, lr) is g


# ----------------------------------------------------------------------------- arguments
def test_bad_arguments_raise_value_error_before_anything_is_allocated():
    from srmi.engine import NetSpec
    from srmi.trainer import FusedTrainer
    cpu = torch.device("cpu")
    bad = [dict(ema=dict(decay=1.0)), dict(ema=dict(decay=-0.1)), dict(ema=dict(decay=0.9, momentum=1)),
           dict(ema=0.999), dict(clip_norm=0.0), dict(clip_norm=-1.0), dict(clip_norm=math.inf),
           dict(clip_norm=math.nan), dict(clip_norm="1"), dict(guard=False, clip_norm=1.0),
           dict(guard=False, ema=dict()), dict(lr_schedule=dict(kind="exponential")),
           dict(lr_schedule=dict(step_size=2)), dict(lr_schedule=dict(kind="step", step_size=0, gamma=0.5)),
           dict(lr_schedule=dict(kind="step", step_size=2)), dict(lr_schedule=dict(kind="cosine", t_max=0)),
           dict(lr_schedule=dict(kind="cosine", t_max=5, gamma=0.1)),
           dict(lr_schedule=dict(kind="constant", warmup=-1)),
           dict(lr_schedule=dict(kind="constant", warmup=3, warmup_start=1.5)), dict(lr_schedule=3)]
    for kw in bad:
        with pytest.raises(ValueError):
            FusedTrainer(NetSpec(), 2, device=cpu, **kw)


def test_guard_defaults():
    from srmi.optim import check_guard
    assert check_guard(None, None, None) is False
    assert check_guard(None, 1.0, None) is True and check_guard(None, None, dict(decay=0.9, warmup=True)) is True
    assert check_guard(True, None, None) is True and check_guard(False, None, None) is False


# ----------------------------------------------------------------------------- checkpoints
def _ckpt_setup():
    from srmi import checkpoint as ck
    from srmi.engine import NetSpec
    from srmi.model.common import _python_table
    table = _python_table(NetSpec(arch="rcan", nchannels_in=2, nchannels_out=2, nlayers=1, nblocks=2))
    n = sum(t[2] for t in table)
    gen = torch.Generator().manual_seed(1)
    flat, ema = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    base = ck.checkpoint(3, 7, flat, table, torch.zeros(n), torch.zeros(n), 0, 1e-4, (0.9, 0.999), 1e-8, 0.0, 0.5)
    return ck, table, flat, ema, base


def _save_load(state):
    buf = io.BytesIO()
    torch.save(state, buf)
    buf.seek(0)
    return torch.load(buf, map_location="cpu", weights_only=True)  # CheckpointStore.load's call


def test_checkpoint_extra_keys_round_trip():
    ck, table, flat, ema, base = _ckpt_setup()
    state = ck.add_optimizer_extras(dict(base), table, 4, dict(decay=0.99, warmup=True), ema)
    assert set(state) == set(base) | {"srmi_optimizer", "ema_state_dict"}
    assert list(state["ema_state_dict"]) == list(state["model_state_dict"])
    back = _save_load(state)
    assert back["srmi_optimizer"] == dict(skipped=4, ema_decay=0.99, ema_warmup=True)
    skipped, host_e = ck.load_optimizer_extras(table, back, flat, torch.zeros_like(ema))
    assert skipped == 4 and torch.equal(host_e, ema)
    # a trainer without averaged weights ignores the key
    assert ck.load_optimizer_extras(table, back, flat, None) == (4, None)
    # without ema: the record alone
    state = ck.add_optimizer_extras(dict(base), table, 0)
    assert "ema_state_dict" not in state and state["srmi_optimizer"] == dict(skipped=0, ema_decay=None, ema_warmup=None)
    # what the reference's loader does with such a file: pops its two dicts, .get()s the rest
    back.pop("model_state_dict"), back.pop("optimizer_state_dict")
    assert back.get("epoch") == 3 and back.get("itime") == 7 and back.get("loss") == 0.5


def test_a_file_without_the_extra_keys_loads():
    ck, table, flat, ema, base = _ckpt_setup()
    back = _save_load(base)
    skipped, host_e = ck.load_optimizer_extras(table, back, flat, torch.zeros_like(ema))
    assert skipped == 0 and torch.equal(host_e, flat) and host_e is not flat  # the average starts at params
    assert ck.load_optimizer_extras(table, back, flat, None) == (0, None)


def test_bad_extra_keys_are_refused_on_the_host():
    ck, table, flat, ema, base = _ckpt_setup()
    good = ck.add_optimizer_extras(dict(base), table, 1, dict(decay=0.9, warmup=False), ema)
    dst = torch.zeros_like(ema)
    for rec in ([1], dict(skipped=-1), dict(skipped=1.5), dict(skipped=True)):
        with pytest.raises(ValueError):
            ck.load_optimizer_extras(table, dict(good, srmi_optimizer=rec), flat, dst)
    sd = dict(good["ema_state_dict"])
    name = next(iter(sd))
    with pytest.raises(KeyError):
        ck.load_optimizer_extras(table, dict(good, ema_state_dict={k: v for k, v in sd.items() if k != name}), flat, dst)
    with pytest.raises(RuntimeError):
        ck.load_optimizer_extras(table, dict(good, ema_state_dict=dict(sd, **{name: sd[name].reshape(-1)[:-1]})), flat, dst)
    assert not dst.any()  # nothing was applied


def test_loss_record_line_carries_the_skipped_count(tmp_path):
    from srmi.harness import LossRecords
    assert LossRecords.serialize("train", 0.5, 1.0, 2.0) == ["train", "0.500", "1.000000", "2.000000"]
    assert LossRecords.serialize("train", 0.5, 1.0, 2.0, skipped=0) == ["train", "0.500", "1.000000", "2.000000"]
    rec = LossRecords(str(tmp_path), "ds", "t", "m")
    rec.record_losses("train", 0.0, 1.0, 2.0)
    rec.record_losses("train", 0.5, 1.0, 2.0, skipped=3, flush=True)
    assert rec.load_results() == [["train", "0.000", "1.000000", "2.000000"],
                                  ["train", "0.500", "1.000000", "2.000000", "skipped=3"]]


# ----------------------------------------------------------------------------- binding
def test_new_symbols_are_declared_exported_and_bound():
    from srmi import _lib, engine
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "srmi.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED and hasattr(lib, name) and f"int {name}(" in header
    assert callable(engine.grad_norm) and callable(engine.adam_step_guarded)
    import ctypes as C
    nbytes = C.c_size_t()
    for n, blocks in ((1, 1), (256, 1), (257, 2), (8192 * 256, 8192), (8192 * 256 * 4 + 3, 8192)):
        assert lib.srmi_grad_norm_workspace(n, C.byref(nbytes)) == 0 and nbytes.value == 8 * blocks
    assert lib.srmi_grad_norm_workspace(0, C.byref(nbytes)) == _lib.SRMI_ERR_ARG
