"""Host side of the optimizer guards (DESIGN.md §1 "Optimizer guards"): the checks of
FusedTrainer's clip_norm / guard / ema / lr_schedule arguments, the EMA decay of a step and
the learning-rate schedules.  Pure Python: nothing here touches a device.

The reference trains at a constant task.lr (dual_trainer.py:126) and keeps no averaged
weights; the schedules restate torch.optim.lr_scheduler's closed forms (StepLR,
CosineAnnealingLR, LinearLR as the warm-up), the average torch.optim.swa_utils'
get_ema_multi_avg_fn.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, Mapping, Optional

EMA_KEYS = {"decay", "warmup"}
SCHEDULE_KEYS = {"constant": set(), "step": {"step_size", "gamma"}, "cosine": {"t_max", "eta_min"}}
WARMUP_KEYS = {"warmup", "warmup_start"}


def _number(x) -> bool:
    return isinstance(x, (int, float)) and not isinstance(x, bool)


def check_clip_norm(clip_norm) -> Optional[float]:
    """None, or a finite float > 0 (ValueError otherwise)."""
    if clip_norm is None:
        return None
    if not _number(clip_norm) or not math.isfinite(clip_norm) or not clip_norm > 0:
        raise ValueError(f"clip_norm: None or a finite number > 0, got {clip_norm!r}")
    return float(clip_norm)


def check_ema(ema) -> Optional[Dict]:
    """None, or dict(decay=0.999, warmup=True) with a missing key at that default ->
    dict(decay=float, warmup=bool).  Unknown keys, a decay outside [0, 1): ValueError."""
    if ema is None:
        return None
    if not isinstance(ema, Mapping):
        raise ValueError(f"ema: a dict(decay=, warmup=) or None, got {ema!r}")
    extra = set(ema) - EMA_KEYS
    if extra:
        raise ValueError(f"ema: unknown keys {sorted(extra)}")
    decay = ema.get("decay", 0.999)
    if not _number(decay) or not (0.0 <= decay < 1.0):
        raise ValueError(f"ema: decay in [0, 1), got {decay!r}")
    return dict(decay=float(decay), warmup=bool(ema.get("warmup", True)))


def check_guard(guard, clip_norm, ema) -> bool:
    """guard=None: on iff clip_norm or ema is set (both need the control record)."""
    need = clip_norm is not None or ema is not None
    if guard is None:
        return need
    if not isinstance(guard, bool):
        raise ValueError(f"guard: None, True or False, got {guard!r}")
    if need and not guard:
        raise ValueError("guard=False with clip_norm or ema: both run through the guarded step")
    return guard


def ema_decay_at(cfg: Mapping, t: int) -> float:
    """The decay used by Adam step t (1-based): min(decay, (1 + t) / (10 + t)) under warm-up."""
    return min(cfg["decay"], (1.0 + t) / (10.0 + t)) if cfg["warmup"] else cfg["decay"]


def make_lr_schedule(schedule, lr: float) -> Optional[Callable[[int], float]]:
    """None, a dict(kind=...), or a callable t0 -> lr  ->  None or a callable t0 -> lr.

    Adam step t (1-based) uses schedule(t - 1): torch's convention of stepping the scheduler
    after the optimizer.  With `lr` the base rate:
      constant                      lr
      step(step_size, gamma)        lr * gamma ** (t0 // step_size)                     (StepLR)
      cosine(t_max, eta_min=0)      eta_min + (lr - eta_min) (1 + cos(pi t0 / t_max)) / 2,
                                    eta_min from t_max on                    (CosineAnnealingLR)
    each with an optional warmup=W, warmup_start=s (LinearLR): lr * (s + (1 - s) t0 / W) for
    t0 < W, and the main schedule at t0 - W from W on.  A pure function of t0: nothing of it is
    stored in a checkpoint.  A bad kind, key or value: ValueError."""
    if schedule is None:
        return None
    if callable(schedule):
        return schedule
    if not isinstance(schedule, Mapping) or "kind" not in schedule:
        raise ValueError(f"lr_schedule: None, a callable or a dict(kind=...), got {schedule!r}")
    kind = schedule["kind"]
    if kind not in SCHEDULE_KEYS:
        raise ValueError(f"lr_schedule: kind one of {sorted(SCHEDULE_KEYS)}, got {kind!r}")
    extra = set(schedule) - SCHEDULE_KEYS[kind] - WARMUP_KEYS - {"kind"}
    if extra:
        raise ValueError(f"lr_schedule {kind}: unknown keys {sorted(extra)}")
    W = schedule.get("warmup", 0)
    s = schedule.get("warmup_start", 0.0)
    if not isinstance(W, int) or isinstance(W, bool) or W < 0:
        raise ValueError(f"lr_schedule: warmup a whole number of steps >= 0, got {W!r}")
    if not _number(s) or not (0.0 <= s <= 1.0):
        raise ValueError(f"lr_schedule: warmup_start in [0, 1], got {s!r}")
    if kind == "constant":
        def main(t0: int) -> float:
            return lr
    elif kind == "step":
        size, gamma = schedule.get("step_size"), schedule.get("gamma")
        if not isinstance(size, int) or isinstance(size, bool) or size < 1:
            raise ValueError(f"lr_schedule step: step_size a whole number >= 1, got {size!r}")
        if not _number(gamma) or not math.isfinite(gamma) or not gamma > 0:
            raise ValueError(f"lr_schedule step: gamma a finite number > 0, got {gamma!r}")

        def main(t0: int) -> float:
            return lr * gamma ** (t0 // size)
    else:
        t_max, eta_min = schedule.get("t_max"), schedule.get("eta_min", 0.0)
        if not isinstance(t_max, int) or isinstance(t_max, bool) or t_max < 1:
            raise ValueError(f"lr_schedule cosine: t_max a whole number >= 1, got {t_max!r}")
        if not _number(eta_min) or not math.isfinite(eta_min) or eta_min < 0:
            raise ValueError(f"lr_schedule cosine: eta_min a finite number >= 0, got {eta_min!r}")

        def main(t0: int) -> float:
            if t0 >= t_max:
                return eta_min
            return eta_min + (lr - eta_min) * (1.0 + math.cos(math.pi * t0 / t_max)) / 2.0

    def at(t0: int) -> float:
        if t0 < W:
            return lr * (s + (1.0 - s) * t0 / W)
        return main(t0 - W)
    return at
