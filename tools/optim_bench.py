#!/usr/bin/env python3
"""What do the optimizer guards cost per train step?  (DESIGN.md §1 "Optimizer guards".)

The C2 shape of bench.py: rcan-10-20-64, two variables, 64 tiles of 48 -> 192 per step, the
trainer's own micro-batch split, bf16.  Two arms are timed, window by window in turn on one
device (device events around --steps steps each, after --warmup steps each):

  off   FusedTrainer(): bench.py's training leg, the step as it was (srmi_adam_step);
  on    FusedTrainer(clip_norm=, ema=dict()): srmi_grad_norm's two launches before Adam, and
        srmi_adam_step_guarded with the averaged weights in place of srmi_adam_step.

The launches are timed too, alone on an idle device on the `on` trainer's own buffers (device
events around --stage-reps calls each, the median of --repeats windows): srmi_grad_norm (both
of its launches), srmi_adam_step, srmi_adam_step_guarded without and with the average.

Expected from bytes alone: the norm reads the 4 n-byte gradient once, the average adds a read and
a write of 4 n bytes to Adam's 28 n (4 reads, 3 writes); the step as a whole moves 78.8 GB.

Prints ONE JSON line and writes it to --out: the median ms per step of each arm with the raw
per-window values, the per-window ratio on / off next to the spread of the `off` windows
themselves (max / min) -- a ratio inside that spread is not a measured difference -- and the
launch times with the bandwidth they imply.  No pass / fail bar.
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "super-resolution-climate_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

STEP_GB = 78.8  # the C2 step's traffic


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7, help="timed windows of each kind")
    ap.add_argument("--stage-reps", type=int, default=20, help="calls per timed window of a launch")
    ap.add_argument("--clip-norm", type=float, default=1.0)
    ap.add_argument("--ema-decay", type=float, default=0.999)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench: no GPU (there is no CPU path to time)")
    from oracle.rcan_oracle import synthetic_hr
    from srmi.engine import NetSpec, adam_step, adam_step_guarded, grad_norm
    from srmi.trainer import FusedTrainer

    dev = torch.device("cuda", 0)
    C, B = a.channels, a.batch
    spec = NetSpec(arch="rcan", nchannels_in=C, nchannels_out=C, nfeatures=64, nlayers=10, nblocks=20, cbottleneck=2,
                   scale=4)
    hr = torch.tensor(synthetic_hr(B, C, 192, 1234)).to(dev)
    arms = {"off": FusedTrainer(spec, B, (48, 48), lr=1e-4, device=dev, seed=0),
            "on": FusedTrainer(spec, B, (48, 48), lr=1e-4, device=dev, seed=0, clip_norm=a.clip_norm,
                               ema=dict(decay=a.ema_decay))}
    last = {}
    for name, tr in arms.items():
        for _ in range(a.warmup):
            last[name] = {k: v.clone() for k, v in tr.step(hr).items()}
    torch.cuda.synchronize()
    st = torch.cuda.current_stream()
    ms = {k: [] for k in arms}
    for _ in range(a.repeats):
        for name, tr in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(a.steps):
                out = tr.step(hr)
            e1.record(st)
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.steps)
            last[name] = {k: v.clone() for k, v in out.items()}
    torch.cuda.synchronize()
    losses = {f"{n}.{k}": float(v) for n, d in last.items() for k, v in d.items()}
    if not all(math.isfinite(v) for v in losses.values()):
        raise SystemExit(f"optim_bench: non-finite result {losses}")
    skipped = arms["on"].skipped_steps()

    # the launches alone, on copies of the `on` trainer's buffers (its state is not advanced)
    tr = arms["on"]
    n = tr.params.numel()
    p, m, v, e = tr.params.clone(), tr.m.clone(), tr.v.clone(), tr.ema.clone()
    ctl = tr.ctl.clone()
    hp = (tr.t, tr.lr, tr.betas, tr.eps, tr.wd)
    stages = {
        "grad_norm": (lambda: grad_norm(tr.grads, ctl, a.clip_norm, tr.norm_ws), 4 * n),
        "adam_step": (lambda: adam_step(p, tr.grads, m, v, *hp), 28 * n),
        "adam_step_guarded": (lambda: adam_step_guarded(p, tr.grads, m, v, ctl, *hp), 28 * n),
        "adam_step_guarded_ema": (lambda: adam_step_guarded(p, tr.grads, m, v, ctl, *hp, ema=e,
                                                            ema_decay=a.ema_decay), 36 * n),
    }
    stage_ms = {k: [] for k in stages}
    for name, (fn, _) in stages.items():
        fn()
        torch.cuda.synchronize()
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(a.stage_reps):
                fn()
            e1.record(st)
            e1.synchronize()
            stage_ms[name].append(e0.elapsed_time(e1) / a.stage_reps)
    torch.cuda.synchronize()

    added_bytes = 4 * n + 8 * n
    res = {"tool": "optim_bench", "device": torch.cuda.get_device_name(0),
           "config": {"workload": f"rcan-10-20-64 train step, {C} vars, {B} tiles 48->192, loss l2",
                      "clip_norm": a.clip_norm, "ema_decay": a.ema_decay, "params": n, "micro": arms["off"].micro,
                      "steps_per_window": a.steps, "warmup": a.warmup, "repeats": a.repeats,
                      "stage_reps": a.stage_reps},
           "ms_per_step": {}, "last": {k: float(f"{x:.6e}") for k, x in losses.items()},
           "skipped_steps_on": skipped}
    for k in arms:
        res["ms_per_step"][k] = {"median": round(statistics.median(ms[k]), 3), "windows": [round(x, 3) for x in ms[k]]}
    res["off_spread_max_over_min"] = round(max(ms["off"]) / min(ms["off"]), 4)
    r = [x / y for x, y in zip(ms["on"], ms["off"])]
    res["ratio_on_over_off"] = {"median": round(statistics.median(r), 4), "min_max": [round(min(r), 4), round(max(r), 4)]}
    res["added_ms_per_step"] = round(statistics.median([x - y for x, y in zip(ms["on"], ms["off"])]), 3)
    res["expected_from_bytes"] = {"added_mb": round(added_bytes / 1e6, 1), "step_gb": STEP_GB,
                                  "share_of_step_bytes": round(added_bytes / (STEP_GB * 1e9), 5)}
    res["launch_ms"] = {}
    for k, x in stage_ms.items():
        med = statistics.median(x)
        res["launch_ms"][k] = {"median": round(med, 4), "windows": [round(q, 4) for q in x],
                               "mb": round(stages[k][1] / 1e6, 1), "gb_per_s": round(stages[k][1] / med / 1e6, 1)}
    res["launch_ms"]["added_by_the_guards"] = round(
        statistics.median(stage_ms["grad_norm"]) + statistics.median(stage_ms["adam_step_guarded_ema"])
        - statistics.median(stage_ms["adam_step"]), 4)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
