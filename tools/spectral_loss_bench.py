#!/usr/bin/env python3
"""What does FusedTrainer(spectral=...) cost per train step?  (DESIGN.md §1 "Spectral loss".)

The C2 shape of bench.py: rcan-10-20-64, two variables, 64 tiles of 48 -> 192 per step, the
trainer's own micro-batch split, bf16.  Two arms are timed, window by window in turn on one
device (device events around --steps steps each, after --warmup steps each):

  off   FusedTrainer(spectral=None): bench.py's training leg, the step as it was;
  on    FusedTrainer(spectral=dict(weight=1.0, window=64, stride=32)): the parts after the
        forward, the finalise, the RMSE's dy as a map instead of formed in the tail kernels,
        the gather into dy.

The spectral stage's own launches are timed too, alone on an idle device over the whole
batch (device events around --stage-reps calls each, the median of --repeats windows):
srmi_spectral_loss_parts (the window kernel and the per-plane sums), the finalise and the
gather into dy.

Prints ONE JSON line and writes it to --out: the median ms per step of each arm with the raw
per-window values, the per-window ratio on / off next to the spread of the `off` windows
themselves (max / min) -- a ratio inside that spread is not a measured difference -- and
the stage times.  No pass / fail bar.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7, help="timed windows of each kind")
    ap.add_argument("--stage-reps", type=int, default=20, help="calls per timed window of a spectral launch")
    ap.add_argument("--loss-fn", default="l2", choices=["l2", "charbonnier"])
    ap.add_argument("--window", type=int, default=64)
    ap.add_argument("--stride", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectral_loss_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spectral_loss_bench: no GPU (there is no CPU path to time)")
    from oracle.rcan_oracle import synthetic_hr
    from srmi.engine import NetSpec
    from srmi.trainer import FusedTrainer

    dev = torch.device("cuda", 0)
    C, B = a.channels, a.batch
    spec = NetSpec(arch="rcan", nchannels_in=C, nchannels_out=C, nfeatures=64, nlayers=10, nblocks=20, cbottleneck=2,
                   scale=4)
    hr = torch.tensor(synthetic_hr(B, C, 192, 1234)).to(dev)
    spectral = dict(weight=1.0, window=a.window, stride=a.stride)
    arms = {"off": FusedTrainer(spec, B, (48, 48), lr=1e-4, device=dev, seed=0, loss_fn=a.loss_fn),
            "on": FusedTrainer(spec, B, (48, 48), lr=1e-4, device=dev, seed=0, loss_fn=a.loss_fn, spectral=spectral)}
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
        raise SystemExit(f"spectral_loss_bench: non-finite loss {losses}")

    # the spectral launches alone, on the `on` trainer's own buffers
    tr = arms["on"]
    sl, dy = tr.spectral, torch.zeros_like(tr.sr)
    stages = {"parts": lambda: sl.parts(tr.sr, hr), "finalize": lambda: sl.finalize(tr.loss4[3:4]),
              "add_dy": lambda: sl.add_dy(dy)}
    stage_ms = {k: [] for k in stages}
    for name, fn in stages.items():
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

    nwin = (sl.workspace.numel() // (B * C)) // (a.window * a.window * 4)
    res = {"tool": "spectral_loss_bench", "device": torch.cuda.get_device_name(0),
           "config": {"workload": f"rcan-10-20-64 train step, {C} vars, {B} tiles 48->192, loss {a.loss_fn}",
                      "spectral": spectral, "jobs": B * C * nwin, "workspace_mb": round(sl.workspace.numel() / 1e6, 1),
                      "micro": arms["off"].micro, "steps_per_window": a.steps, "warmup": a.warmup,
                      "repeats": a.repeats, "stage_reps": a.stage_reps},
           "ms_per_step": {}, "last_loss": {k: round(v, 6) for k, v in losses.items()}}
    for k in arms:
        res["ms_per_step"][k] = {"median": round(statistics.median(ms[k]), 3), "windows": [round(v, 3) for v in ms[k]]}
    res["off_spread_max_over_min"] = round(max(ms["off"]) / min(ms["off"]), 4)
    r = [x / y for x, y in zip(ms["on"], ms["off"])]
    res["ratio_on_over_off"] = {"median": round(statistics.median(r), 4),
                                "min_max": [round(min(r), 4), round(max(r), 4)]}
    res["added_ms_per_step"] = round(statistics.median([x - y for x, y in zip(ms["on"], ms["off"])]), 3)
    res["spectral_launch_ms"] = {k: {"median": round(statistics.median(v), 4), "windows": [round(x, 4) for x in v]}
                                 for k, v in stage_ms.items()}
    res["spectral_launch_ms"]["sum_of_medians"] = round(sum(statistics.median(v) for v in stage_ms.values()), 4)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
