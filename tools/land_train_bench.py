#!/usr/bin/env python3
"""What does FusedTrainer(land=True) cost per train step?  (DESIGN.md §1 "Land in
training", §6.)

The C2 shape of bench.py: rcan-10-20-64, two variables, 64 tiles of 48 -> 192 per step,
the trainer's own micro-batch split.  Three things are timed, window by window in turn on
one device (device events around --steps steps each, after --warmup steps each):

  off       FusedTrainer(land=False) on an all-wet batch (bench.py's training leg);
  on_wet    FusedTrainer(land=True) on the same all-wet batch: the fill finds nothing, the
            masked loss kernels count every element, and the backward reads a dy map instead
            of forming (sr - hr) * scale in the tail kernels;
  on_coast  FusedTrainer(land=True) on that batch with a coast painted into every tile but
            the first (NaN: a smooth coastline, a lake, an island).

One land=True trainer serves both of its windows, so the two differ in the batch only.
Prints ONE JSON line and writes it to --out: the median ms per step of each with the raw
per-window values, and the per-window ratios on_wet / off and on_coast / off next to the
spread of the `off` windows themselves (max / min) -- a ratio inside that spread is not a
measured difference.  No pass / fail bar.
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


def paint_coast(hr):
    """NaN (the same mask in every channel) in every tile of hr [B, C, T, T] but tile 0:
    the land right of a sinusoidal coastline whose phase moves with the tile, a lake in
    the land, an island in the sea."""
    B, _, T, _ = hr.shape
    yy, xx = torch.meshgrid(torch.arange(T, device=hr.device), torch.arange(T, device=hr.device), indexing="ij")
    yy, xx = yy.float(), xx.float()
    out = hr.clone()
    for k in range(1, B):
        dry = xx > 0.55 * T + 0.2 * T * torch.sin(7.0 * yy / T + 0.37 * k)
        dry[T // 8:T // 8 + 5, T - 6:T - 1] = False
        dry[(3 * T) // 4 - 4:(3 * T) // 4 + 5, T // 4 - 8:T // 4 + 9] = True
        if k % 2 == 0:
            dry = dry.T.flip(0, 1)
        out[k][:, dry] = float("nan")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7, help="timed windows of each kind")
    ap.add_argument("--loss-fn", default="l2", choices=["l2", "charbonnier"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "land_train_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("land_train_bench: no GPU (there is no CPU path to time)")
    from oracle.rcan_oracle import synthetic_hr
    from srmi.engine import NetSpec
    from srmi.trainer import FusedTrainer

    dev = torch.device("cuda", 0)
    C, B = a.channels, a.batch
    spec = NetSpec(arch="rcan", nchannels_in=C, nchannels_out=C, nfeatures=64, nlayers=10, nblocks=20, cbottleneck=2,
                   scale=4)
    wet = torch.tensor(synthetic_hr(B, C, 192, 1234)).to(dev)
    coast = paint_coast(wet)
    trs = {land: FusedTrainer(spec, B, (48, 48), lr=1e-4, device=dev, seed=0, loss_fn=a.loss_fn, land=land)
           for land in (False, True)}
    kinds = {"off": (trs[False], wet), "on_wet": (trs[True], wet), "on_coast": (trs[True], coast)}
    last = {}
    for name, (tr, hr) in kinds.items():
        for _ in range(a.warmup):
            last[name] = tr.step(hr)["loss"].clone()
    torch.cuda.synchronize()
    st = torch.cuda.current_stream()
    ms = {k: [] for k in kinds}
    for _ in range(a.repeats):
        for name, (tr, hr) in kinds.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(a.steps):
                out = tr.step(hr)
            e1.record(st)
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.steps)
            last[name] = out["loss"].clone()
    torch.cuda.synchronize()
    losses = {k: float(v) for k, v in last.items()}
    if not all(math.isfinite(v) for v in losses.values()):
        raise SystemExit(f"land_train_bench: non-finite loss {losses}")
    res = {"tool": "land_train_bench", "device": torch.cuda.get_device_name(0),
           "config": {"workload": f"rcan-10-20-64 train step, {C} vars, {B} tiles 48->192, loss {a.loss_fn}",
                      "micro": trs[False].micro, "steps_per_window": a.steps, "warmup": a.warmup, "repeats": a.repeats,
                      "dry_share_coast": round(1.0 - float(torch.isfinite(coast).float().mean()), 4)},
           "ms_per_step": {}, "last_loss": {k: round(v, 6) for k, v in losses.items()}}
    for k in kinds:
        res["ms_per_step"][k] = {"median": round(statistics.median(ms[k]), 3), "windows": [round(v, 3) for v in ms[k]]}
    res["off_spread_max_over_min"] = round(max(ms["off"]) / min(ms["off"]), 4)
    for k in ("on_wet", "on_coast"):
        r = [x / y for x, y in zip(ms[k], ms["off"])]
        res[f"ratio_{k}_over_off"] = {"median": round(statistics.median(r), 4),
                                      "min_max": [round(min(r), 4), round(max(r), 4)]}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
