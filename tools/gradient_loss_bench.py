#!/usr/bin/env python3
"""What does FusedTrainer(gradient=...) cost per train step?  (DESIGN.md §1 "Gradient loss".)

The C2 shape of bench.py: rcan-10-20-64, two variables, 64 tiles of 48 -> 192 per step, the
trainer's own micro-batch split, bf16.  Two arms are timed, window by window in turn on one
device (device events around --steps steps each, after --warmup steps each):

  off   FusedTrainer(gradient=None): bench.py's training leg, the step as it was;
  on    FusedTrainer(gradient=dict(weight=1.0)): the parts after the forward, the finalise, the
        RMSE's dy as a map instead of formed in the tail kernels, the term's gradient into dy.

The term's own launches are timed too, alone on an idle device over the whole batch (device
events around --stage-reps calls each, the median of --repeats windows):
srmi_gradient_loss_parts (tile pass, per-plane sums), the finalise and srmi_gradient_loss_dy.
Beside each time stand the bytes the launch has to move, computed from the shapes
(launch_bytes) -- parts: prediction and target read once; dy: prediction and target read once,
dy read and written (U and V are recomputed, not stored) -- and the time those bytes take at
--hbm-tbs (the achievable HBM rate): the memory floor, a figure computed from shapes and not
measured.  The batch's working set is smaller than the 256 MiB Infinity Cache, so a launch may
run below that floor; it is a yardstick, not a bound.

The network is UNTRAINED (seeded initial weights, synthetic fields): the figures are costs of
the step, and no claim is made that the term improves skill on real data.

Prints ONE JSON line and writes it to --out: the median ms per step of each arm with the raw
per-window values, the per-window ratio on / off next to the spread of the `off` windows
themselves (max / min) -- a ratio inside that spread is not a measured difference -- and
the launch times.  No pass / fail bar.
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


def launch_bytes(nplanes: int, H: int, W: int) -> dict:
    """The bytes each launch has to move, from the shapes (fp32 everywhere): 2 and 4 plane-sized
    transfers per plane, 6 over the two launches."""
    hw = H * W
    return {"parts": nplanes * 4 * 2 * hw, "add_dy": nplanes * 4 * (2 * hw + 2 * hw)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7, help="timed windows of each kind")
    ap.add_argument("--stage-reps", type=int, default=20, help="calls per timed window of one of the term's launches")
    ap.add_argument("--loss-fn", default="l2", choices=["l2", "charbonnier"])
    ap.add_argument("--hbm-tbs", type=float, default=6.3, help="achievable HBM rate the memory floor is taken at")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gradient_loss_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gradient_loss_bench: no GPU (there is no CPU path to time)")
    from oracle.rcan_oracle import synthetic_hr
    from srmi.engine import NetSpec
    from srmi.trainer import FusedTrainer

    dev = torch.device("cuda", 0)
    C, B = a.channels, a.batch
    spec = NetSpec(arch="rcan", nchannels_in=C, nchannels_out=C, nfeatures=64, nlayers=10, nblocks=20, cbottleneck=2,
                   scale=4)
    hr = torch.tensor(synthetic_hr(B, C, 192, 1234)).to(dev)
    gradient = dict(weight=1.0)
    arms = {"off": FusedTrainer(spec, B, (48, 48), lr=1e-4, device=dev, seed=0, loss_fn=a.loss_fn),
            "on": FusedTrainer(spec, B, (48, 48), lr=1e-4, device=dev, seed=0, loss_fn=a.loss_fn, gradient=gradient)}
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
        raise SystemExit(f"gradient_loss_bench: non-finite loss {losses}")

    # the term's launches alone, on the `on` trainer's own buffers
    tr = arms["on"]
    gl, dy = tr.gradient, torch.zeros_like(tr.sr)
    stages = {"parts": lambda: gl.parts(tr.sr, hr), "finalize": lambda: gl.finalize(tr.loss4[3:4]),
              "add_dy": lambda: gl.add_dy(dy, tr.sr, hr)}
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

    nbytes = launch_bytes(B * C, 192, 192)
    res = {"tool": "gradient_loss_bench", "device": torch.cuda.get_device_name(0),
           "config": {"workload": f"rcan-10-20-64 train step, {C} vars, {B} tiles 48->192, loss {a.loss_fn}",
                      "network": "untrained (seeded initial weights, synthetic fields)", "gradient": gradient,
                      "positions": B * C * 190 * 190, "workspace_kb": round(gl.workspace.numel() / 1e3, 1),
                      "micro": arms["off"].micro, "steps_per_window": a.steps, "warmup": a.warmup,
                      "repeats": a.repeats, "stage_reps": a.stage_reps, "hbm_tbs": a.hbm_tbs},
           "ms_per_step": {}, "last_loss": {k: round(v, 6) for k, v in losses.items()}}
    for k in arms:
        res["ms_per_step"][k] = {"median": round(statistics.median(ms[k]), 3), "windows": [round(v, 3) for v in ms[k]]}
    res["off_spread_max_over_min"] = round(max(ms["off"]) / min(ms["off"]), 4)
    r = [x / y for x, y in zip(ms["on"], ms["off"])]
    res["ratio_on_over_off"] = {"median": round(statistics.median(r), 4),
                                "min_max": [round(min(r), 4), round(max(r), 4)]}
    res["added_ms_per_step"] = round(statistics.median([x - y for x, y in zip(ms["on"], ms["off"])]), 3)
    res["gradient_launch_ms"] = {}
    for k, v in stage_ms.items():
        med = statistics.median(v)
        res["gradient_launch_ms"][k] = {"median": round(med, 4), "windows": [round(x, 4) for x in v]}
        if k in nbytes:  # the finalise is one workgroup over 2 * planes floats: a launch, not a stream
            floor = nbytes[k] / (a.hbm_tbs * 1e12) * 1e3
            res["gradient_launch_ms"][k].update(bytes=nbytes[k], memory_floor_ms=round(floor, 5),
                                                time_over_floor=round(med / floor, 2),
                                                tb_per_s=round(nbytes[k] / (med * 1e-3) / 1e12, 2))
    res["gradient_launch_ms"]["sum_of_medians"] = round(sum(statistics.median(v) for v in stage_ms.values()), 4)
    res["memory_floor_ms_both_launches"] = round(sum(nbytes.values()) / (a.hbm_tbs * 1e12) * 1e3, 5)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
