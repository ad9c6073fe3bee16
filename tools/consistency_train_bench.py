#!/usr/bin/env python3
"""What does FusedTrainer(consistent=K) cost per train step?  (DESIGN.md §1 "Consistency in
training".)

The C2 shape of bench.py: rcan-10-20-64, two variables, 64 tiles of 48 -> 192 per step, the
trainer's own micro-batch split, bf16.  Two arms are timed, window by window in turn on one
device (device events around --steps steps each, after --warmup steps each):

  off   FusedTrainer(consistent=0): bench.py's training leg, the step as it was;
  on    FusedTrainer(consistent=K) (default 2): the layer's three launches after the forward,
        the RMSE's dy as a map instead of formed in the tail kernels, the adjoint's three
        launches before the backward.

The layer's six launches are timed too, alone on an idle device over the whole batch (device
events around --stage-reps calls each, the median of --repeats windows): residual, the K
iterations, apply, and the adjoint's gather, K iterations and apply.

rms(D(sr) - lr) of both arms' last step says what the layer is for: the `on` arm's output
coarse-grains back to the network's input.

Prints ONE JSON line and writes it to --out: the median ms per step of each arm with the raw
per-window values, the per-window ratio on / off next to the spread of the `off` windows
themselves (max / min) -- a ratio inside that spread is not a measured difference -- the
launch times and the two rms values.  No pass / fail bar.

--train-steps N > 0 also trains both arms for N more steps on the same synthetic tiles and
prints both losses: synthetic fields, no evidence about real data.
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
    ap.add_argument("--stage-reps", type=int, default=20, help="calls per timed window of a layer launch")
    ap.add_argument("--loss-fn", default="l2", choices=["l2", "charbonnier"])
    ap.add_argument("--consistent", type=int, default=2)
    ap.add_argument("--train-steps", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consistency_train_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("consistency_train_bench: no GPU (there is no CPU path to time)")
    from oracle.rcan_oracle import synthetic_hr
    from srmi._lib import call, ptr
    from srmi.engine import NetSpec, downsample
    from srmi.trainer import FusedTrainer

    dev = torch.device("cuda", 0)
    C, B, K = a.channels, a.batch, a.consistent
    spec = NetSpec(arch="rcan", nchannels_in=C, nchannels_out=C, nfeatures=64, nlayers=10, nblocks=20, cbottleneck=2,
                   scale=4)
    hr = torch.tensor(synthetic_hr(B, C, 192, 1234)).to(dev)
    arms = {"off": FusedTrainer(spec, B, (48, 48), lr=1e-4, device=dev, seed=0, loss_fn=a.loss_fn),
            "on": FusedTrainer(spec, B, (48, 48), lr=1e-4, device=dev, seed=0, loss_fn=a.loss_fn, consistent=K)}
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
        raise SystemExit(f"consistency_train_bench: non-finite loss {losses}")
    rms = {}
    for name, tr in arms.items():  # D(sr) against the LR batch the network was fed
        d = downsample(tr.sr, 4, mode=tr.dmode) - tr.lrbuf
        rms[name] = float(d.double().pow(2).mean().sqrt())

    # the six launches alone, on the `on` trainer's own buffers
    tr = arms["on"]
    L = tr.layer
    n, h, w, s = B * C, 48, 48, 4
    x, dy = tr.sr.clone(), torch.zeros_like(tr.sr)
    S = st.cuda_stream
    act, R = ptr(L.active), ptr(L.R)

    def iterate(name, a0, a1):
        src, dst = a0, a1
        for k in range(K):
            call(name, ptr(src), act, n, h, w, s, L.um, L.dm, int(k == 0), R, ptr(dst), S)
            src, dst = dst, (a0 if dst is a1 else a1)
    stages = {
        "residual": lambda: call("srmi_consistency_residual", ptr(x), ptr(tr.lrbuf), n, h, w, s, L.dm, ptr(L.r0), act,
                                 S),
        f"iterate_x{K}": lambda: iterate("srmi_consistency_iterate", L.pp[0], L.pp[1]),
        "apply": lambda: call("srmi_consistency_apply", R, n, h, w, s, L.um, ptr(x), S),
        "adjoint_gather": lambda: call("srmi_consistency_adjoint_gather", ptr(dy), n, h, w, s, L.um, ptr(L.pp[0]), S),
        f"adjoint_iterate_x{K}": lambda: iterate("srmi_consistency_adjoint_iterate", L.pp[0], L.pp[1]),
        "adjoint_apply": lambda: call("srmi_consistency_adjoint_apply", R, act, n, h, w, s, L.dm, ptr(dy), S),
    }
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

    res = {"tool": "consistency_train_bench", "device": torch.cuda.get_device_name(0),
           "config": {"workload": f"rcan-10-20-64 train step, {C} vars, {B} tiles 48->192, loss {a.loss_fn}",
                      "consistent": K, "sr_mb": round(tr.sr.numel() * 4 / 1e6, 1), "micro": arms["off"].micro,
                      "steps_per_window": a.steps, "warmup": a.warmup, "repeats": a.repeats,
                      "stage_reps": a.stage_reps},
           "ms_per_step": {}, "last_loss": {k: round(v, 6) for k, v in losses.items()},
           "rms_D_sr_minus_lr": {k: float(f"{v:.4e}") for k, v in rms.items()}}
    for k in arms:
        res["ms_per_step"][k] = {"median": round(statistics.median(ms[k]), 3), "windows": [round(v, 3) for v in ms[k]]}
    res["off_spread_max_over_min"] = round(max(ms["off"]) / min(ms["off"]), 4)
    r = [p / q for p, q in zip(ms["on"], ms["off"])]
    res["ratio_on_over_off"] = {"median": round(statistics.median(r), 4), "min_max": [round(min(r), 4), round(max(r), 4)]}
    res["added_ms_per_step"] = round(statistics.median([p - q for p, q in zip(ms["on"], ms["off"])]), 3)
    res["layer_launch_ms"] = {k: {"median": round(statistics.median(v), 4), "windows": [round(q, 4) for q in v]}
                              for k, v in stage_ms.items()}
    res["layer_launch_ms"]["sum_of_medians"] = round(sum(statistics.median(v) for v in stage_ms.values()), 4)
    if a.train_steps > 0:
        for name, t in arms.items():
            for _ in range(a.train_steps):
                out = t.step(hr)
            torch.cuda.synchronize()
            res.setdefault("loss_after_training_on_synthetic_tiles_no_evidence_about_real_data", {})[name] = round(
                float(out["loss"]), 6)
        res["train_steps"] = a.train_steps
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
