#!/usr/bin/env python3
"""Mean kernel duration per kind of step of a traced tools/land_train_bench.py run
(tools/land_train_trace.sh): kernel_trace.csv of rocprofv3 -> the table of
profiles/land_train_trace.txt.

The bench runs, with --repeats 1, --warmup W steps of off, on_wet and on_coast in turn and
then --steps S timed steps of each in turn.  A kernel's dispatches, sorted by start time,
therefore fall into those six blocks in order; only the timed blocks are averaged.  Which
kinds launch a kernel follows from its name: the masked loss kernels, the fill and the dy
kernel run in the two land kinds only, the unmasked loss kernels in `off` only, every other
kernel in all three.  A kernel whose call count does not divide into such blocks is listed
unsplit."""
import argparse
import csv
from collections import defaultdict

KEYS = ["tail_dgrad", "tail_wgrad_lds", "tail_fwd", "tiles_fill", "loss_dy_masked", "tile_loss_parts", "loss_from_parts",
        "downsample_kernel", "upsample_kernel"]
LAND_ONLY = ("masked", "tiles_fill")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace", help="rocprofv3's *_kernel_trace.csv")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    rows = defaultdict(list)
    with open(a.trace) as f:
        for r in csv.DictReader(f):
            rows[r["Kernel_Name"]].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    for name, ds in sorted(rows.items()):
        if not any(k in name for k in KEYS):
            continue
        short = name.split("(")[0].replace("void ", "")
        if any(k in name for k in LAND_ONLY):
            kinds = ["on_wet", "on_coast"]
        elif "loss_parts_kernel" in name or "loss_from_parts_kernel" in name:
            kinds = ["off"]
        else:
            kinds = ["off", "on_wet", "on_coast"]
        ds.sort()
        n, per = len(ds), len(kinds) * (a.warmup + a.steps)
        if n % per:
            print(f"{short} [{n} calls]: not split")
            continue
        c = n // per  # launches per step
        first = len(kinds) * a.warmup * c
        out = []
        for i, kind in enumerate(kinds):
            blk = ds[first + i * a.steps * c:first + (i + 1) * a.steps * c]
            out.append(f"{kind} {sum(e - s for s, e in blk) / len(blk) / 1e3:.1f} us")
        print(f"{short} [{n} calls, {c} a step]: " + ", ".join(out))


if __name__ == "__main__":
    main()
