#!/usr/bin/env python3
"""How fast is RegionSuperResolver.super_resolve?  (DESIGN.md §1 "Overlapped tiles", §6.)

A 1024^2 LR region, one variable, the full rcan-10-20-64 at scale 4, LR tile 48: one
RegionSuperResolver at overlap 0 (22^2 = 484 tiles) and one at overlap 8 (26^2 = 676
tiles), each producing the whole 4096^2 HR field per call (cut + norm, forward, bicubic
baseline of the whole region, blend).  Prints ONE JSON line and writes it to --out:
produced HR MPix/s = 16.78 MPix over the median time of --repeats timed windows of
--regions calls each (device events; the two overlaps alternate window by window, after
--warmup calls each), with the spread of the windows and the device's name.

No pass / fail bar.  The structural expectation next to the measured ratio: the forward
dominates, so overlap 8 should cost about 676 / 484 = 1.40 x overlap 0, and overlap 0
about 484 / 441 = 1.10 x the floor grid's C5 region (bench.py --full, 441 tiles, which
also scores and mosaics four images).
"""
import argparse
import json
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
    ap.add_argument("--side", type=int, default=1024, help="LR region side")
    ap.add_argument("--tile", type=int, default=48)
    ap.add_argument("--overlaps", type=int, nargs="+", default=[0, 8])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--regions", type=int, default=5, help="super_resolve calls per timed window")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--max-batch", type=int, default=None, help="RegionSuperResolver(max_batch=...); default: its own")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "superres_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("superres_bench: no GPU (there is no CPU path to time)")
    from oracle.rcan_oracle import synthetic_hr
    from srmi.engine import NetSpec, param_table
    from srmi.superres import RegionSuperResolver
    from srmi.trainer import default_init_

    dev = torch.device("cuda", 0)
    spec = NetSpec(arch="rcan", nchannels_in=1, nchannels_out=1, nfeatures=64, nlayers=10, nblocks=20, cbottleneck=2,
                   scale=4)
    table = param_table(spec)
    params = torch.empty(sum(t[2] for t in table), dtype=torch.float32, device=dev)
    default_init_(params, table, 0)
    lr = torch.tensor(synthetic_hr(1, 1, a.side, 99)[0]).to(dev)
    kw = {} if a.max_batch is None else {"max_batch": a.max_batch}
    rs = {r: RegionSuperResolver(spec, params, tuple(lr.shape), (a.tile, a.tile), (r, r), device=dev,
                                 graph=not a.no_graph, **kw) for r in a.overlaps}
    for r in a.overlaps:
        for _ in range(a.warmup):
            out = rs[r].super_resolve(lr)
        torch.cuda.synchronize()
        if not bool(torch.isfinite(out["model"]).all()):
            raise SystemExit(f"superres_bench: overlap {r}: non-finite output")
    st = torch.cuda.current_stream()
    ms = {r: [] for r in a.overlaps}
    for _ in range(a.repeats):
        for r in a.overlaps:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(a.regions):
                rs[r].super_resolve(lr)
            e1.record(st)
            e1.synchronize()
            ms[r].append(e0.elapsed_time(e1) / a.regions)
    mpix = (a.side * spec.scale) ** 2 / 1e6
    res = {"tool": "superres_bench", "device": torch.cuda.get_device_name(0),
           "config": {"workload": f"rcan-10-20-64 super_resolve, 1 var, {a.side}^2 LR region -> "
                                  f"{a.side * spec.scale}^2 HR, LR tile {a.tile}", "graph": not a.no_graph,
                      "warmup": a.warmup, "repeats": a.repeats, "regions_per_window": a.regions},
           "hr_mpix_per_region": round(mpix, 3), "overlap": {}}
    for r in a.overlaps:
        med = statistics.median(ms[r])
        res["overlap"][str(r)] = {"tiles": rs[r].n, "engines": rs[r].micro,
                                  "chunk_tiles": [e.batch for e in rs[r].engs], "ms_per_region": round(med, 3),
                                  "ms_min_max": [round(min(ms[r]), 3), round(max(ms[r]), 3)],
                                  "hr_mpix_per_s": round(mpix / (med * 1e-3), 2),
                                  "tiles_per_s": round(rs[r].n / (med * 1e-3), 1)}
    if len(a.overlaps) > 1:
        r0, r1 = a.overlaps[0], a.overlaps[-1]
        res["ratio"] = {"measured_ms": round(statistics.median(ms[r1]) / statistics.median(ms[r0]), 4),
                        "tiles": round(rs[r1].n / rs[r0].n, 4), "of": [r1, r0]}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
