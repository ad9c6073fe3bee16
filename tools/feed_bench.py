#!/usr/bin/env python3
"""Does the time-slice feed keep the fused step fed?  

Writes full-size synthetic LLC4320 inputs (tests/llc_synth.py: a 13 * 4320^2 template,
one '>f4' wet-value file per variable and time slice) and prints ONE JSON line:

* existing:  seconds and bytes per time slice of LLCSource.load_region_data + get_tiles
             (whole-file reads, pageable upload, a host sync for the keep list);
* feed:      the same for srmi.feed.TimesliceFeed alone (nothing trains), with the
             feed's own stage timers;
* train:     C2 (RCAN 10 x 20, two variables, 48 -> 192 tiles) tiles/s of
             harness.train_timeslices over tiles already resident on the device, and
             over the feed, with the same prepare (norm + one xyflip per batch); the
             two are interleaved, --repeats each, in this one process.

The engine is called "not starved" only when the fed / resident ratio of the medians
lies inside the spread of the resident repeats; otherwise the line names the feed stage
(feed.stats()) with the largest share of the fed run's time.  The files were written
moments before they are read, so reads are served by the page cache: the read times say
what the read path costs the host, not what a disk delivers.
"""
import argparse
import json
import os
import random
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "super-resolution-climate_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def log(msg):
    print(f"[feed_bench] {msg}", file=sys.stderr, flush=True)


def write_inputs(root, roi, nvars, nslices):
    import llc_synth
    os.makedirs(root, exist_ok=True)
    tmpl = llc_synth.template(llc_synth.NX, roi)
    tpath = os.path.join(root, "tmpl.data")
    tmpl.astype(">f4").tofile(tpath)
    log(f"template written ({tmpl.size} cells)")
    paths = []
    for i in range(nslices):
        row = []
        for v in range(nvars):
            p = os.path.join(root, f"t{i}_var{v}.data")
            llc_synth.wet_values(tmpl, nvars * i + v).astype(">f4").tofile(p)
            log(f"{p} written")
            row.append(p)
        paths.append(row)
    return tpath, paths


def median(xs):
    return float(statistics.median(xs))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=None, help="directory for the synthetic files (default: a temporary one)")
    ap.add_argument("--keep-files", action="store_true")
    ap.add_argument("--nslices", type=int, default=2)
    ap.add_argument("--roi", type=int, nargs=4, metavar=("Y0", "YS", "X0", "XS"), default=[9500, 2304, 7104, 3072],
                    help="ROI of the [3nx, 4nx] image (default: 12 x 16 tiles of 192 across the east/west seam)")
    ap.add_argument("--tile", type=int, default=192)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--epochs", type=int, default=8, help="passes over the time slices per timed training run")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--readers", type=int, default=2)
    ap.add_argument("--block-words", type=int, default=1024)
    ap.add_argument("--max-gap-blocks", type=int, default=0)
    ap.add_argument("--norm", default="lnorm", choices=["lnorm", "lscale"])
    ap.add_argument("--nlayers", type=int, default=10)
    ap.add_argument("--nblocks", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    from srmi.engine import NetSpec
    from srmi.feed import TimesliceFeed
    from srmi.harness import train_timeslices
    from srmi.llc import LLCSource, get_tiles
    from srmi.trainer import FusedTrainer

    C = 2
    roi = dict(y0=args.roi[0], ys=args.roi[1], x0=args.roi[2], xs=args.roi[3])
    root = args.root or tempfile.mkdtemp(prefix="srmi_feed_bench_")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    try:
        tpath, paths = write_inputs(root, roi, C, args.nslices)
        source = LLCSource(tpath, roi=roi, device=dev)
        log(f"source ready: {source.n_wet} wet values per file, ROI {source.ys} x {source.xs}")

        # (1) the existing path, slice by slice
        t_exist, ntiles = [], []
        for rep in range(2):
            for p in paths:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tiles, _, grid = get_tiles(source.load_region_data(p), args.tile, args.tile)
                torch.cuda.synchronize()
                if rep:
                    t_exist.append(time.perf_counter() - t0)
                    ntiles.append(int(tiles.shape[0]))
        del tiles
        log(f"existing path: {median(t_exist):.3f} s per slice, {ntiles} tiles")

        feed = TimesliceFeed(source, paths, args.tile, depth=args.depth, readers=args.readers,
                             block_words=args.block_words, max_gap_blocks=args.max_gap_blocks)
        with feed:
            plan = feed.plan
            # (2) the feed alone: nothing to overlap with, so this is its latency per slice
            for i in range(args.nslices):
                feed.timeslice(i)
            torch.cuda.synchronize()
            n0 = {k: len(v) for k, v in feed.stats().items()}
            t0 = time.perf_counter()
            for _ in range(3):
                for i in range(args.nslices):
                    feed.timeslice(i)
            torch.cuda.synchronize()
            t_feed = (time.perf_counter() - t0) / (3 * args.nslices)
            st = feed.stats()
            feed_alone = {"s_per_slice": round(t_feed, 5), "bytes_per_slice": C * plan.nbytes,
                          "read_s_median": round(median(st["read_s"][n0["read_s"]:]), 5),
                          "read_wait_s_median": round(median(st["read_wait_s"][n0["read_wait_s"]:]), 5),
                          "enqueue_s_median": round(median(st["enqueue_s"][n0["enqueue_s"]:]), 6),
                          "count_wait_s_median": round(median(st["count_wait_s"][n0["count_wait_s"]:]), 5)}
            log(f"feed alone: {t_feed:.4f} s per slice, {C * plan.nbytes} bytes")

            # (3), (4) training, resident and fed, interleaved
            resident = [feed.timeslice(i)[0].clone() for i in range(args.nslices)]
            spec = NetSpec(arch="rcan", nchannels_in=C, nchannels_out=C, nfeatures=64, nlayers=args.nlayers,
                           nblocks=args.nblocks, cbottleneck=2, scale=4)
            tr = FusedTrainer(spec, args.batch, (args.tile // 4, args.tile // 4), lr=1e-4, device=dev, seed=0)
            prepare = feed.prepare(args.norm)
            sources = {"resident": [lambda i=i: resident[i] for i in range(args.nslices)], "fed": feed.timeslices()}
            per_run = args.epochs * sum(t.shape[0] for t in resident)

            def run(kind, epochs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                train_timeslices(tr, sources[kind], epochs + 1, args.batch, refresh_state=True,
                                 rng=random.Random(17), prepare=prepare, xyflip=True)
                torch.cuda.synchronize()
                return time.perf_counter() - t0

            for kind in sources:
                run(kind, 1)  # warm-up
            rates = {"resident": [], "fed": []}
            fed_stats = []
            for rep in range(args.repeats):
                for kind in ("resident", "fed"):
                    n0 = {k: len(v) for k, v in feed.stats().items()}
                    dt = run(kind, args.epochs)
                    rates[kind].append(per_run / dt)
                    if kind == "fed":
                        s = feed.stats()
                        fed_stats.append({"run_s": round(dt, 4),
                                          "read_s_sum": round(sum(s["read_s"][n0["read_s"]:]), 4),
                                          "read_wait_s_sum": round(sum(s["read_wait_s"][n0["read_wait_s"]:]), 4),
                                          "enqueue_s_sum": round(sum(s["enqueue_s"][n0["enqueue_s"]:]), 4),
                                          "count_wait_s_sum": round(sum(s["count_wait_s"][n0["count_wait_s"]:]), 4)})
                    log(f"repeat {rep} {kind}: {per_run / dt:.1f} tiles/s")
        res_med, fed_med = median(rates["resident"]), median(rates["fed"])
        ratio = fed_med / res_med
        spread = (max(rates["resident"]) - min(rates["resident"])) / res_med
        lo, hi = min(rates["resident"]) / res_med, max(rates["resident"]) / res_med
        inside = ratio >= lo  # (a fed rate above the resident range is no starvation either)
        # the consumer-side stages are host time on the training thread; read_s runs in
        # the reader threads and costs the loop only where read_wait_s shows it
        shares = {k: median([f[k + "_sum"] / f["run_s"] for f in fed_stats]) for k in ("read_wait_s", "enqueue_s", "count_wait_s")}
        rec = {
            "tool": "feed_bench", "device": torch.cuda.get_device_name(dev),
            "inputs": {"nx": 4320, "roi": roi, "variables": C, "time_slices": args.nslices, "tile": args.tile,
                       "tiles_per_slice": ntiles, "n_wet": source.n_wet, "file_bytes": 4 * source.n_wet,
                       "page_cache": "files written by this run just before they are read"},
            "plan": {"block_words": args.block_words, "max_gap_blocks": args.max_gap_blocks,
                     "extents": len(plan.extents), "nbytes_per_file": plan.nbytes,
                     "share_of_file": round(plan.nbytes / (4.0 * source.n_wet), 5)},
            "existing": {"s_per_slice": round(median(t_exist), 5), "bytes_per_slice": C * 4 * source.n_wet},
            "feed": dict(feed_alone, depth=args.depth, readers=args.readers),
            "train": {"config": f"C2: RCAN {args.nlayers} x {args.nblocks}, {C} variables, batch {args.batch}, "
                                f"{args.tile // 4} -> {args.tile} tiles, norm {args.norm}, xyflip",
                      "tiles_per_run": per_run,
                      "resident_tiles_per_s": [round(r, 1) for r in rates["resident"]],
                      "fed_tiles_per_s": [round(r, 1) for r in rates["fed"]],
                      "fed_over_resident": round(ratio, 4),
                      "resident_spread": round(spread, 4), "resident_range_over_median": [round(lo, 4), round(hi, 4)],
                      "not_starved": bool(inside),
                      "fed_runs": fed_stats,
                      "bottleneck": None if inside else max(shares, key=shares.get),
                      # the consumer's feed stages are host time of the training thread: they
                      # explain a shortfall only if together they are as large as it
                      "shortfall": round(max(0.0, 1.0 - ratio), 4),
                      "shortfall_covered_by_consumer_stages": bool(sum(shares.values()) >= 1.0 - ratio),
                      "consumer_stage_share_of_fed_run": {k: round(v, 4) for k, v in shares.items()}},
        }
        line = json.dumps(rec)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
        print(line, flush=True)
    finally:
        if not args.keep_files and args.root is None:
            shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
