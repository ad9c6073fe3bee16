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

--land FRACTION: what does land mode cost?  A synthetic coast (a smooth boundary plus a
few islands, about FRACTION of the pixels dry, NaN) is painted onto the region, and
RegionSuperResolver(land=True) and (land=False) -- the path above, unchanged -- run on it
at the last of --overlaps, window by window in turn, together with a control pair on the
unpainted region (there both modes hand the forward the same number of finite tiles, so
the pair isolates the added kernels from what the tiles' CONTENT does to the forward).
Reports the HR MPix/s of all four, the ratio land on / land off per pair of windows
(median and spread) with and without land, the share of the wet HR pixels each delivers
finite, and the eager time of the three pieces land mode adds or replaces (cut, baseline,
blends); writes profiles/superres_land_bench.json.

--spectra [WINDOW]: what does the spectral score cost?  One RegionSuperResolver at the last
of --overlaps scores a synthetic HR truth: ``score`` and ``score_spectra`` (window WINDOW,
default 256, stride WINDOW / 2) alternate window by window, and the spectral stage alone
(SpectralScore.measure of 'model' and of 'interpolated' against the truth) is timed in a
window of its own.  Reports the median and the spread of each, the stage's share of the
``score_spectra`` call, nused, the effective resolution of both images, and -- the only
baseline there is -- the time of the numpy oracle (tests/spectra_oracle.py, fp64) on the
host for the same two pairs of fields, run once, with the device's largest deviation from
it; writes profiles/spectra_bench.json.

--ssim: what does the SSIM / PSNR score cost?  One RegionSuperResolver at the last of
--overlaps scores a synthetic HR truth: ``score``, ``score_ssim`` (with and without the
maps) and the SSIM stage alone (SSIMScore.measure of 'model' and of 'interpolated' against
the truth, with and without the map) alternate window by window on one device.  Reports the
median and the spread of each, the stage's share of the ``score_ssim`` call and its time
beside ``score``'s, the bytes the stage must move (a and b read once per measure, the map
written when asked for) with the bytes/s that makes, the scores, and -- for context -- the
time of the numpy oracle (tests/ssim_oracle.py, fp64 and fp32) on the host for the same two
pairs of fields, run once, with the device's largest deviation from the fp64 oracle next to
e32, the fp32 oracle's; writes profiles/ssim_bench.json.  No pass / fail bar.

--gradient: what does the gradient score cost?  The same arrangement with ``score_gradient``
and GradientScore.measure: ``score``, ``score_gradient`` (with and without the maps) and the
stage alone alternate window by window.  The bytes the stage must move are both fields read
once per measure plus the two magnitude maps written when asked for (gradient_stage_bytes);
they are reported with the bytes/s they make and the time they take at --hbm-tbs (the
achievable HBM rate): a floor computed from shapes, not measured.  The numpy oracle
(tests/gradient_oracle.py) runs once on the host for the counts and the largest deviation of
the map; writes profiles/gradient_bench.json.  No pass / fail bar.

--fss: what does the fractions skill score cost?  ``score`` and ``score_fss`` (two C = 1 scores,
thresholds from the truth's quantiles on the device) alternate window by window with the stage
alone -- two srmi_fss calls on C = 2 fields, T = 4 thresholds at the truth's quantiles (0.5, 0.9,
0.99, 0.999), scales (1, 3, 5, 9, 17, 33, 65, 129) -- with each of its three launches alone, and
with the windows launch of a one-scale ladder at n = 3 and at n = 255, whose ratio shows that the
cost does not follow n^2.  The bytes each launch must move (fss_launch_bytes) are reported with
the time they take at --hbm-tbs: a floor computed from shapes, not measured.  The numpy oracle
(tests/fss_oracle.py) runs once on the host on one channel and one threshold, where the
device's tables must equal it; writes profiles/fss_bench.json.  No pass / fail bar.

--ensemble-score: what do the member fields and the ensemble score cost?  For K = 4 and 8, two
RegionSuperResolver(ensemble=K), members=True and members=False, on the default region at the
last of --overlaps.  The arms alternate window by window on one device: the region with members
off and on, ``score`` and ``score_ensemble`` (edges from the spread's quantiles on the device),
the K member launches alone, and the score's stage alone -- one srmi_ensemble_score call on the
[K, 1, 4096, 4096] members (B = 10), its main launch alone without and with the CRPS map, and its
finish launch alone.  The bytes the main launch must move, (K + 1) H W 4 (+ H W 4 with the map),
are reported with the time they take at --hbm-tbs: a floor computed from shapes, not measured.
Also reports what the score says of this ensemble; writes profiles/ensemble_score_bench.json.
No pass / fail bar.  The weights are default_init_'s, untrained: the numbers say nothing about
the calibration of a trained network on real data.

--distribution: what does the distribution score cost, and on which data?  One
RegionSuperResolver at the last of --overlaps scores a synthetic HR truth: ``score``,
``score_distribution`` and, window by window in turn on one device, the score's launches alone
(two DistributionScore.measure per stage) beside the SSIM stage (two SSIMScore.measure), on
three inputs because a histogram's cost depends on the data: the tool's two images against
its synthetic truth (white Gaussian noise; the images are smooth), a smooth field (sinusoids
as long as the region, so that a wave's pixels share a bin) and white noise, both over the
truth's range.  Every alternative of the
histogram kernel (one copy of the tables, the copy chosen by the wave, run merging) and
the score with the range given (which drops the range launch) are arms of the same loop.
Reports the median and the spread of each, the bytes/s against reading both fields once, the
scores, and the time of the numpy oracle (tests/distribution_oracle.py) on the host for the
same fields, run once -- the device's tables must equal its tables; writes
profiles/distribution_bench.json.  No pass / fail bar.

--ensemble K [K ...]: what does the self-ensemble cost, and what does it give?  One
RegionSuperResolver(ensemble=K) per K in {1, 4, 8} (1 always among them) on the default
region at the last of --overlaps, the arms alternating window by window.  Reports the HR
MPix/s of each, t(K) / (K t(1)) per pair of neighbouring windows (median and spread; the
forward dominates, so it should sit near 1), the eager time of the two launches the
ensemble adds (srmi_tiles_dihedral, srmi_tiles_blend_ensemble) and their share of the
largest K's region, and -- on a synthetic truth through ``score`` -- the RMSE of 'model' at
each K and the correlation of 'spread' with |model - truth|; writes
profiles/ensemble_bench.json.  The weights are default_init_'s, untrained: the last two
describe the tool's network, not a trained one's gain.

--consistent K [K ...]: what does the consistency correction cost, and what does it leave?
One RegionSuperResolver(consistent=K) per K (0 always among them) on the default region at
the last of --overlaps, the arms alternating window by window on one device.  Reports the
HR MPix/s of each and t(K) / t(0) per pair of neighbouring windows, the eager time of the
launches the largest K adds (residual, K iterations, apply) with the bytes/s they achieve
against 3 C (s h) (s w) 4 bytes (one read of the HR field, one read-modify-write), the rms
of 'residual' and of 'residual_left', the rms of D('model') - input through the existing
downsample, and ``score``'s RMSE against a synthetic truth for every arm; writes
profiles/consistency_bench.json.  No pass / fail bar: none of it had been measured before,
and the weights are default_init_'s, untrained -- the residuals and RMSEs describe the
tool's network, not a trained one.

--quantile-map: what does the quantile map cost, and what does it move?  A
srmi.quantile_map.QuantileMap (256 bins, on="detail", tail_count 16) is fitted by
``fit_quantile_map`` on one synthetic region and applied to another seed.  Reports the eager
times of accumulate, fit and apply alone with the bytes each must move (accumulate: three
reads of the field; apply: two reads and one write; value mode one read fewer) and the bytes/s
they achieve beside the achievable bandwidth DESIGN.md section 3 uses, on the tool's images, a
smooth field and white noise; srmi_distribution's range pass (two reads, nothing else),
measured in the same run, as the pure-read yardstick; the region time with the map on and
off, the arms alternating window by window on one device, beside the spread of the off
windows; and 'q_bias', 'pss', 'w1' and the RMSE of 'model' against the held-out truth before
and after, with consistent 0 and 3; writes profiles/quantile_map_bench.json.  No pass / fail
bar.  The weights are default_init_'s, untrained: the numbers show the mechanism and make no
claim of skill on real data.
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


def paint_coast(lr, fraction):
    """NaN on about `fraction` of lr [1, n, n]: the land right of a smooth coastline (85 %
    of it) and five round islands in the sea."""
    n = lr.shape[-1]
    yy, xx = torch.meshgrid(torch.arange(n, device=lr.device), torch.arange(n, device=lr.device), indexing="ij")
    yy, xx = yy.float(), xx.float()
    coast = n * (1.0 - 0.85 * fraction) + 0.03 * n * torch.sin(yy * (2 * math.pi * 3 / n)) \
        + 0.01 * n * torch.sin(yy * (2 * math.pi * 17 / n))
    dry = xx >= coast
    r = math.sqrt(0.15 * fraction * n * n / (5 * math.pi))
    for k in range(5):
        cy, cx = n * (0.12 + 0.19 * k), n * (0.15 + 0.11 * ((3 * k) % 5))
        dry |= (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
    out = lr.clone()
    out[0][dry] = float("nan")
    return out


def timed(fn, reps=20):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def land_main(a, spec, params, lr, dev, kw):
    from srmi.engine import upsample
    from srmi.superres import RegionSuperResolver
    r = a.overlaps[-1]
    sea = lr  # the control: the same field without land, where both modes feed the forward the same tiles
    lr = paint_coast(lr, a.land)
    # (land mode, region): the pair the issue asks for, and the control pair on the unpainted region
    modes = {"on": (True, lr), "off": (False, lr), "on_sea": (True, sea), "off_sea": (False, sea)}
    rs = {m: RegionSuperResolver(spec, params, tuple(lr.shape), (a.tile, a.tile), (r, r), device=dev,
                                 graph=not a.no_graph, land=land, **kw) for m, (land, _) in modes.items()}
    s = spec.scale
    share = {}
    for m, (_, reg) in modes.items():
        for _ in range(a.warmup):
            out = rs[m].super_resolve(reg)
        torch.cuda.synchronize()
        wet_hr = torch.isfinite(reg).repeat_interleave(s, 1).repeat_interleave(s, 2)
        share[m] = float((torch.isfinite(out["model"]) & wet_hr).sum()) / float(wet_hr.sum())
    st = torch.cuda.current_stream()
    ms = {m: [] for m in modes}
    for _ in range(a.repeats):
        for m, (_, reg) in modes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(a.regions):
                rs[m].super_resolve(reg)
            e1.record(st)
            e1.synchronize()
            ms[m].append(e0.elapsed_time(e1) / a.regions)
    ratios = [x / y for x, y in zip(ms["on"], ms["off"])]
    ratios_sea = [x / y for x, y in zip(ms["on_sea"], ms["off_sea"])]
    on, off = rs["on"], rs["off"]
    pieces = {"cut": [timed(on._cut), timed(off._cut)],
              "baseline": [timed(lambda: (upsample(on.tiles, s, out=on.up, mode=on.umode),
                                          on._blend_masked(on.up, on.images["interpolated"]))),
                           timed(lambda: upsample(off.region[None], s, out=off.images["interpolated"][None],
                                                  mode=off.umode))],
              "blend": [timed(on._blend), timed(off._blend)]}
    mpix = (a.side * s) ** 2 / 1e6
    res = {"tool": "superres_bench --land", "device": torch.cuda.get_device_name(0),
           "config": {"workload": f"rcan-10-20-64 super_resolve, 1 var, {a.side}^2 LR region with a coast -> "
                                  f"{a.side * s}^2 HR, LR tile {a.tile}, overlap {r}", "graph": not a.no_graph,
                      "warmup": a.warmup, "repeats": a.repeats, "regions_per_window": a.regions,
                      "land_fraction_asked": a.land, "dry_share": round(1.0 - float(torch.isfinite(lr).float().mean()), 4),
                      "min_wet": on.min_wet},
           "hr_mpix_per_region": round(mpix, 3), "land": {}}
    for m in modes:
        med = statistics.median(ms[m])
        res["land"][m] = {
            "tiles": rs[m].n, "bad_tiles": int(rs[m].bad.sum()), "ms_per_region": round(med, 3),
            "ms_min_max": [round(min(ms[m]), 3), round(max(ms[m]), 3)], "hr_mpix_per_s": round(mpix / (med * 1e-3), 2),
            "wet_hr_share_finite": round(share[m], 5)}
    res["ratio_on_over_off"] = {"median": round(statistics.median(ratios), 4),
                                "min_max": [round(min(ratios), 4), round(max(ratios), 4)]}
    res["ratio_on_over_off_without_land"] = {"median": round(statistics.median(ratios_sea), 4),
                                             "min_max": [round(min(ratios_sea), 4), round(max(ratios_sea), 4)]}
    res["pieces_eager_ms_on_off"] = {k: [round(v[0], 4), round(v[1], 4)] for k, v in pieces.items()}
    return res


def spectra_main(a, spec, params, dev, kw):
    import time

    import numpy as np
    from oracle.rcan_oracle import synthetic_hr
    from srmi.spectra import effective_resolution
    from srmi.superres import RegionSuperResolver
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import spectra_oracle as so
    r, s, P = a.overlaps[-1], spec.scale, a.spectra
    hr = torch.tensor(synthetic_hr(1, 1, a.side * s, 98)[0]).to(dev)
    rs = RegionSuperResolver(spec, params, (1, a.side, a.side), (a.tile, a.tile), (r, r), device=dev,
                             graph=not a.no_graph, **kw)
    for _ in range(a.warmup):
        images, losses, spectra = rs.score_spectra(hr, window=P)
    torch.cuda.synchronize()
    scorers = rs._spectra[(P, None)]

    def stage():
        for name, sc in scorers.items():
            sc.measure(images[name], hr)

    runs = {"score": lambda: rs.score(hr), "score_spectra": lambda: rs.score_spectra(hr, window=P), "stage": stage}
    st = torch.cuda.current_stream()
    ms = {k: [] for k in runs}
    for _ in range(a.repeats):
        for k, fn in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(a.regions):
                fn()
            e1.record(st)
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.regions)
    images, losses, spectra = rs.score_spectra(hr, window=P)
    torch.cuda.synchronize()
    truth = hr.cpu().numpy()
    host, dev_err = 0.0, {}
    for name in ("model", "interpolated"):
        img = images[name].cpu().numpy()
        t0 = time.perf_counter()
        o64, n64 = so.spectra(img, truth, P, P // 2)
        host += time.perf_counter() - t0
        got = scorers[name].out.cpu().numpy().astype(np.float64)
        dev_err[name] = float((np.abs(got - o64) / (o64[:, 0] + o64[:, 1])[:, None]).max())
        if int(spectra[name]["nused"].item()) != n64:
            raise SystemExit(f"superres_bench: {name}: nused {int(spectra[name]['nused'].item())} != oracle {n64}")
    med = {k: statistics.median(v) for k, v in ms.items()}
    sc0 = scorers["model"]
    res = {"tool": "superres_bench --spectra", "device": torch.cuda.get_device_name(0),
           "config": {"workload": f"rcan-10-20-64 score_spectra, 1 var, {a.side}^2 LR region -> {a.side * s}^2 HR, LR "
                                  f"tile {a.tile}, overlap {r}; two spectral scores (model, interpolated) per call",
                      "graph": not a.no_graph, "warmup": a.warmup, "repeats": a.repeats,
                      "regions_per_window": a.regions, "window": P, "stride": sc0.stride,
                      "windows": int(so.origins(a.side * s, P, sc0.stride).size) ** 2,
                      "workspace_mib_per_score": round(sc0.workspace.numel() / 2 ** 20, 1)},
           "ms": {k: {"median": round(med[k], 3), "min_max": [round(min(v), 3), round(max(v), 3)]}
                  for k, v in ms.items()},
           "stage_share_of_score_spectra": round(med["stage"] / med["score_spectra"], 4),
           "score_spectra_over_score": round(med["score_spectra"] / med["score"], 4),
           "nused": int(spectra["model"]["nused"].item()),
           "effective_resolution_px": {k: effective_resolution(spectra[k]["error_ratio"], P)
                                       for k in ("model", "interpolated")},
           "host_oracle_fp64_s": round(host, 2),
           "device_vs_oracle_max_rel": {k: float(f"{v:.3e}") for k, v in dev_err.items()}}
    return res


def ssim_main(a, spec, params, dev, kw):
    import time

    import numpy as np
    from oracle.rcan_oracle import synthetic_hr
    from srmi.ssim import SSIMScore
    from srmi.superres import RegionSuperResolver
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ssim_oracle as so
    r, s = a.overlaps[-1], spec.scale
    side = a.side * s
    hr = torch.tensor(synthetic_hr(1, 1, side, 98)[0]).to(dev)
    rs = RegionSuperResolver(spec, params, (1, a.side, a.side), (a.tile, a.tile), (r, r), device=dev,
                             graph=not a.no_graph, **kw)
    for _ in range(a.warmup):
        images, losses, ssim = rs.score_ssim(hr, maps=True)
        rs.score_ssim(hr)
    torch.cuda.synchronize()
    names = ("model", "interpolated")
    scorers = {True: rs._ssim[(None, True)], False: rs._ssim[(None, False)]}

    def stage(maps):
        for name in names:
            scorers[maps][name].measure(images[name], hr)

    runs = {"score": lambda: rs.score(hr), "score_ssim": lambda: rs.score_ssim(hr),
            "score_ssim_maps": lambda: rs.score_ssim(hr, maps=True), "stage": lambda: stage(False),
            "stage_maps": lambda: stage(True)}
    st = torch.cuda.current_stream()
    ms = {k: [] for k in runs}
    for _ in range(a.repeats):  # the arms alternate window by window
        for k, fn in runs.items():
            n = a.regions * (20 if k.startswith("stage") else 1)  # a window of the stage alone is many calls
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(n):
                fn()
            e1.record(st)
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / n)
    images, losses, ssim = rs.score_ssim(hr, maps=True)
    torch.cuda.synchronize()
    truth = hr.cpu().numpy()
    host = {"float64": 0.0, "float32": 0.0}
    dev_err, e32s, scores = {}, {}, {}
    for name in names:
        img = images[name].cpu().numpy()
        t0 = time.perf_counter()
        o64 = so.ssim(img, truth)
        host["float64"] += time.perf_counter() - t0
        t0 = time.perf_counter()
        o32 = so.ssim(img, truth, dtype=np.float32)
        host["float32"] += time.perf_counter() - t0
        got = ssim[name]["map"].cpu().numpy().astype(np.float64)
        counts = (int(ssim[name]["nwin"].item()), int(ssim[name]["npix"].item()))
        if counts != (int(o64["nwin"][0]), int(o64["npix"][0])):
            raise SystemExit(f"superres_bench: {name}: counts differ from the oracle's")
        dev_err[name] = float(np.nanmax(np.abs(got - o64["map"])))
        e32s[name] = float(np.nanmax(np.abs(o32["map"].astype(np.float64) - o64["map"])))
        scores[name] = {q: float(ssim[name][q]) for q in ("ssim", "cs", "psnr", "mse", "data_range")}
        scores[name]["rmse_of_score"] = float(losses[name])
    med = {k: statistics.median(v) for k, v in ms.items()}
    px = float(side) ** 2
    nbytes = {"stage": 2 * 2 * 4 * px, "stage_maps": 2 * 3 * 4 * px}  # two measures: a, b read once (+ the map written)
    sc0 = scorers[True]["model"]
    res = {"tool": "superres_bench --ssim", "device": torch.cuda.get_device_name(0),
           "config": {"workload": f"rcan-10-20-64 score_ssim, 1 var, {a.side}^2 LR region -> {side}^2 HR, LR tile "
                                  f"{a.tile}, overlap {r}; two SSIM scores (model, interpolated) per call",
                      "graph": not a.no_graph, "warmup": a.warmup, "repeats": a.repeats,
                      "regions_per_window": a.regions, "stage_calls_per_window": a.regions * 20,
                      "workspace_mib_per_score": round(sc0.workspace.numel() / 2 ** 20, 2)},
           "ms": {k: {"median": round(med[k], 4), "min_max": [round(min(v), 4), round(max(v), 4)]}
                  for k, v in ms.items()},
           "stage_share_of_score_ssim": round(med["stage"] / med["score_ssim"], 5),
           "stage_maps_share_of_score_ssim_maps": round(med["stage_maps"] / med["score_ssim_maps"], 5),
           "stage_over_score": round(med["stage"] / med["score"], 5),
           "score_ssim_over_score": round(med["score_ssim"] / med["score"], 4),
           "stage_bytes": {k: int(v) for k, v in nbytes.items()},
           "stage_gb_per_s": {k: round(v / (med[k] * 1e-3) / 1e9, 1) for k, v in nbytes.items()},
           "scores": scores, "nwin": int(ssim["model"]["nwin"].item()),
           "host_oracle_s": {k: round(v, 2) for k, v in host.items()},
           "device_map_vs_oracle_max_abs": {k: float(f"{v:.3e}") for k, v in dev_err.items()},
           "e32_map_max_abs": {k: float(f"{v:.3e}") for k, v in e32s.items()}}
    return res


def gradient_stage_bytes(px: float) -> dict:
    """The bytes the two measures (model, interpolated) of one call must move: both fields read
    once, plus the two magnitude maps written when asked for (fp32)."""
    return {"stage": 2 * 2 * 4 * px, "stage_maps": 2 * 4 * 4 * px}


def gradient_main(a, spec, params, dev, kw):
    import time

    import numpy as np
    from oracle.rcan_oracle import synthetic_hr
    from srmi.superres import RegionSuperResolver
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gradient_oracle as go
    r, s = a.overlaps[-1], spec.scale
    side = a.side * s
    hr = torch.tensor(synthetic_hr(1, 1, side, 98)[0]).to(dev)
    rs = RegionSuperResolver(spec, params, (1, a.side, a.side), (a.tile, a.tile), (r, r), device=dev,
                             graph=not a.no_graph, **kw)
    for _ in range(a.warmup):
        images, losses, grad = rs.score_gradient(hr, maps=True)
        rs.score_gradient(hr)
    torch.cuda.synchronize()
    names = ("model", "interpolated")
    sp = (1.0, 1.0)
    scorers = {True: rs._gradient[(sp, True, None)], False: rs._gradient[(sp, False, None)]}

    def stage(maps):
        for name in names:
            scorers[maps][name][0].measure(images[name], hr)

    runs = {"score": lambda: rs.score(hr), "score_gradient": lambda: rs.score_gradient(hr),
            "score_gradient_maps": lambda: rs.score_gradient(hr, maps=True), "stage": lambda: stage(False),
            "stage_maps": lambda: stage(True)}
    st = torch.cuda.current_stream()
    ms = {k: [] for k in runs}
    for _ in range(a.repeats):  # the arms alternate window by window
        for k, fn in runs.items():
            n = a.regions * (20 if k.startswith("stage") else 1)  # a window of the stage alone is many calls
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(n):
                fn()
            e1.record(st)
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / n)
    images, losses, grad = rs.score_gradient(hr, maps=True)
    torch.cuda.synchronize()
    truth = hr.cpu().numpy()
    host, dev_err, e32s, scores = 0.0, {}, {}, {}
    for name in names:
        img = images[name].cpu().numpy()
        t0 = time.perf_counter()
        o64 = go.score(img, truth)
        host += time.perf_counter() - t0
        o32 = go.score(img, truth, dtype=np.float32)
        if int(grad[name]["count"].item()) != int(o64["count"][0]):
            raise SystemExit(f"superres_bench: {name}: count differs from the oracle's")
        got = grad[name]["gmag_pred"].cpu().numpy().astype(np.float64)
        dev_err[name] = float(np.nanmax(np.abs(got - o64["gmag_pred"])))
        e32s[name] = float(np.nanmax(np.abs(o32["gmag_pred"].astype(np.float64) - o64["gmag_pred"])))
        scores[name] = {q: float(grad[name][q]) for q in go.STATS}
        scores[name]["rmse_of_score"] = float(losses[name])
    med = {k: statistics.median(v) for k, v in ms.items()}
    nbytes = gradient_stage_bytes(float(side) ** 2)
    res = {"tool": "superres_bench --gradient", "device": torch.cuda.get_device_name(0),
           "config": {"workload": f"rcan-10-20-64 score_gradient, 1 var, {a.side}^2 LR region -> {side}^2 HR, LR tile "
                                  f"{a.tile}, overlap {r}; two gradient scores (model, interpolated) per call",
                      "network": "untrained (seeded initial weights, synthetic fields)",
                      "graph": not a.no_graph, "warmup": a.warmup, "repeats": a.repeats,
                      "regions_per_window": a.regions, "stage_calls_per_window": a.regions * 20,
                      "workspace_mib_per_score": round(scorers[True]["model"][0].workspace.numel() / 2 ** 20, 2),
                      "hbm_tbs": a.hbm_tbs},
           "ms": {k: {"median": round(med[k], 4), "min_max": [round(min(v), 4), round(max(v), 4)]}
                  for k, v in ms.items()},
           "stage_share_of_score_gradient": round(med["stage"] / med["score_gradient"], 5),
           "stage_maps_share_of_score_gradient_maps": round(med["stage_maps"] / med["score_gradient_maps"], 5),
           "stage_over_score": round(med["stage"] / med["score"], 5),
           "score_gradient_over_score": round(med["score_gradient"] / med["score"], 4),
           "stage_bytes": {k: int(v) for k, v in nbytes.items()},
           "stage_gb_per_s": {k: round(v / (med[k] * 1e-3) / 1e9, 1) for k, v in nbytes.items()},
           "stage_memory_floor_ms": {k: round(v / (a.hbm_tbs * 1e12) * 1e3, 4) for k, v in nbytes.items()},
           "stage_time_over_floor": {k: round(med[k] / (v / (a.hbm_tbs * 1e12) * 1e3), 2) for k, v in nbytes.items()},
           "scores": scores, "count": int(grad["model"]["count"].item()), "host_oracle_fp64_s": round(host, 2),
           "device_map_vs_oracle_max_abs": {k: float(f"{v:.3e}") for k, v in dev_err.items()},
           "e32_map_max_abs": {k: float(f"{v:.3e}") for k, v in e32s.items()}}
    return res


def fss_launch_bytes(C, H, W, T, N):
    """The bytes each launch of one srmi_fss call must move (srmi.h, "the fractions skill
    score"): events reads both fields once and writes the 2 C T bit planes and its partials;
    windows reads the bit planes (once, if every scale shared them) and writes two int64 per
    (channel, threshold, scale, tile); finish reads the partials it sums and writes the tables."""
    from srmi.fss import FSS_TILE
    px, ww = H * W, -(-W // 64)
    planes = 2 * C * T * H * ww * 8
    evb = -(-(H * ww) // 32)  # workgroups of the events launch per channel
    evp = C * (1 + 2 * T) * evb * 4
    winp = C * T * N * -(-H // FSS_TILE[0]) * ww * 16
    return {"events": 2 * 4 * C * px + planes + evp, "windows": planes + winp,
            "finish": C * T * 3 * evb * 4 + winp + C * T * (2 * N * 8 + 16 + (N + 6) * 8) + C * 8}


def fss_main(a, spec, params, dev, kw):
    import time

    import numpy as np
    from oracle.rcan_oracle import synthetic_hr
    from srmi.distribution import DistributionScore
    from srmi.fss import EVENTS, FINISH, WINDOWS, FractionsSkillScore
    from srmi.superres import RegionSuperResolver
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import fss_oracle as fo
    r, s = a.overlaps[-1], spec.scale
    side = a.side * s
    probs, scales = (0.5, 0.9, 0.99, 0.999), (1, 3, 5, 9, 17, 33, 65, 129)
    hr = torch.tensor(synthetic_hr(1, 1, side, 98)[0]).to(dev)
    rs = RegionSuperResolver(spec, params, (1, a.side, a.side), (a.tile, a.tile), (r, r), device=dev,
                             graph=not a.no_graph, **kw)
    for _ in range(a.warmup):
        images, losses, _ = rs.score_fss(hr, probs=probs, scales=scales)
    torch.cuda.synchronize()
    # the stage alone on C = 2: (model, interpolated) against (truth, truth), and the two swapped
    Cn, T, N = 2, len(probs), len(scales)
    shape = (Cn, side, side)
    pairs = [(torch.cat([images["model"], images["interpolated"]]).contiguous(), torch.cat([hr, hr]).contiguous()),
             (torch.cat([images["interpolated"], images["model"]]).contiguous(), torch.cat([hr, hr]).contiguous())]
    thr = DistributionScore(shape, 1024, 0, probs, device=dev).measure(*pairs[0])["q_truth"].float().contiguous()
    scorers = [FractionsSkillScore(shape, thr, scales, device=dev) for _ in pairs]
    small = [FractionsSkillScore(shape, thr, (3,), device=dev) for _ in pairs]
    large = [FractionsSkillScore(shape, thr, (255,), device=dev) for _ in pairs]

    def stage(objs, launches=0):
        def fn():
            for sc, (p, t) in zip(objs, pairs):
                sc.measure(p, t, launches)
        return fn
    runs = {"score": lambda: rs.score(hr), "score_fss": lambda: rs.score_fss(hr, probs=probs, scales=scales),
            "stage": stage(scorers), "stage_events": stage(scorers, EVENTS), "stage_windows": stage(scorers, WINDOWS),
            "stage_finish": stage(scorers, FINISH), "windows_all_3": stage(small, WINDOWS),
            "windows_all_255": stage(large, WINDOWS)}
    for k, fn in runs.items():
        if k != "score":
            fn()  # every workspace holds a whole call's bit planes and partials before a launch runs alone
    for fn in (stage(small), stage(large)):
        fn()
    torch.cuda.synchronize()
    st = torch.cuda.current_stream()
    ms = {k: [] for k in runs}
    for _ in range(a.repeats):  # the arms alternate window by window
        for k, fn in runs.items():
            n = a.regions * (1 if k.startswith("score") else 4)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(n):
                fn()
            e1.record(st)
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / n)
    res0 = {k: v.cpu().numpy().copy() for k, v in scorers[0].measure(*pairs[0]).items()}
    torch.cuda.synchronize()
    p0, t0 = pairs[0][0][:1].cpu().numpy(), pairs[0][1][:1].cpu().numpy()
    thr0 = thr[:1, 1:2].cpu().numpy()
    tic = time.perf_counter()
    o = fo.fss(p0, t0, thr0, scales)  # one channel and one threshold of the 2 x 4: an eighth of one measure
    host = time.perf_counter() - tic
    if not (np.array_equal(o["num"][0, 0], res0["num"][0, 1]) and np.array_equal(o["den"][0, 0], res0["den"][0, 1])
            and o["used"][0] == res0["used"][0]):
        raise SystemExit("superres_bench: the tables differ from the oracle's")
    med = {k: statistics.median(v) for k, v in ms.items()}
    per_call = fss_launch_bytes(Cn, side, side, T, N)
    nbytes = {"stage_" + k: 2 * v for k, v in per_call.items()}  # two measures per stage call
    nbytes["stage"] = sum(nbytes.values())
    return {"tool": "superres_bench --fss", "device": torch.cuda.get_device_name(0),
            "config": {"workload": f"rcan-10-20-64 score_fss, 1 var, {a.side}^2 LR region -> {side}^2 HR, LR tile {a.tile}, "
                                   f"overlap {r}: two C = 1 scores (model, interpolated) per score_fss call, thresholds "
                                   "from the truth's quantiles on the device; the stage arms: two srmi_fss calls on C = 2 "
                                   f"fields [2, {side}, {side}] ((model, interpolated) and the two swapped, against the "
                                   "truth twice)",
                       "probs": list(probs), "scales": list(scales), "T": T, "N": N,
                       "network": "untrained (seeded initial weights, synthetic fields)",
                       "graph": not a.no_graph, "warmup": a.warmup, "repeats": a.repeats,
                       "regions_per_window": a.regions, "stage_calls_per_window": a.regions * 4,
                       "workspace_mib_per_score": round(scorers[0].workspace.numel() / 2 ** 20, 2), "hbm_tbs": a.hbm_tbs},
            "ms": {k: {"median": round(med[k], 4), "min_max": [round(min(v), 4), round(max(v), 4)]} for k, v in ms.items()},
            "score_fss_over_score": round(med["score_fss"] / med["score"], 4),
            "stage_over_score": round(med["stage"] / med["score"], 5),
            "launch_bytes": {k: int(v) for k, v in nbytes.items()},
            "launch_memory_floor_ms": {k: round(v / (a.hbm_tbs * 1e12) * 1e3, 5) for k, v in nbytes.items()},
            "launch_time_over_floor": {k: round(med[k] / (v / (a.hbm_tbs * 1e12) * 1e3), 2) for k, v in nbytes.items()},
            "windows_all_255_over_all_3": round(med["windows_all_255"] / med["windows_all_3"], 3),
            "n_squared_ratio_255_over_3": round((255 / 3) ** 2, 1),
            "fss_model": [round(float(v), 5) for v in res0["fss"][0, 1]],
            "fss_interpolated": [round(float(v), 5) for v in res0["fss"][1, 1]],
            "skilful_scale": res0["skilful_scale"].tolist(), "used": res0["used"].tolist(),
            "host_oracle_s_one_channel_one_threshold": round(host, 2),
            "host_oracle_s_two_measures_extrapolated": round(host * Cn * T * 2, 1),
            "tables_equal_the_oracle_on_that_slice": True}


def distribution_main(a, spec, params, dev, kw):
    import time

    import numpy as np
    from oracle.rcan_oracle import synthetic_hr
    from srmi.distribution import COPY_BY_WAVE, MERGE_RUNS, ONE_COPY, DistributionScore
    from srmi.ssim import SSIMScore
    from srmi.superres import RegionSuperResolver
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import distribution_oracle as do
    r, s = a.overlaps[-1], spec.scale
    side = a.side * s
    shape = (1, side, side)
    hr = torch.tensor(synthetic_hr(1, 1, side, 98)[0]).to(dev)
    rs = RegionSuperResolver(spec, params, (1, a.side, a.side), (a.tile, a.tile), (r, r), device=dev,
                             graph=not a.no_graph, **kw)
    for _ in range(a.warmup):
        images, losses, dist = rs.score_distribution(hr)
    torch.cuda.synchronize()
    names = ("model", "interpolated")
    # the inputs: the tool's two images against its synthetic truth (white Gaussian noise; the
    # images are smooth), a smooth field (a few sinusoids as long as the region, the prediction
    # pulled to the mean or shifted) and white noise, both over the truth's range
    lo, hi = float(hr.min()), float(hr.max())
    g = torch.Generator(device=dev).manual_seed(7)
    wtruth = lo + (hi - lo) * torch.rand(shape, device=dev, generator=g)
    y = torch.arange(side, device=dev, dtype=torch.float64)[:, None] / side
    x = torch.arange(side, device=dev, dtype=torch.float64)[None, :] / side
    t = (torch.sin(2 * math.pi * (y / 1.7 + x / 3.1)) + 0.5 * torch.sin(2 * math.pi * (y / 0.9 - x / 1.3) + 1.0)
         + 0.25 * torch.cos(2 * math.pi * (y / 0.6 + x / 0.45)))
    t = (t - t.min()) / (t.max() - t.min())  # 0 .. 1
    struth = (lo + (hi - lo) * t).float()[None].contiguous()
    pairs = {"synthetic": [(images[n].clone(), hr) for n in names],
             "smooth": [((lo + (hi - lo) * (0.1 + 0.8 * t)).float()[None].contiguous(), struth),
                        ((lo + (hi - lo) * (t + 0.02)).float()[None].contiguous(), struth)],
             "white": [((wtruth + 0.05 * (hi - lo) * torch.randn(shape, device=dev, generator=g)).contiguous(), wtruth)
                       for _ in names]}
    variants = {"stage": 0, "one_copy": ONE_COPY, "copy_by_wave": COPY_BY_WAVE, "merge_runs": MERGE_RUNS,
                "merge_runs_one_copy": MERGE_RUNS | ONE_COPY}
    scorers = {k: [DistributionScore(shape, device=dev, flags=f) for _ in names] for k, f in variants.items()}
    scorers["given_range"] = [DistributionScore(shape, value_range=(lo, hi), device=dev) for _ in names]
    ssim = [SSIMScore(shape, device=dev) for _ in names]

    def stage(scs, inp):
        def fn():
            for sc, (p, t) in zip(scs, pairs[inp]):
                sc.measure(p, t)
        return fn

    runs = {"score": lambda: rs.score(hr), "score_distribution": lambda: rs.score_distribution(hr)}
    for inp in pairs:
        for k, scs in scorers.items():
            runs[f"{inp}/{k}"] = stage(scs, inp)
        runs[f"{inp}/ssim_stage"] = stage(ssim, inp)
    for fn in runs.values():
        fn()
    torch.cuda.synchronize()
    st = torch.cuda.current_stream()
    ms = {k: [] for k in runs}
    for _ in range(a.repeats):  # the arms alternate window by window
        for k, fn in runs.items():
            n = a.regions * (20 if "/" in k else 1)  # a window of a stage alone is many calls
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(n):
                fn()
            e1.record(st)
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / n)
    med = {k: statistics.median(v) for k, v in ms.items()}
    nbytes = 2 * 2 * 4 * float(side) ** 2  # two measures: a and b read once each
    # the numpy oracle on the same fields, run once, and the device's tables against it
    host, summary = {}, {}
    for inp, prs in pairs.items():
        host[inp] = 0.0
        for name, sc, (p, t) in zip(names, scorers["stage"], prs):
            m = sc.measure(p, t)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            o = do.distribution(p.cpu().numpy(), t.cpu().numpy())
            host[inp] += time.perf_counter() - t0
            for q in ("hist_pred", "hist_truth", "joint", "count"):
                if not np.array_equal(m[q].cpu().numpy(), o[q]):
                    raise SystemExit(f"superres_bench: {inp} {name}: {q} differs from the oracle's")
            err = float(np.nanmax(np.abs(sc.derived.cpu().numpy() - o["derived"])
                                  / np.maximum(np.abs(o["derived"]), hi - lo)))
            occupied = int((o["hist_truth"][0] > 0).sum())
            summary[f"{inp}/{name}"] = {"pss": float(m["pss"]), "w1": float(m["w1"]), "under": float(m["under"]),
                                        "over": float(m["over"]),
                                        "q_bias": [float(f"{v:.5g}") for v in m["q_bias"][0].tolist()],
                                        "derived_vs_oracle_max_rel": float(f"{err:.2e}"),
                                        "occupied_truth_bins": occupied}
    sc0 = scorers["stage"][0]
    res = {"tool": "superres_bench --distribution", "device": torch.cuda.get_device_name(0),
           "config": {"workload": f"rcan-10-20-64 score_distribution, 1 var, {a.side}^2 LR region -> {side}^2 HR, LR "
                                  f"tile {a.tile}, overlap {r}; two distribution scores per call and per stage, "
                                  f"bins {sc0.bins}, joint {sc0.joint}, {len(sc0.probs)} quantiles",
                      "inputs": {"synthetic": "'model' and 'interpolated' against the tool's synthetic truth (white "
                                              "Gaussian noise; the images are smooth)",
                                 "smooth": "sinusoids as long as the region over the truth's range; the prediction "
                                           "pulled to the mean (first score) or shifted by 2 % (second)",
                                 "white": "uniform noise over the truth's range, the prediction that plus 5 % noise"},
                      "graph": not a.no_graph, "warmup": a.warmup, "repeats": a.repeats,
                      "regions_per_window": a.regions, "stage_calls_per_window": a.regions * 20,
                      "workspace_mib_per_score": round(sc0.workspace.numel() / 2 ** 20, 2)},
           "ms": {k: {"median": round(med[k], 4), "min_max": [round(min(v), 4), round(max(v), 4)]}
                  for k, v in ms.items()},
           "stage_bytes": int(nbytes),
           "stage_gb_per_s": {k: round(nbytes / (med[k] * 1e-3) / 1e9, 1) for k in med if "/" in k},
           "stage_share_of_score_distribution": round(med["synthetic/stage"] / med["score_distribution"], 5),
           "stage_over_score": round(med["synthetic/stage"] / med["score"], 5),
           "score_distribution_over_score": round(med["score_distribution"] / med["score"], 4),
           "white_over_smooth": round(med["white/stage"] / med["smooth/stage"], 4),
           "stage_over_ssim_stage": {inp: round(med[f"{inp}/stage"] / med[f"{inp}/ssim_stage"], 4) for inp in pairs},
           "range_launch_ms": {inp: round(med[f"{inp}/stage"] - med[f"{inp}/given_range"], 4) for inp in pairs},
           "scores": summary, "host_oracle_s": {k: round(v, 2) for k, v in host.items()}}
    return res


ACHIEVABLE_TB_PER_S = 6.3


def quantile_map_main(a, spec, params, dev, kw):
    from oracle.rcan_oracle import synthetic_hr
    from srmi.distribution import DistributionScore
    from srmi.quantile_map import QuantileMap
    from srmi.superres import RegionSuperResolver
    r, s = a.overlaps[-1], spec.scale
    side = a.side * s
    shape = (1, side, side)
    hr_fit = torch.tensor(synthetic_hr(1, 1, side, 98)[0]).to(dev)
    hr_test = torch.tensor(synthetic_hr(1, 1, side, 97)[0]).to(dev)
    BINS, TAIL, KC = 256, 16, 3

    def make(**more):
        return RegionSuperResolver(spec, params, (1, a.side, a.side), (a.tile, a.tile), (r, r), device=dev,
                                   graph=not a.no_graph, **more, **kw)

    off = {0: make(), KC: make(consistent=KC)}
    qm = off[0].fit_quantile_map([hr_fit], bins=BINS, on="detail", tail_count=TAIL)
    on = {K: make(consistent=K, quantile_map=qm) for K in off}
    arms = {"off": off[0], "on": on[0], f"off_consistent{KC}": off[KC], f"on_consistent{KC}": on[KC]}

    # ---- what the map moves: the scores of 'model' against the held-out truth, every arm
    def scores(rs):
        images, losses, dist = rs.score_distribution(hr_test)
        m = dist["model"]
        return {"rmse_model": float(losses["model"]), "rmse_interpolated": float(losses["interpolated"]),
                "pss": float(m["pss"]), "w1": float(m["w1"]), "under": float(m["under"]), "over": float(m["over"]),
                "q_bias": [float(f"{v:.5g}") for v in m["q_bias"][0].tolist()]}

    truth = {k: scores(rs) for k, rs in arms.items()}
    probs = list(off[0]._distribution[next(iter(off[0]._distribution))]["model"].probs)
    flat = int((qm.knots[0, 1:] == qm.knots[0, :-1]).sum())
    lr_test = off[0].images["input"].clone()

    # ---- the region with the map on and off, the arms alternating window by window
    for rs in arms.values():
        for _ in range(a.warmup):
            out = rs.super_resolve(lr_test)
        torch.cuda.synchronize()
        if not bool(torch.isfinite(out["model"]).all()):
            raise SystemExit("superres_bench: quantile map: non-finite output")
    st = torch.cuda.current_stream()
    ms = {k: [] for k in arms}
    for _ in range(a.repeats):
        for k, rs in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(a.regions):
                rs.super_resolve(lr_test)
            e1.record(st)
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.regions)
    med = {k: statistics.median(v) for k, v in ms.items()}

    # ---- the launches alone, eager, on three kinds of field
    lo, hi = float(hr_test.min()), float(hr_test.max())
    g = torch.Generator(device=dev).manual_seed(7)
    y = torch.arange(side, device=dev, dtype=torch.float64)[:, None] / side
    x = torch.arange(side, device=dev, dtype=torch.float64)[None, :] / side
    t = (torch.sin(2 * math.pi * (y / 1.7 + x / 3.1)) + 0.5 * torch.sin(2 * math.pi * (y / 0.9 - x / 1.3) + 1.0)
         + 0.25 * torch.cos(2 * math.pi * (y / 0.6 + x / 0.45)))
    t = (t - t.min()) / (t.max() - t.min())  # 0 .. 1
    images = off[0].super_resolve(lr_test)
    fields = {  # kind -> (src, truth, base); the detail is src - base
        "synthetic": (images["model"].clone(), hr_test, images["interpolated"].clone()),
        "smooth": ((lo + (hi - lo) * (0.1 + 0.8 * t)).float()[None].contiguous(),
                   (lo + (hi - lo) * t).float()[None].contiguous(),
                   torch.full(shape, lo + 0.5 * (hi - lo), device=dev)),
        "white": (lo + (hi - lo) * torch.rand(shape, device=dev, generator=g),
                  lo + (hi - lo) * torch.rand(shape, device=dev, generator=g),
                  torch.full(shape, lo + 0.5 * (hi - lo), device=dev))}
    HW4 = 4.0 * side * side
    launches = {}
    for kind, (src, tr, base) in fields.items():
        d = src - base
        rng_ = (float(d.min()), float(d.max()) + 1e-3)
        q = {"detail": QuantileMap(1, rng_, bins=BINS, on="detail", tail_count=TAIL, device=dev),
             "value": QuantileMap(1, (lo, hi), bins=BINS, on="value", tail_count=TAIL, device=dev)}
        out = torch.empty_like(src)
        for mode, m in q.items():
            b = base if mode == "detail" else None
            nread = 3 if mode == "detail" else 2

            def acc(m=m, b=b):
                m.reset()
                m.accumulate(src, tr, b)
            t_acc = timed(acc)
            t_fit = timed(m.fit)
            t_app = timed(lambda m=m, b=b: m.apply(src, b, out=out))
            work = src.clone()
            t_inp = timed(lambda m=m, b=b: m.apply(work, b, out=work))
            moved = float((out - src).abs().mean())
            launches[f"{kind}/{mode}"] = {
                "accumulate_ms": round(t_acc, 4), "accumulate_bytes": int(nread * HW4),
                "accumulate_gb_per_s": round(nread * HW4 / (t_acc * 1e-3) / 1e9, 1),
                "fit_ms": round(t_fit, 4), "fit_bytes": int(2 * (BINS + 2) * 8 + (BINS + 3) * 12 + 16),
                "apply_ms": round(t_app, 4), "apply_in_place_ms": round(t_inp, 4), "apply_bytes": int(nread * HW4),
                "apply_gb_per_s": round(nread * HW4 / (t_app * 1e-3) / 1e9, 1),
                "apply_share_of_achievable": round(nread * HW4 / (t_app * 1e-3) / 1e12 / ACHIEVABLE_TB_PER_S, 3),
                "mean_abs_correction": float(f"{moved:.4g}")}
        # the pure-read yardstick: srmi_distribution with and without its range pass, which reads two fields
        free = DistributionScore(shape, bins=BINS, joint=0, device=dev)
        given = DistributionScore(shape, bins=BINS, joint=0, value_range=(lo, hi), device=dev)
        t_free, t_given = timed(lambda: free.measure(src, tr)), timed(lambda: given.measure(src, tr))
        t_range = t_free - t_given  # a difference of two timings: it carries the noise of both
        launches[f"{kind}/range_pass"] = {
            "ms": round(t_range, 4), "score_ms": round(t_free, 4), "score_given_range_ms": round(t_given, 4),
            "bytes": int(2 * HW4),
            "gb_per_s": round(2 * HW4 / (t_range * 1e-3) / 1e9, 1) if t_range > 0 else None}

    mpix = side * side / 1e6
    ratios = {k: [p / q for p, q in zip(ms["on" + k], ms["off" + k])] for k in ("", f"_consistent{KC}")}
    spread_off = {k: round((max(ms["off" + k]) - min(ms["off" + k])) / med["off" + k], 5) for k in ratios}
    return {"tool": "superres_bench --quantile-map", "device": torch.cuda.get_device_name(0),
            "config": {"workload": f"rcan-10-20-64 super_resolve, 1 var, {a.side}^2 LR region -> {side}^2 HR, LR tile "
                                   f"{a.tile}, overlap {r}; QuantileMap bins {BINS}, on=detail, tail_count {TAIL}, "
                                   f"fitted on one synthetic region (seed 98), applied to another (seed 97)",
                       "graph": not a.no_graph, "warmup": a.warmup, "repeats": a.repeats,
                       "regions_per_window": a.regions, "achievable_tb_per_s": ACHIEVABLE_TB_PER_S,
                       "fields": {"synthetic": "'model', the synthetic truth and 'interpolated' of the held-out region",
                                  "smooth": "sinusoids as long as the region, the source pulled to the mean, a "
                                            "constant base", "white": "uniform noise, a constant base"},
                       "weights": "default_init_ (untrained): the numbers show the mechanism and make no claim of "
                                  "skill on real data; no pass / fail bar"},
            "hr_mpix_per_region": round(mpix, 3),
            "region_ms": {k: {"median": round(med[k], 3), "min_max": [round(min(v), 3), round(max(v), 3)]}
                          for k, v in ms.items()},
            "on_over_off": {("consistent0" if k == "" else k[1:]): {
                "median": round(statistics.median(v), 5), "min_max": [round(min(v), 5), round(max(v), 5)],
                "spread_of_off_windows": spread_off[k]} for k, v in ratios.items()},
            "map": {"range": [float(v) for v in qm.range[0]], "count": int(qm.count[0]),
                    "shift_below": float(qm.meta[0, 2]), "shift_above": float(qm.meta[0, 3]),
                    "flat_knot_intervals": flat}, "probs": probs,
            "scores_of_model_against_held_out_truth": truth, "launches": launches}


def ensemble_main(a, spec, params, lr, dev, kw):
    from oracle.rcan_oracle import synthetic_hr
    from srmi.superres import RegionSuperResolver
    r, s = a.overlaps[-1], spec.scale
    Ks = sorted(set([1] + list(a.ensemble)))
    rs = {K: RegionSuperResolver(spec, params, tuple(lr.shape), (a.tile, a.tile), (r, r), device=dev,
                                 graph=not a.no_graph, ensemble=K, **kw) for K in Ks}
    for K in Ks:
        for _ in range(a.warmup):
            out = rs[K].super_resolve(lr)
        torch.cuda.synchronize()
        if not bool(torch.isfinite(out["model"]).all()):
            raise SystemExit(f"superres_bench: ensemble {K}: non-finite output")
    st = torch.cuda.current_stream()
    ms = {K: [] for K in Ks}
    for _ in range(a.repeats):  # the arms alternate window by window
        for K in Ks:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(a.regions):
                rs[K].super_resolve(lr)
            e1.record(st)
            e1.synchronize()
            ms[K].append(e0.elapsed_time(e1) / a.regions)
    mpix = (a.side * s) ** 2 / 1e6
    res = {"tool": "superres_bench --ensemble", "device": torch.cuda.get_device_name(0),
           "config": {"workload": f"rcan-10-20-64 super_resolve, 1 var, {a.side}^2 LR region -> {a.side * s}^2 HR, LR "
                                  f"tile {a.tile}, overlap {r}", "graph": not a.no_graph, "warmup": a.warmup,
                      "repeats": a.repeats, "regions_per_window": a.regions,
                      "weights": "default_init_ (untrained): the RMSE and the correlation say how the ensemble of "
                                 "THIS network behaves, not what a trained one gains"},
           "hr_mpix_per_region": round(mpix, 3), "ensemble": {}}
    for K in Ks:
        med = statistics.median(ms[K])
        ratios = [x / (K * y) for x, y in zip(ms[K], ms[1])]  # per pair of neighbouring windows
        res["ensemble"][str(K)] = {
            "variants": list(rs[K].variants), "forward_tiles": rs[K].nfwd, "engines": rs[K].micro,
            "chunk_tiles": [e.batch for e in rs[K].engs], "ms_per_region": round(med, 3),
            "ms_min_max": [round(min(ms[K]), 3), round(max(ms[K]), 3)], "hr_mpix_per_s": round(mpix / (med * 1e-3), 2),
            "t_over_K_t1": {"median": round(statistics.median(ratios), 4),
                            "min_max": [round(min(ratios), 4), round(max(ratios), 4)]}}
    # the two launches the ensemble adds (the blend replaces the plain one), eager, in the largest K's run
    Kmax = Ks[-1]
    if Kmax > 1:
        big = rs[Kmax]
        expand, blend, plain = timed(big._expand), timed(big._blend), timed(rs[1]._blend)
        total = statistics.median(ms[Kmax])
        hr_px = (a.side * s) ** 2
        res["new_launches"] = {
            "K": Kmax, "dihedral_ms": round(expand, 4), "blend_ensemble_ms": round(blend, 4),
            "plain_blend_ms": round(plain, 4), "share_of_region": round((expand + blend) / total, 5),
            "blend_ensemble_gb_per_s": round(4.0 * (Kmax + 2) * hr_px / (blend * 1e-3) / 1e9, 1),
            "dihedral_gb_per_s": round(4.0 * (Kmax + 1) * big.tiles.numel() / (expand * 1e-3) / 1e9, 1)}
    # a synthetic truth through score: the RMSE of 'model' at each K, and how |model - truth| follows 'spread'
    hr = torch.tensor(synthetic_hr(1, 1, a.side * s, 98)[0]).to(dev)
    res["truth"] = {}
    for K in Ks:
        images, losses = rs[K].score(hr)
        entry = {"rmse_model": float(losses["model"]), "rmse_interpolated": float(losses["interpolated"])}
        if K > 1:
            err, sp = (images["model"] - hr).abs().double().flatten(), images["spread"].double().flatten()
            entry["corr_spread_abs_error"] = round(float(torch.corrcoef(torch.stack([sp, err]))[0, 1]), 4)
            entry["spread_median"] = float(sp.median())
        res["truth"][str(K)] = entry
    return res


def ensemble_score_main(a, spec, params, lr, dev, kw):
    from oracle.rcan_oracle import synthetic_hr
    from srmi.ensemble_score import FINISH, MAIN, EnsembleScore
    from srmi.superres import RegionSuperResolver
    r, s = a.overlaps[-1], spec.scale
    side = a.side * s
    px = side * side
    hr = torch.tensor(synthetic_hr(1, 1, side, 98)[0]).to(dev)
    st = torch.cuda.current_stream()
    res = {"tool": "superres_bench --ensemble-score", "device": torch.cuda.get_device_name(0),
           "config": {"workload": f"rcan-10-20-64, 1 var, {a.side}^2 LR region -> {side}^2 HR, LR tile {a.tile}, overlap "
                                  f"{r}; the stage arms: one srmi_ensemble_score call on members [K, 1, {side}, {side}], "
                                  "B = 10 spread bins at the spread's deciles",
                      "network": "untrained (default_init_, synthetic fields): no claim about calibration on real data",
                      "graph": not a.no_graph, "warmup": a.warmup, "repeats": a.repeats,
                      "regions_per_window": a.regions, "stage_calls_per_window": a.regions * 4, "hbm_tbs": a.hbm_tbs},
           "K": {}}
    for K in (4, 8):
        mk = dict(device=dev, graph=not a.no_graph, ensemble=K, **kw)
        on = RegionSuperResolver(spec, params, tuple(lr.shape), (a.tile, a.tile), (r, r), members=True, **mk)
        off = RegionSuperResolver(spec, params, tuple(lr.shape), (a.tile, a.tile), (r, r), **mk)
        for _ in range(a.warmup):
            off.super_resolve(lr)
            on.super_resolve(lr)
            images, losses, got = on.score_ensemble(hr)
        torch.cuda.synchronize()
        members = images["members"]
        edges = got["edges"].clone()
        plain = EnsembleScore((K, 1, side, side), edges, False, device=dev)
        mapped = EnsembleScore((K, 1, side, side), edges, True, device=dev)
        runs = {"region_members_off": lambda: off.super_resolve(lr), "region_members_on": lambda: on.super_resolve(lr),
                "score": lambda: on.score(hr), "score_ensemble": lambda: on.score_ensemble(hr),
                "member_launches": on._members, "stage": lambda: plain.measure(members, hr),
                "stage_main": lambda: plain.measure(members, hr, MAIN),
                "stage_main_with_map": lambda: mapped.measure(members, hr, MAIN),
                "stage_finish": lambda: plain.measure(members, hr, FINISH)}
        for fn in runs.values():
            fn()  # every workspace holds a whole call's partials before a launch runs alone
        torch.cuda.synchronize()
        ms = {k: [] for k in runs}
        for _ in range(a.repeats):  # the arms alternate window by window
            for k, fn in runs.items():
                n = a.regions * (1 if k.startswith(("region", "score")) else 4)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(n):
                    fn()
                e1.record(st)
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1) / n)
        images, losses, got = on.score_ensemble(hr)
        torch.cuda.synchronize()
        med = {k: statistics.median(v) for k, v in ms.items()}
        nbytes = {"stage_main": (K + 1) * px * 4, "stage_main_with_map": (K + 2) * px * 4}
        ratios = [x / y for x, y in zip(ms["region_members_on"], ms["region_members_off"])]
        res["K"][str(K)] = {
            "ms": {k: {"median": round(med[k], 4), "min_max": [round(min(v), 4), round(max(v), 4)]} for k, v in ms.items()},
            "region_on_over_off": {"median": round(statistics.median(ratios), 5),
                                   "min_max": [round(min(ratios), 5), round(max(ratios), 5)]},
            "score_ensemble_over_score": round(med["score_ensemble"] / med["score"], 5),
            "member_launches_bytes_written": K * px * 4,
            "main_bytes_floor": nbytes,
            "main_memory_floor_ms": {k: round(v / (a.hbm_tbs * 1e12) * 1e3, 5) for k, v in nbytes.items()},
            "main_time_over_floor": {k: round(med[k] / (v / (a.hbm_tbs * 1e12) * 1e3), 2) for k, v in nbytes.items()},
            "main_tb_per_s": {k: round(v / (med[k] * 1e-3) / 1e12, 3) for k, v in nbytes.items()},
            "workspace_kib": round(plain.workspace.numel() / 1024, 1),
            "result": {k: round(float(got[k][0]), 6) for k in ("crps", "crps_fair", "rmse_mean", "spread_rms", "ssr",
                                                                "spread_error_corr", "outliers", "outliers_expected",
                                                                "reliability_index")},
            "rank_hist": got["rank_hist"][0].tolist(), "tied": int(got["tied"][0]), "used": int(got["used"][0]),
            "bin_spread": [round(float(v), 5) for v in got["bin_spread"][0]],
            "bin_rmse": [round(float(v), 5) for v in got["bin_rmse"][0]],
            "rmse_model": float(losses["model"])}
        del runs, fn, on, off, plain, mapped, members, images, got
        torch.cuda.empty_cache()
    return res


def consistency_main(a, spec, params, lr, dev, kw):
    from oracle.rcan_oracle import synthetic_hr
    from srmi.engine import downsample
    from srmi.superres import RegionSuperResolver
    r, s = a.overlaps[-1], spec.scale
    Ks = sorted(set([0] + list(a.consistent)))
    rs = {K: RegionSuperResolver(spec, params, tuple(lr.shape), (a.tile, a.tile), (r, r), device=dev,
                                 graph=not a.no_graph, consistent=K, **kw) for K in Ks}

    def rms(t):
        return float(t.double().pow(2).mean().sqrt())

    left = {}
    for K in Ks:
        for _ in range(a.warmup):
            out = rs[K].super_resolve(lr)
        torch.cuda.synchronize()
        if not bool(torch.isfinite(out["model"]).all()):
            raise SystemExit(f"superres_bench: consistent {K}: non-finite output")
        left[K] = {"rms_D_model_minus_input": rms(downsample(out["model"][None], s, mode=rs[K].dmode)[0] - lr)}
        if K:
            left[K].update(rms_residual=rms(out["residual"]), rms_residual_left=rms(out["residual_left"]))
    st = torch.cuda.current_stream()
    ms = {K: [] for K in Ks}
    for _ in range(a.repeats):  # the arms alternate window by window
        for K in Ks:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(a.regions):
                rs[K].super_resolve(lr)
            e1.record(st)
            e1.synchronize()
            ms[K].append(e0.elapsed_time(e1) / a.regions)
    mpix = (a.side * s) ** 2 / 1e6
    res = {"tool": "superres_bench --consistent", "device": torch.cuda.get_device_name(0),
           "config": {"workload": f"rcan-10-20-64 super_resolve, 1 var, {a.side}^2 LR region -> {a.side * s}^2 HR, LR "
                                  f"tile {a.tile}, overlap {r}", "graph": not a.no_graph, "warmup": a.warmup,
                      "repeats": a.repeats, "regions_per_window": a.regions,
                      "downsample": rs[0].dmode, "upsample": rs[0].umode,
                      "weights": "default_init_ (untrained): the residuals and RMSEs describe THIS network, not a "
                                 "trained one; no pass / fail bar"},
           "hr_mpix_per_region": round(mpix, 3), "consistent": {}}
    for K in Ks:
        med = statistics.median(ms[K])
        ratios = [x / y for x, y in zip(ms[K], ms[0])]  # per pair of neighbouring windows
        res["consistent"][str(K)] = dict(
            ms_per_region=round(med, 3), ms_min_max=[round(min(ms[K]), 3), round(max(ms[K]), 3)],
            hr_mpix_per_s=round(mpix / (med * 1e-3), 2),
            t_over_t0={"median": round(statistics.median(ratios), 4), "min_max": [round(min(ratios), 4),
                                                                                  round(max(ratios), 4)]}, **left[K])
    # a synthetic truth through score: the RMSE of every arm (before the eager timing below rewrites 'model')
    hr = torch.tensor(synthetic_hr(1, 1, a.side * s, 98)[0]).to(dev)
    res["truth"] = {}
    for K in Ks:
        images, losses = rs[K].score(hr)
        res["truth"][str(K)] = {"rmse_model": float(losses["model"]),
                                "rmse_interpolated": float(losses["interpolated"])}
    Kmax = Ks[-1]
    if Kmax > 0:  # the added launches, eager, on the largest K's buffers (each call corrects 'model' once more)
        t = timed(rs[Kmax]._correct)
        nbytes = 3.0 * lr.shape[0] * (a.side * s) ** 2 * 4
        res["new_launches"] = {"K": Kmax, "launches": Kmax + 2, "ms": round(t, 4), "bytes_model": int(nbytes),
                               "gb_per_s": round(nbytes / (t * 1e-3) / 1e9, 1),
                               "share_of_region": round(t / statistics.median(ms[Kmax]), 5)}
    return res


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
    ap.add_argument("--land", type=float, default=None, metavar="FRACTION",
                    help="paint a coast with about this share of dry pixels and compare land=True with land=False")
    ap.add_argument("--spectra", type=int, nargs="?", const=256, default=None, metavar="WINDOW",
                    help="time score_spectra's spectral stage at this window (default 256) beside score")
    ap.add_argument("--ssim", action="store_true", help="time score_ssim's SSIM stage beside score")
    ap.add_argument("--gradient", action="store_true", help="time score_gradient's stage beside score")
    ap.add_argument("--fss", action="store_true", help="time score_fss, its stage and each of its launches beside score")
    ap.add_argument("--ensemble-score", action="store_true",
                    help="time members=True, score_ensemble, the member launches and the score's launches at K = 4, 8")
    ap.add_argument("--hbm-tbs", type=float, default=6.3, help="achievable HBM rate the memory floor is taken at")
    ap.add_argument("--distribution", action="store_true",
                    help="time score_distribution's stage beside score and the SSIM stage, on a smooth and a white input")
    ap.add_argument("--ensemble", type=int, nargs="+", default=None, metavar="K", choices=(1, 4, 8),
                    help="time RegionSuperResolver(ensemble=K) for each K (1 is always among them)")
    ap.add_argument("--consistent", type=int, nargs="+", default=None, metavar="K", choices=range(17),
                    help="time RegionSuperResolver(consistent=K) for each K (0 is always among them)")
    ap.add_argument("--quantile-map", action="store_true",
                    help="time the quantile map's launches and the region with the map on and off, and score both")
    ap.add_argument("--out", default=None, help="default: profiles/superres_bench.json (superres_land_bench.json, "
                                                "spectra_bench.json, ssim_bench.json, gradient_bench.json, "
                                                "fss_bench.json, ensemble_score_bench.json, "
                                                "distribution_bench.json, "
                                                "ensemble_bench.json, consistency_bench.json, "
                                                "quantile_map_bench.json)")
    a = ap.parse_args()
    if (sum(x is not None for x in (a.land, a.spectra, a.ensemble, a.consistent)) + a.ssim + a.distribution
            + a.quantile_map + a.gradient + a.fss + a.ensemble_score > 1):
        raise SystemExit("superres_bench: --land, --spectra, --ssim, --gradient, --fss, --ensemble-score, --distribution, "
                         "--ensemble, --consistent and --quantile-map are separate runs")
    if a.land is not None and not 0.0 < a.land < 1.0:
        raise SystemExit("superres_bench: --land takes a fraction in (0, 1)")
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "superres_land_bench.json" if a.land is not None else
                             "spectra_bench.json" if a.spectra is not None else
                             "ssim_bench.json" if a.ssim else
                             "gradient_bench.json" if a.gradient else
                             "fss_bench.json" if a.fss else
                             "ensemble_score_bench.json" if a.ensemble_score else
                             "distribution_bench.json" if a.distribution else
                             "ensemble_bench.json" if a.ensemble is not None else
                             "consistency_bench.json" if a.consistent is not None else
                             "quantile_map_bench.json" if a.quantile_map else "superres_bench.json")
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
    if (a.land is not None or a.spectra is not None or a.ssim or a.distribution or a.ensemble is not None
            or a.consistent is not None or a.quantile_map or a.gradient or a.fss or a.ensemble_score):
        line = json.dumps(land_main(a, spec, params, lr, dev, kw) if a.land is not None else
                          spectra_main(a, spec, params, dev, kw) if a.spectra is not None else
                          ssim_main(a, spec, params, dev, kw) if a.ssim else
                          gradient_main(a, spec, params, dev, kw) if a.gradient else
                          fss_main(a, spec, params, dev, kw) if a.fss else
                          ensemble_score_main(a, spec, params, lr, dev, kw) if a.ensemble_score else
                          distribution_main(a, spec, params, dev, kw) if a.distribution else
                          ensemble_main(a, spec, params, lr, dev, kw) if a.ensemble is not None else
                          quantile_map_main(a, spec, params, dev, kw) if a.quantile_map else
                          consistency_main(a, spec, params, lr, dev, kw))
        print(line)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
        return
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
