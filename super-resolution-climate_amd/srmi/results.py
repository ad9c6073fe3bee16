"""Inference result files: drop-in for sres/data/inference.py.

Reference (sres/data/inference.py:10-50, called from WorkflowController.inference,
sres/controller/workflow.py:53-75):

* ``results_path``: ``{platform.results}/inference/{dataset}/{task}/{var}-{t}.{tiles|image}[_ds-{f:.2f}].nc``
  (``_ds-`` only when ``task.data_downsample`` != 1).
* ``save_inference_results``: one Dataset per variable and time step with the data
  variables ``input`` (dims renamed y -> ys, x -> xs), ``target``, ``interpolated``
  and ``model``, and the global attributes ``loss_keys`` / ``loss_values``.
* The arrays come in two structures:
  - Image (process_image -> assemble_images, dual_trainer.py:449-480): ``[y, x]``
    mosaics, coordinates ``arange(0, 100, 100 / n)`` on both axes;
  - Tiles (evaluate -> to_xa, dual_trainer.py:148-155): ``[tiles, channels, y, x]``
    float32 with integer coordinates, then ``squeeze()`` for one variable (the
    ``channels`` coordinate stays as a scalar) or ``sel(channels=v, drop=True)``
    for several (workflow.py:61-67).

xarray and netCDF4 are not installed here, so the file is written with
``scipy.io.netcdf_file`` -- the engine xarray itself falls back to without
netCDF4 -- as NETCDF3_64BIT: int64 coordinates are stored as int32 (xarray's
netCDF-3 coercion), float variables carry ``_FillValue = NaN`` (xarray's
default encoding), a scalar string coordinate is a char variable over a
``string{N}`` dimension.  netCDF-3 has no string-array attributes, so
``loss_keys`` is stored as ONE char attribute, the keys joined by ``,``;
``load_inference_results`` splits it back (the reference's loader zips the
attribute as a list and would need that split).  Parity of the byte layout
against xarray's own writer is unpinned (no xarray here); the round trip through
scipy is tested.
"""
from __future__ import annotations

import glob
import os
from dataclasses import dataclass, field
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .gradient_names import GRADIENT_STATS

STRUCTURES = ("tiles", "image")  # ResultStructure values (sres/controller/config.py:3-5)


@dataclass
class Var:
    """A labelled array (the subset of xarray.DataArray the result files need)."""
    dims: Tuple[str, ...]
    values: np.ndarray
    coords: Dict[str, np.ndarray] = field(default_factory=dict)  # dimension coordinates
    scalar_coords: Dict[str, object] = field(default_factory=dict)  # e.g. channels='SST'


def results_path(results_root: str, dataset: str, task: str, varname: str, timestep, structure: str,
                 data_downsample: float = 1.0, remove: bool = False) -> str:
    """results_path (inference.py:10-18)."""
    if structure not in STRUCTURES:
        raise ValueError(f"unknown result structure {structure!r}")
    f = float(data_downsample)
    dss = "" if f == 1.0 else f"_ds-{f:.2f}"
    p = f"{results_root}/inference/{dataset}/{task}/{varname}-{timestep}.{structure}{dss}.nc"
    os.makedirs(os.path.dirname(p), exist_ok=True)
    if remove and os.path.exists(p):
        os.remove(p)
    return p


def time_indices(results_root: str, dataset: str, task: str, varname: str, structure: str,
                 data_downsample: float = 1.0) -> List[int]:
    """time_indices (inference.py:20-22): the time steps that have a result file."""
    pat = results_path(results_root, dataset, task, varname, "*", structure, data_downsample)
    return [int(Path(fn).stem.split(".")[0].split("-")[1]) for fn in glob.glob(pat)]


def _np(x) -> np.ndarray:
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x)


def image_results(images: Dict[str, object], varnames: Sequence[str]) -> Dict[str, Dict[str, Var]]:
    """Per-variable Image results from srmi.inference.TiledInference.process_region
    images ([C, H, W] per type): assemble_images' [y, x] arrays with coordinates
    arange(0, 100, 100 / n) (dual_trainer.py:475-478)."""
    out: Dict[str, Dict[str, Var]] = {}
    for iv, v in enumerate(varnames):
        d = {}
        for k, img in images.items():
            a = _np(img)[iv].astype(np.float64)  # np.block of float64 NaN-filled cells
            co = {cn: np.arange(0.0, 100.0, 100.0 / a.shape[ic]) for ic, cn in enumerate(("y", "x"))}
            d[k] = Var(("y", "x"), a, co)
        out[v] = d
    return out


def tiles_results(results: Dict[str, object], varnames: Sequence[str]) -> Dict[str, Dict[str, Var]]:
    """Per-variable Tiles results from TiledInference.evaluate's [n, C, h, w] arrays:
    to_xa (dual_trainer.py:148-155, float32, coords tiles / channels / y / x),
    then squeeze() for one variable or sel(channels=v, drop=True) (workflow.py:61-67)."""
    out: Dict[str, Dict[str, Var]] = {v: {} for v in varnames}
    for k, arr in results.items():
        a = _np(arr).astype(np.float32)
        n, C, h, w = a.shape
        if C != len(varnames):
            raise ValueError(f"{k}: {C} channels for {len(varnames)} variables")
        coords = {"tiles": np.arange(n), "y": np.arange(h), "x": np.arange(w)}
        for iv, v in enumerate(varnames):
            if len(varnames) == 1:  # squeeze(): every size-1 dim becomes a scalar coordinate
                dims = [d for d, s in zip(("tiles", "channels", "y", "x"), a.shape) if s != 1]
                sc = {"channels": v}
                if n == 1:
                    sc["tiles"] = 0
                co = {d: coords[d] for d in dims}
                out[v][k] = Var(tuple(dims), a.reshape([s for s in a.shape if s != 1]), co, sc)
            else:
                out[v][k] = Var(("tiles", "y", "x"), a[:, iv], dict(coords))
    return out


def _nc3(a: np.ndarray) -> np.ndarray:
    """xarray's netCDF-3 dtype coercion (int64 -> int32, bool -> int8)."""
    if a.dtype == np.int64 or a.dtype == np.uint64:
        return a.astype(np.int32)
    if a.dtype == np.bool_:
        return a.astype(np.int8)
    return a


def save_inference_results(path: str, var_results: Dict[str, Var], losses: Dict[str, float]) -> str:
    """save_inference_results (inference.py:24-31) for ONE variable: ``input``'s
    y / x renamed ys / xs, Dataset(data_vars, attrs(loss_keys, loss_values))."""
    from scipy.io import netcdf_file
    vr = dict(var_results)
    if "input" in vr:
        iv = vr["input"]
        ren = {"y": "ys", "x": "xs"}
        vr["input"] = Var(tuple(ren.get(d, d) for d in iv.dims), iv.values,
                          {ren.get(d, d): c for d, c in iv.coords.items()}, dict(iv.scalar_coords))
    dims: Dict[str, int] = {}
    coords: Dict[str, np.ndarray] = {}
    scalars: Dict[str, object] = {}
    for name, v in vr.items():
        if v.values.ndim != len(v.dims):
            raise ValueError(f"{name}: {v.values.ndim}-d values for dims {v.dims}")
        for d, s in zip(v.dims, v.values.shape):
            if dims.setdefault(d, s) != s:
                raise ValueError(f"dimension {d}: size {s} != {dims[d]}")
        coords.update(v.coords)
        scalars.update(v.scalar_coords)
    if os.path.exists(path):
        os.remove(path)
    with netcdf_file(path, "w", version=2) as f:
        f.loss_keys = ",".join(str(k) for k in losses.keys())
        f.loss_values = np.asarray([float(x) for x in losses.values()], dtype=np.float64)
        for d, s in dims.items():
            f.createDimension(d, s)
        for d, c in coords.items():  # dimension coordinates
            c = _nc3(np.asarray(c))
            cv = f.createVariable(d, c.dtype, (d,))
            cv[:] = c
            if c.dtype.kind == "f":
                cv._FillValue = np.array([np.nan], dtype=c.dtype)
        for sname, sval in scalars.items():  # scalar coordinates
            if isinstance(sval, str):
                b = np.frombuffer(sval.encode("utf-8"), dtype="S1")
                sd = f"string{len(b)}"
                if sd not in dims:
                    f.createDimension(sd, len(b))
                    dims[sd] = len(b)
                sv = f.createVariable(sname, "c", (sd,))
                sv[:] = b
            else:
                a = _nc3(np.asarray(sval))
                sv = f.createVariable(sname, a.dtype, ())
                sv.assignValue(a)
        for name, v in vr.items():
            a = _nc3(np.ascontiguousarray(v.values))
            dv = f.createVariable(name, a.dtype, v.dims)
            if a.dtype.kind == "f":
                dv._FillValue = np.array([np.nan], dtype=a.dtype)
            if v.scalar_coords:
                dv.coordinates = " ".join(v.scalar_coords.keys())
            dv[:] = a
    return path


def save_superres_results(path_for_var, images: Dict[str, object], varnames: Sequence[str],
                          losses: Optional[Dict[str, float]] = None) -> List[str]:
    """The three images of srmi.superres.RegionSuperResolver.super_resolve ('input'
    [C, h, w], 'interpolated' and 'model' [C, s h, s w]) as one Image-structure file per
    variable: image_results' [y, x] arrays through save_inference_results (the same
    netCDF-3 writer and coercions; 'input' on ys / xs).  There is no 'target' -- a field
    with no HR has none -- and ``losses`` is empty unless RegionSuperResolver.score
    supplied some.  path_for_var: varname -> file path (e.g. a results_path partial).
    'spread' [C, s h, s w] (RegionSuperResolver(ensemble > 1)) is written as a fourth
    variable when ``images`` holds it; the file is unchanged otherwise.
    'residual' [C, h, w] (RegionSuperResolver(consistent > 0): the input minus the
    downsample of the uncorrected model) is written on the input's ys / xs when ``images``
    holds it; the file is unchanged otherwise.
    No reference counterpart (its files come from process_image only)."""
    missing = [k for k in ("input", "interpolated", "model") if k not in images]
    if missing:
        raise ValueError(f"super_resolve images lack {missing}")
    keys = ("input", "interpolated", "model") + (("spread",) if "spread" in images else ())
    per_var = image_results({k: images[k] for k in keys}, varnames)
    if "residual" in images:
        ren = {"y": "ys", "x": "xs"}
        for v, d in image_results({"residual": images["residual"]}, varnames).items():
            r = d["residual"]
            per_var[v]["residual"] = Var(tuple(ren[k] for k in r.dims), r.values,
                                         {ren[k]: c for k, c in r.coords.items()})
    return [save_inference_results(path_for_var(v), per_var[v], dict(losses or {})) for v in varnames]


def load_inference_results(path: str) -> Tuple[Dict[str, Var], Dict[str, float]]:
    """load_inference_results (inference.py:40-50): the data variables (``input``
    renamed back to y / x) and the losses dict."""
    from scipy.io import netcdf_file
    with netcdf_file(path, "r", mmap=False) as f:
        keys = f.loss_keys.decode() if isinstance(f.loss_keys, bytes) else str(f.loss_keys)
        vals = np.atleast_1d(f.loss_values).tolist()
        losses = dict(zip(keys.split(",") if keys else [], vals))
        names = [n for n in ("input", "target", "interpolated", "model", "spread", "residual") if n in f.variables]
        out: Dict[str, Var] = {}
        for n in names:
            v = f.variables[n]
            dims = tuple(v.dimensions)
            co = {d: np.array(f.variables[d][:]) for d in dims if d in f.variables}
            sc: Dict[str, object] = {}
            for s in getattr(v, "coordinates", b"").decode().split() if hasattr(v, "coordinates") else []:
                sv = f.variables[s]
                sc[s] = b"".join(sv[:].tolist()).decode() if sv.typecode() == "c" else sv.getValue()
            vals_ = np.array(v[:])
            if n == "input":
                ren = {"ys": "y", "xs": "x"}
                dims = tuple(ren.get(d, d) for d in dims)
                co = {ren.get(d, d): c for d, c in co.items()}
            out[n] = Var(dims, vals_, co, sc)
    return out, losses


SPECTRA_QUANTITIES = ("power_pred", "power_truth", "power_error", "cross", "error_ratio", "power_ratio", "coherence")


def save_spectra(path: str, spectra: Dict[str, object], window: int, varnames: Sequence[str]) -> str:
    """One spectral score (the dict of srmi.spectra.SpectralScore.measure, e.g. one entry
    of RegionSuperResolver.score_spectra's third result) as a netCDF-3 file, through the
    same scipy writer: one float32 variable per quantity on ('channel', 'shell'), the
    coordinate ``wavenumber`` on 'shell' (cycles per pixel), ``nused`` as one int32 (on 'one'),
    and the attributes ``window`` and ``varnames`` (the channel names joined by ``,``, as
    loss_keys is).  No reference counterpart."""
    from scipy.io import netcdf_file
    missing = [k for k in SPECTRA_QUANTITIES + ("wavenumber", "nused") if k not in spectra]
    if missing:
        raise ValueError(f"spectra lack {missing}")
    K = int(window) // 2 + 1
    wn = _np(spectra["wavenumber"]).astype(np.float32)
    if wn.shape != (K,):
        raise ValueError(f"wavenumber {wn.shape} for a window of {window}")
    if os.path.exists(path):
        os.remove(path)
    with netcdf_file(path, "w", version=2) as f:
        f.window = np.int32(window)
        f.varnames = ",".join(str(v) for v in varnames)
        f.createDimension("channel", len(varnames))
        f.createDimension("shell", K)
        wv = f.createVariable("wavenumber", np.float32, ("shell",))
        wv[:] = wn
        wv.units = "cycles per pixel"
        f.createDimension("one", 1)  # scipy's writer cannot assign a 0-d variable
        nv = f.createVariable("nused", np.int32, ("one",))
        nv[:] = _np(spectra["nused"]).reshape(-1)[:1].astype(np.int32)
        for q in SPECTRA_QUANTITIES:
            a = np.ascontiguousarray(_np(spectra[q]).astype(np.float32))
            if a.shape != (len(varnames), K):
                raise ValueError(f"{q}: {a.shape} is not {(len(varnames), K)}")
            dv = f.createVariable(q, np.float32, ("channel", "shell"))
            dv._FillValue = np.array([np.nan], dtype=np.float32)
            dv[:] = a
    return path


SSIM_SCALARS = ("ssim", "cs", "mse", "psnr", "data_range")
SSIM_COUNTS = ("nwin", "npix")


def save_ssim(path: str, ssim: Dict[str, object], varnames: Sequence[str]) -> str:
    """One SSIM score (the dict of srmi.ssim.SSIMScore.measure, e.g. one entry of
    RegionSuperResolver.score_ssim's third result) as a netCDF-3 file, through the same scipy
    writer: 'ssim', 'cs', 'mse', 'psnr', 'data_range' as float32 and 'nwin', 'npix' as float64
    (netCDF-3 has no int64; a double holds every count below 2^53 exactly) on ('channel',),
    'map' as float32 on ('channel', 'y', 'x') with ``_FillValue = NaN`` when the dict holds
    it, and the attribute ``varnames`` (the channel names joined by ``,``, as loss_keys is).
    No reference counterpart."""
    from scipy.io import netcdf_file
    missing = [k for k in SSIM_SCALARS + SSIM_COUNTS if k not in ssim]
    if missing:
        raise ValueError(f"ssim lacks {missing}")
    n = len(varnames)
    if os.path.exists(path):
        os.remove(path)
    with netcdf_file(path, "w", version=2) as f:
        f.varnames = ",".join(str(v) for v in varnames)
        f.createDimension("channel", n)
        for q in SSIM_SCALARS + SSIM_COUNTS:
            dt = np.float32 if q in SSIM_SCALARS else np.float64
            a = np.ascontiguousarray(_np(ssim[q]).astype(dt))
            if a.shape != (n,):
                raise ValueError(f"{q}: {a.shape} is not {(n,)}")
            dv = f.createVariable(q, dt, ("channel",))
            if q in SSIM_SCALARS:
                dv._FillValue = np.array([np.nan], dtype=np.float32)
            dv[:] = a
        if "map" in ssim:
            m = np.ascontiguousarray(_np(ssim["map"]).astype(np.float32))
            if m.ndim != 3 or m.shape[0] != n:
                raise ValueError(f"map: {m.shape} is not [{n}, H, W]")
            f.createDimension("y", m.shape[1])
            f.createDimension("x", m.shape[2])
            mv = f.createVariable("map", np.float32, ("channel", "y", "x"))
            mv._FillValue = np.array([np.nan], dtype=np.float32)
            mv[:] = m
    return path


def load_ssim(path: str) -> Tuple[Dict[str, np.ndarray], List[str]]:
    """The inverse of save_ssim: (the score as numpy arrays, the counts int64 again; varnames)."""
    from scipy.io import netcdf_file
    with netcdf_file(path, "r", mmap=False) as f:
        names = f.varnames.decode() if isinstance(f.varnames, bytes) else str(f.varnames)
        out = {q: np.array(f.variables[q][:], dtype=np.float32) for q in SSIM_SCALARS}
        out.update({q: np.array(f.variables[q][:]).astype(np.int64) for q in SSIM_COUNTS})
        if "map" in f.variables:
            out["map"] = np.array(f.variables["map"][:], dtype=np.float32)
        return out, names.split(",") if names else []


GRADIENT_SCALARS = GRADIENT_STATS  # srmi.gradient_names: the order of srmi_gradient's stats columns
GRADIENT_MAPS = ("gmag_pred", "gmag_truth")


def save_gradient(path: str, gradient: Dict[str, object], varnames: Sequence[str], spacing=(1.0, 1.0)) -> str:
    """One gradient score (the dict of srmi.gradient.GradientScore.measure, e.g. one entry of
    RegionSuperResolver.score_gradient's third result) as a netCDF-3 file, through the same
    scipy writer: 'mean_pred', 'mean_truth', 'sharpness', 'rmse_mag', 'rmse_vec', 'cosine' as
    float64 with ``_FillValue = NaN`` and 'count' as float64 (netCDF-3 has no int64; a double
    holds every count below 2^53 exactly) on ('channel',), 'sums' as float64 on ('channel',
    'sum') when the dict holds it, 'gmag_pred' / 'gmag_truth' as float32 on ('channel', 'y',
    'x') with ``_FillValue = NaN`` when the dict holds them, and the attributes ``varnames``
    (the channel names joined by ``,``) and ``spacing`` (dy, dx).  A 'distribution' entry is
    not written: save_distribution takes it.  No reference counterpart."""
    from scipy.io import netcdf_file
    missing = [k for k in GRADIENT_SCALARS + ("count",) if k not in gradient]
    if missing:
        raise ValueError(f"gradient lacks {missing}")
    n = len(varnames)
    maps = [q for q in GRADIENT_MAPS if q in gradient]
    if os.path.exists(path):
        os.remove(path)
    with netcdf_file(path, "w", version=2) as f:
        f.varnames = ",".join(str(v) for v in varnames)
        f.spacing = np.array([float(v) for v in spacing], dtype=np.float64)
        f.createDimension("channel", n)
        for q in GRADIENT_SCALARS + ("count",):
            a = np.ascontiguousarray(_np(gradient[q]).astype(np.float64))
            if a.shape != (n,):
                raise ValueError(f"{q}: {a.shape} is not {(n,)}")
            dv = f.createVariable(q, np.float64, ("channel",))
            if q != "count":
                dv._FillValue = np.array([np.nan], dtype=np.float64)
            dv[:] = a
        if "sums" in gradient:
            a = np.ascontiguousarray(_np(gradient["sums"]).astype(np.float64))
            if a.ndim != 2 or a.shape[0] != n:
                raise ValueError(f"sums: {a.shape} is not [{n}, 7]")
            f.createDimension("sum", a.shape[1])
            dv = f.createVariable("sums", np.float64, ("channel", "sum"))
            dv._FillValue = np.array([np.nan], dtype=np.float64)
            dv[:] = a
        for i, q in enumerate(maps):
            m = np.ascontiguousarray(_np(gradient[q]).astype(np.float32))
            if m.ndim != 3 or m.shape[0] != n:
                raise ValueError(f"{q}: {m.shape} is not [{n}, H, W]")
            if i == 0:
                f.createDimension("y", m.shape[1])
                f.createDimension("x", m.shape[2])
            mv = f.createVariable(q, np.float32, ("channel", "y", "x"))
            mv._FillValue = np.array([np.nan], dtype=np.float32)
            mv[:] = m
    return path


def load_gradient(path: str) -> Tuple[Dict[str, np.ndarray], List[str], Tuple[float, float]]:
    """The inverse of save_gradient: (the score as numpy arrays, 'count' int64 again; varnames;
    spacing)."""
    from scipy.io import netcdf_file
    with netcdf_file(path, "r", mmap=False) as f:
        names = f.varnames.decode() if isinstance(f.varnames, bytes) else str(f.varnames)
        out = {q: np.array(f.variables[q][:], dtype=np.float64) for q in GRADIENT_SCALARS}
        out["count"] = np.array(f.variables["count"][:]).astype(np.int64)
        if "sums" in f.variables:
            out["sums"] = np.array(f.variables["sums"][:], dtype=np.float64)
        for q in GRADIENT_MAPS:
            if q in f.variables:
                out[q] = np.array(f.variables[q][:], dtype=np.float32)
        sp = np.atleast_1d(np.array(f.spacing, dtype=np.float64))
        return out, names.split(",") if names else [], (float(sp[0]), float(sp[1]))


FSS_TABLES = ("num", "den")
FSS_EVENTS = ("events_pred", "events_truth")
FSS_SCALARS = ("f_pred", "f_truth", "bias", "target", "afss", "skilful_scale")  # srmi.fss.FSS_DERIVED


def save_fss(path: str, fss: Dict[str, object], varnames: Sequence[str], thresholds, scales: Sequence[int]) -> str:
    """One fractions skill score (the dict of srmi.fss.FractionsSkillScore.measure, e.g. one
    entry of RegionSuperResolver.score_fss's third result) as a netCDF-3 file, through the same
    scipy writer.  The integer tables -- 'num', 'den' on ('channel', 'threshold', 'scale'),
    'events_pred', 'events_truth' on ('channel', 'threshold'), 'used' on ('channel',) -- are
    written as PAIRS of int32, '<name>_hi' and '<name>_lo' (value = hi 2^32 + lo as unsigned):
    netCDF-3 has no int64 and 'num' and 'den' pass 2^53, so a double would not hold them.
    'fss' is float64 on ('channel', 'threshold', 'scale'), 'f_pred', 'f_truth', 'bias',
    'target', 'afss', 'skilful_scale' float64 on ('channel', 'threshold'), all with
    ``_FillValue = NaN``; 'thresholds' float32 on ('channel', 'threshold'); the coordinate
    'scale' int32; the attribute ``varnames`` holds the channel names joined by ``,``.  No
    reference counterpart."""
    from scipy.io import netcdf_file
    keys = FSS_TABLES + FSS_EVENTS + FSS_SCALARS + ("used", "fss")
    missing = [k for k in keys if k not in fss]
    if missing:
        raise ValueError(f"fss lacks {missing}")
    n, sc = len(varnames), np.asarray([int(v) for v in scales], dtype=np.int32)
    thr = np.ascontiguousarray(_np(thresholds).astype(np.float32))
    if thr.ndim != 2 or thr.shape[0] != n:
        raise ValueError(f"thresholds: {thr.shape} is not [{n}, T]")
    T, N = thr.shape[1], len(sc)
    dims = {"used": ("channel",), "fss": ("channel", "threshold", "scale")}
    dims.update({q: ("channel", "threshold", "scale") for q in FSS_TABLES})
    dims.update({q: ("channel", "threshold") for q in FSS_EVENTS + FSS_SCALARS})
    sizes = {"channel": n, "threshold": T, "scale": N}
    arrays = {}
    for q in keys:
        a = _np(fss[q])
        a = np.ascontiguousarray(a.astype(np.float64 if q in FSS_SCALARS + ("fss",) else np.int64))
        shape = tuple(sizes[d] for d in dims[q])
        if a.shape != shape:
            raise ValueError(f"{q}: {a.shape} is not {shape}")
        arrays[q] = a
    if os.path.exists(path):
        os.remove(path)
    with netcdf_file(path, "w", version=2) as f:
        f.varnames = ",".join(str(v) for v in varnames)
        for d, size in sizes.items():
            f.createDimension(d, size)
        sv = f.createVariable("scale", np.int32, ("scale",))
        sv[:] = sc
        tv = f.createVariable("thresholds", np.float32, ("channel", "threshold"))
        tv._FillValue = np.array([np.nan], dtype=np.float32)
        tv[:] = thr
        for q in FSS_TABLES + FSS_EVENTS + ("used",):
            u = arrays[q].view(np.uint64)
            for part, half in (("hi", u >> np.uint64(32)), ("lo", u & np.uint64(0xFFFFFFFF))):
                dv = f.createVariable(f"{q}_{part}", np.int32, dims[q])
                dv[:] = half.astype(np.uint32).view(np.int32)
        for q in FSS_SCALARS + ("fss",):
            dv = f.createVariable(q, np.float64, dims[q])
            dv._FillValue = np.array([np.nan], dtype=np.float64)
            dv[:] = arrays[q]
    return path


def load_fss(path: str) -> Tuple[Dict[str, np.ndarray], List[str], np.ndarray, Tuple[int, ...]]:
    """The inverse of save_fss: (the score as numpy arrays, the tables int64 again; varnames;
    thresholds [C, T] fp32; scales)."""
    from scipy.io import netcdf_file
    with netcdf_file(path, "r", mmap=False) as f:
        names = f.varnames.decode() if isinstance(f.varnames, bytes) else str(f.varnames)
        out = {}
        for q in FSS_TABLES + FSS_EVENTS + ("used",):
            hi = np.array(f.variables[f"{q}_hi"][:], dtype=np.int32).view(np.uint32).astype(np.uint64)
            lo = np.array(f.variables[f"{q}_lo"][:], dtype=np.int32).view(np.uint32).astype(np.uint64)
            out[q] = ((hi << np.uint64(32)) | lo).view(np.int64)
        for q in FSS_SCALARS + ("fss",):
            out[q] = np.array(f.variables[q][:], dtype=np.float64)
        thr = np.array(f.variables["thresholds"][:], dtype=np.float32)
        sc = tuple(int(v) for v in np.array(f.variables["scale"][:]))
        return out, names.split(",") if names else [], thr, sc


ENSEMBLE_TABLES = ("used", "rank_hist", "tied", "bin_count")
ENSEMBLE_SCALARS = ("crps", "crps_fair", "rmse_mean", "spread_rms", "ssr", "spread_error_corr", "outliers",
                    "outliers_expected", "reliability_index")  # srmi.ensemble_score.ENS_DERIVED
ENSEMBLE_BINS = ("bin_spread", "bin_rmse")


def save_ensemble_score(path: str, score: Dict[str, object], varnames: Sequence[str]) -> str:
    """One ensemble score (the dict of srmi.ensemble_score.EnsembleScore.measure, e.g.
    RegionSuperResolver.score_ensemble's third result) as a netCDF-3 file, through the same scipy
    writer.  The integer tables -- 'used', 'tied' on ('channel',), 'rank_hist' on ('channel',
    'rank'), 'bin_count' on ('channel', 'bin') -- are written as PAIRS of int32, '<name>_hi' and
    '<name>_lo' (value = hi 2^32 + lo as unsigned), as save_fss writes its tables; 'sums' is
    float64 on ('channel', 'sum'), the derived values float64 on ('channel',) and 'bin_spread',
    'bin_rmse' on ('channel', 'bin'), all with ``_FillValue = NaN``; 'edges' float32 on
    ('channel', 'edge') (left out with one bin: netCDF-3 has no empty dimension); 'crps_map',
    when the score holds one, float32 on ('channel', 'y', 'x'); the attribute ``varnames`` holds
    the channel names joined by ``,``.  K is the length of 'rank' minus one.  No reference
    counterpart."""
    from scipy.io import netcdf_file
    keys = ENSEMBLE_TABLES + ENSEMBLE_SCALARS + ENSEMBLE_BINS + ("sums", "edges")
    missing = [k for k in keys if k not in score]
    if missing:
        raise ValueError(f"score lacks {missing}")
    n = len(varnames)
    hist = _np(score["rank_hist"])
    bins = _np(score["bin_count"])
    if hist.ndim != 2 or bins.ndim != 2:
        raise ValueError(f"rank_hist {hist.shape} and bin_count {bins.shape}: [C, K + 1] and [C, B] are needed")
    B = bins.shape[1]
    sizes = {"channel": n, "rank": hist.shape[1], "bin": B, "sum": 9 + 2 * B}
    if B > 1:
        sizes["edge"] = B - 1
    dims = {"used": ("channel",), "tied": ("channel",), "rank_hist": ("channel", "rank"),
            "bin_count": ("channel", "bin"), "sums": ("channel", "sum"), "edges": ("channel", "edge")}
    dims.update({q: ("channel",) for q in ENSEMBLE_SCALARS})
    dims.update({q: ("channel", "bin") for q in ENSEMBLE_BINS})
    arrays = {}
    for q in keys:
        a = _np(score[q])
        a = np.ascontiguousarray(a.astype(np.int64 if q in ENSEMBLE_TABLES else np.float32 if q == "edges"
                                          else np.float64))
        shape = tuple(sizes.get(d, 0) for d in dims[q])
        if a.shape != shape:
            raise ValueError(f"{q}: {a.shape} is not {shape}")
        arrays[q] = a
    cmap = None
    if score.get("crps_map") is not None:
        cmap = np.ascontiguousarray(_np(score["crps_map"]).astype(np.float32))
        if cmap.ndim != 3 or cmap.shape[0] != n:
            raise ValueError(f"crps_map: {cmap.shape} is not [{n}, H, W]")
        sizes["y"], sizes["x"] = cmap.shape[1], cmap.shape[2]
    if os.path.exists(path):
        os.remove(path)
    with netcdf_file(path, "w", version=2) as f:
        f.varnames = ",".join(str(v) for v in varnames)
        for d, size in sizes.items():
            f.createDimension(d, size)
        for q in ENSEMBLE_TABLES:
            u = arrays[q].view(np.uint64)
            for part, half in (("hi", u >> np.uint64(32)), ("lo", u & np.uint64(0xFFFFFFFF))):
                dv = f.createVariable(f"{q}_{part}", np.int32, dims[q])
                dv[:] = half.astype(np.uint32).view(np.int32)
        for q in ENSEMBLE_SCALARS + ENSEMBLE_BINS + ("sums",):
            dv = f.createVariable(q, np.float64, dims[q])
            dv._FillValue = np.array([np.nan], dtype=np.float64)
            dv[:] = arrays[q]
        if B > 1:
            ev = f.createVariable("edges", np.float32, dims["edges"])
            ev._FillValue = np.array([np.nan], dtype=np.float32)
            ev[:] = arrays["edges"]
        if cmap is not None:
            mv = f.createVariable("crps_map", np.float32, ("channel", "y", "x"))
            mv._FillValue = np.array([np.nan], dtype=np.float32)
            mv[:] = cmap
    return path


def load_ensemble_score(path: str) -> Tuple[Dict[str, np.ndarray], List[str]]:
    """The inverse of save_ensemble_score: (the score as numpy arrays, the tables int64 again,
    'edges' [C, B - 1] fp32, 'crps_map' when the file holds one; varnames)."""
    from scipy.io import netcdf_file
    with netcdf_file(path, "r", mmap=False) as f:
        names = f.varnames.decode() if isinstance(f.varnames, bytes) else str(f.varnames)
        out = {}
        for q in ENSEMBLE_TABLES:
            hi = np.array(f.variables[f"{q}_hi"][:], dtype=np.int32).view(np.uint32).astype(np.uint64)
            lo = np.array(f.variables[f"{q}_lo"][:], dtype=np.int32).view(np.uint32).astype(np.uint64)
            out[q] = ((hi << np.uint64(32)) | lo).view(np.int64)
        for q in ENSEMBLE_SCALARS + ENSEMBLE_BINS + ("sums",):
            out[q] = np.array(f.variables[q][:], dtype=np.float64)
        if "edges" in f.variables:
            out["edges"] = np.array(f.variables["edges"][:], dtype=np.float32)
        else:
            out["edges"] = np.zeros((out["used"].shape[0], 0), dtype=np.float32)
        if "crps_map" in f.variables:
            out["crps_map"] = np.array(f.variables["crps_map"][:], dtype=np.float32)
        return out, names.split(",") if names else []


DISTRIBUTION_SCALARS = ("pss", "w1", "under", "over")
DISTRIBUTION_QUANTILES = ("q_pred", "q_truth", "q_bias")
DISTRIBUTION_TABLES = ("hist_pred", "hist_truth")


def save_distribution(path: str, dist: Dict[str, object], varnames: Sequence[str],
                      probs: Sequence[float]) -> str:
    """One distribution score (the dict of srmi.distribution.DistributionScore.measure, e.g.
    one entry of RegionSuperResolver.score_distribution's third result) as a netCDF-3 file,
    through the same scipy writer.  The counts -- 'hist_pred', 'hist_truth' on ('channel',
    'entry'), 'joint' on ('channel', 'jpred', 'jtruth') when it has bins, 'count' on
    ('channel',) -- are float64: netCDF-3 has no int64, and a double holds every count below
    2^53 exactly (a count is at most H W < 2^31).  'lo', 'hi' are float32; 'pss', 'w1',
    'under', 'over' float64 on ('channel',); 'q_pred', 'q_truth', 'q_bias' float64 on
    ('channel', 'prob') with the coordinate 'prob'; 'edges' float64 on ('channel', 'edge'),
    the B + 3 edges of the B + 2 entries (srmi.distribution.bin_edges).  The attribute
    ``varnames`` holds the channel names joined by ``,``, as loss_keys does.  No reference
    counterpart."""
    from scipy.io import netcdf_file

    from .distribution import bin_edges
    keys = DISTRIBUTION_SCALARS + DISTRIBUTION_QUANTILES + DISTRIBUTION_TABLES + ("joint", "lo", "hi", "count")
    missing = [k for k in keys if k not in dist]
    if missing:
        raise ValueError(f"dist lacks {missing}")
    n, pr = len(varnames), np.asarray(list(probs), dtype=np.float64)
    tables = {q: np.ascontiguousarray(_np(dist[q]).astype(np.int64)) for q in DISTRIBUTION_TABLES + ("joint", "count")}
    nb2 = tables["hist_pred"].shape[-1]
    J = tables["joint"].shape[-1]
    for q, shape in (("hist_pred", (n, nb2)), ("hist_truth", (n, nb2)), ("joint", (n, J, J)), ("count", (n,))):
        if tables[q].shape != shape:
            raise ValueError(f"{q}: {tables[q].shape} is not {shape}")
        if tables[q].size and int(tables[q].max()) >= 2 ** 53:
            raise ValueError(f"{q}: a count of 2^53 or more does not fit a double")
    if nb2 < 4:
        raise ValueError(f"hist_pred: {nb2} entries are fewer than 2 bins and the two outer entries")
    if os.path.exists(path):
        os.remove(path)
    with netcdf_file(path, "w", version=2) as f:
        f.varnames = ",".join(str(v) for v in varnames)
        f.bins = np.int32(nb2 - 2)
        f.createDimension("channel", n)
        f.createDimension("entry", nb2)
        f.createDimension("edge", nb2 + 1)
        if len(pr):
            f.createDimension("prob", len(pr))
            pv = f.createVariable("prob", np.float64, ("prob",))
            pv[:] = pr
        for q in DISTRIBUTION_TABLES:
            dv = f.createVariable(q, np.float64, ("channel", "entry"))
            dv[:] = tables[q].astype(np.float64)
        if J:
            f.createDimension("jpred", J)
            f.createDimension("jtruth", J)
            dv = f.createVariable("joint", np.float64, ("channel", "jpred", "jtruth"))
            dv[:] = tables["joint"].astype(np.float64)
        dv = f.createVariable("count", np.float64, ("channel",))
        dv[:] = tables["count"].astype(np.float64)
        lohi = {}
        for q in ("lo", "hi"):
            lohi[q] = np.ascontiguousarray(_np(dist[q]).astype(np.float32))
            if lohi[q].shape != (n,):
                raise ValueError(f"{q}: {lohi[q].shape} is not {(n,)}")
            dv = f.createVariable(q, np.float32, ("channel",))
            dv._FillValue = np.array([np.nan], dtype=np.float32)
            dv[:] = lohi[q]
        ev = f.createVariable("edges", np.float64, ("channel", "edge"))
        ev._FillValue = np.array([np.nan], dtype=np.float64)
        ev[:] = bin_edges(lohi["lo"], lohi["hi"], nb2 - 2)
        for q in DISTRIBUTION_SCALARS + (DISTRIBUTION_QUANTILES if len(pr) else ()):
            a = np.ascontiguousarray(_np(dist[q]).astype(np.float64))
            shape = (n,) if q in DISTRIBUTION_SCALARS else (n, len(pr))
            if a.shape != shape:
                raise ValueError(f"{q}: {a.shape} is not {shape}")
            dv = f.createVariable(q, np.float64, ("channel",) if q in DISTRIBUTION_SCALARS else ("channel", "prob"))
            dv._FillValue = np.array([np.nan], dtype=np.float64)
            dv[:] = a
    return path


def load_distribution(path: str) -> Tuple[Dict[str, np.ndarray], List[str], np.ndarray]:
    """The inverse of save_distribution: (the score as numpy arrays, the counts int64 again,
    with 'edges' beside them; varnames; probs)."""
    from scipy.io import netcdf_file
    with netcdf_file(path, "r", mmap=False) as f:
        names = f.varnames.decode() if isinstance(f.varnames, bytes) else str(f.varnames)
        n = f.dimensions["channel"]
        pr = np.array(f.variables["prob"][:], dtype=np.float64) if "prob" in f.variables else np.zeros(0)
        out = {q: np.array(f.variables[q][:]).astype(np.int64) for q in DISTRIBUTION_TABLES + ("count",)}
        out["joint"] = (np.array(f.variables["joint"][:]).astype(np.int64) if "joint" in f.variables
                        else np.zeros((n, 0, 0), dtype=np.int64))
        for q in ("lo", "hi"):
            out[q] = np.array(f.variables[q][:], dtype=np.float32)
        for q in DISTRIBUTION_SCALARS + ("edges",):
            out[q] = np.array(f.variables[q][:], dtype=np.float64)
        for q in DISTRIBUTION_QUANTILES:
            out[q] = np.array(f.variables[q][:], dtype=np.float64) if len(pr) else np.zeros((n, 0))
        return out, names.split(",") if names else [], pr


def save_quantile_map(path: str, qmap, varnames: Sequence[str]) -> str:
    """One quantile map (srmi.quantile_map.QuantileMap, or its ``state_dict()``) as a netCDF-3
    file, through the same scipy writer.  The integer tables -- 'hist_src', 'hist_truth' on
    ('channel', 'entry'), 'count' on ('channel',) -- are float64 as save_distribution's are
    (netCDF-3 has no int64; a double holds every count below 2^53 exactly, and a larger one
    is refused).  'lo', 'hi' float32 on ('channel',); 'edges' float64 on ('channel', 'edge'),
    the B + 3 positions of the knots (srmi.distribution.bin_edges); 'knots' float64 on
    ('channel', 'edge') when the map was fitted.  Attributes: ``varnames`` (the channel names
    joined by ``,``), ``bins``, ``on``, ``tail_count``.  The table itself is not stored:
    load_state_dict re-derives it from the integer tables.  No reference counterpart."""
    from scipy.io import netcdf_file

    from .distribution import bin_edges
    sd = qmap.state_dict() if hasattr(qmap, "state_dict") else qmap
    missing = [k for k in ("hist", "count", "range", "bins", "on", "tail_count") if k not in sd]
    if missing:
        raise ValueError(f"the quantile map's state lacks {missing}")
    n, B = len(varnames), int(sd["bins"])
    hist = np.ascontiguousarray(_np(sd["hist"]).astype(np.int64))
    count = np.ascontiguousarray(_np(sd["count"]).astype(np.int64))
    rng = np.ascontiguousarray(_np(sd["range"]).astype(np.float32))
    for q, a, shape in (("hist", hist, (n, 2, B + 2)), ("count", count, (n,)), ("range", rng, (n, 2))):
        if a.shape != shape:
            raise ValueError(f"{q}: {a.shape} is not {shape}")
    if hist.size and int(hist.max()) >= 2 ** 53 or int(count.max()) >= 2 ** 53:
        raise ValueError("a count of 2^53 or more does not fit a double")
    if sd["on"] not in ("detail", "value"):
        raise ValueError(f"on {sd['on']!r}")
    knots = None
    if sd.get("knots") is not None:
        knots = np.ascontiguousarray(_np(sd["knots"]).astype(np.float64))
        if knots.shape != (n, B + 3):
            raise ValueError(f"knots: {knots.shape} is not {(n, B + 3)}")
    if os.path.exists(path):
        os.remove(path)
    with netcdf_file(path, "w", version=2) as f:
        f.varnames = ",".join(str(v) for v in varnames)
        f.bins = np.int32(B)
        f.on = str(sd["on"])
        f.tail_count = np.float64(int(sd["tail_count"]))
        f.createDimension("channel", n)
        f.createDimension("entry", B + 2)
        f.createDimension("edge", B + 3)
        for k, q in enumerate(("hist_src", "hist_truth")):
            dv = f.createVariable(q, np.float64, ("channel", "entry"))
            dv[:] = hist[:, k].astype(np.float64)
        dv = f.createVariable("count", np.float64, ("channel",))
        dv[:] = count.astype(np.float64)
        for k, q in enumerate(("lo", "hi")):
            dv = f.createVariable(q, np.float32, ("channel",))
            dv[:] = rng[:, k]
        ev = f.createVariable("edges", np.float64, ("channel", "edge"))
        ev[:] = bin_edges(rng[:, 0], rng[:, 1], B)
        if knots is not None:
            kv = f.createVariable("knots", np.float64, ("channel", "edge"))
            kv[:] = knots
    return path


def load_quantile_map(path: str) -> Tuple[Dict[str, object], List[str]]:
    """The inverse of save_quantile_map: (the state QuantileMap.load_state_dict takes, the
    counts int64 again, with 'edges' and, where stored, 'knots' beside them; varnames)."""
    from scipy.io import netcdf_file
    with netcdf_file(path, "r", mmap=False) as f:
        names = f.varnames.decode() if isinstance(f.varnames, bytes) else str(f.varnames)
        on = f.on.decode() if isinstance(f.on, bytes) else str(f.on)
        hist = np.stack([np.array(f.variables[q][:]).astype(np.int64) for q in ("hist_src", "hist_truth")], 1)
        sd = {"hist": hist, "count": np.array(f.variables["count"][:]).astype(np.int64),
              "range": np.stack([np.array(f.variables[q][:], dtype=np.float32) for q in ("lo", "hi")], 1),
              "bins": int(f.bins), "on": on, "tail_count": int(f.tail_count),
              "edges": np.array(f.variables["edges"][:], dtype=np.float64)}
        if "knots" in f.variables:
            sd["knots"] = np.array(f.variables["knots"][:], dtype=np.float64)
        return sd, names.split(",") if names else []


def load_spectra(path: str) -> Tuple[Dict[str, np.ndarray], int, List[str]]:
    """The inverse of save_spectra: (spectra as numpy arrays, window, varnames)."""
    from scipy.io import netcdf_file
    with netcdf_file(path, "r", mmap=False) as f:
        names = f.varnames.decode() if isinstance(f.varnames, bytes) else str(f.varnames)
        out = {q: np.array(f.variables[q][:], dtype=np.float32) for q in SPECTRA_QUANTITIES + ("wavenumber",)}
        out["nused"] = np.array(f.variables["nused"][:], dtype=np.int32).reshape(1)
        return out, int(f.window), names.split(",") if names else []
