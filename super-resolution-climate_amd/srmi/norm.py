"""The six ``task.norm`` modes and the dataset tile statistics, on the device.

Reference: ``SWOTRawDataLoader.norm`` (sres/base/source/swot/raw.py:169-214)
normalises every selected tile batch by ``task.norm``:

* ``lnorm`` / ``lscale``: (x - mean) / std and (x - min) / (max - min) of the
  tile itself (:177-186);
* ``gnorm`` / ``gscale``: the same with ONE statistic per variable over the whole
  dataset, ``global_norm_stats`` = ``globalize_norm`` of the tile statistics
  (:187-195, :23-30);
* ``tnorm`` / ``tscale``: one statistic per tile position over all time slices,
  ``norm_stats`` (:196-209).

The tile statistics come from ``_compute_normalization`` (:89-106): for every
time slice, every tile and every variable, ``NormData.add_entry`` (:55-60) takes
the plane's mean, variance, max and min -- a Python double loop.  Here that is
one HIP launch per time slice (``srmi_tile_stats``, tiles.hip) over the tensor
``srmi.llc.get_tiles`` returns, and ``srmi_tile_stats_finalize`` forms
``get_norm_stats`` (:62-63) and ``globalize_norm``.  ``_write_norm_stats`` /
``_read_norm_stats`` (:78-87) keep them in a netCDF file; ``NormStats.save`` /
``load`` write the same variables (one per varname, dims ('tiles', 'stat'), stat
order STATS) with scipy's netCDF-3 writer, as srmi.results does -- byte-layout
parity with xarray's NETCDF4 file is not claimed (no xarray here).

One divergence, by design: the reference's ``tscale`` branch (:204-209) subtracts
the UN-sliced ``[ntiles]`` statistics from the batch through xarray's label
alignment, whose labels are original grid indices on the batch and compacted
positions on the statistics.  That cannot be reproduced (or pinned) without
xarray; ``tscale`` here takes the rows ``tile_range`` positionally, exactly as
``tnorm`` does (:198).  The two coincide whenever no tile was dropped.
"""
from __future__ import annotations

from typing import Callable, Dict, Iterable, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from ._lib import SRMI_NORM_AFFINE, SRMI_NORM_LNORM, SRMI_NORM_LSCALE, call, ptr, stream_handle

NORM_TYPES = ("lnorm", "lscale", "gnorm", "gscale", "tnorm", "tscale")
STATS = ("mean", "var", "max", "min")  # raw.py:18
DATASET_NORMS = ("gnorm", "gscale", "tnorm", "tscale")  # need NormStats
MODES = {"lnorm": SRMI_NORM_LNORM, "lscale": SRMI_NORM_LSCALE, "gnorm": SRMI_NORM_AFFINE,
         "gscale": SRMI_NORM_AFFINE, "tnorm": SRMI_NORM_AFFINE, "tscale": SRMI_NORM_AFFINE}
# the statistics norm() leaves in attrs (raw.py:179-180, :184-185, :201-202, :208-209;
# the global branches :187-195 set none), which decide denorm's branch (dual_trainer.py:71-75)
ATTR_KEYS = {"lnorm": ("mean", "std"), "tnorm": ("mean", "std"), "lscale": ("max", "min"),
             "tscale": ("max", "min"), "gnorm": (), "gscale": ()}
LNORM_MAX_BATCH = 65535  # srmi_batch_prep's grid.y


def check_norm(norm) -> str:
    if norm not in NORM_TYPES:
        raise Exception(f"Unknown norm: {norm}")  # raw.py:210
    return norm


def norm_type(task) -> str:
    """``cfg().task.norm`` (raw.py:171), 'lnorm' when the task does not set it."""
    norm = task.get("norm", "lnorm") if task is not None else "lnorm"
    return check_norm("lnorm" if norm is None else norm)


def _check_tiles(tiles: torch.Tensor, what: str) -> None:
    if tiles.dtype != torch.float32 or tiles.dim() != 4 or not tiles.is_contiguous():
        raise ValueError(f"{what}: tiles must be a contiguous fp32 [n, C, ty, tx] tensor")


class NormStats:
    """Per-tile and global statistics of a dataset (``norm_stats`` /
    ``global_norm_stats``, raw.py:115-123).

    ``accumulate(tiles)`` once per time slice, then ``finalize()``:
    ``.tiles`` [n, C, 4] and ``.globals`` [C, 4] fp32 in STATS order.  Tile row i is
    tile POSITION i of the compacted tensor, as ``NormData.itile`` is (raw.py:96-100),
    so every time slice must hold the same number of tiles."""

    def __init__(self):
        self.acc: Optional[torch.Tensor] = None  # [n, C, 4] fp64
        self.ntimes = 0
        self.tiles: Optional[torch.Tensor] = None
        self.globals: Optional[torch.Tensor] = None

    # ------------------------------------------------------------- computing
    def accumulate(self, tiles: torch.Tensor, stream=None) -> "NormStats":
        _check_tiles(tiles, "NormStats.accumulate")
        n, C, ty, tx = tiles.shape
        if self.acc is None:
            self.acc = torch.empty(n, C, 4, dtype=torch.float64, device=tiles.device)
        elif tuple(self.acc.shape[:2]) != (n, C):
            raise ValueError(f"time slice of {n} x {C} tile planes after slices of {tuple(self.acc.shape[:2])}")
        call("srmi_tile_stats", ptr(tiles), n, C, ty, tx, ptr(self.acc), int(self.ntimes == 0),
             stream_handle(stream))
        self.ntimes += 1
        self.tiles = self.globals = None
        return self

    def finalize(self, stream=None) -> "NormStats":
        if self.acc is None:
            raise ValueError("NormStats.finalize: no time slice accumulated")
        n, C, _ = self.acc.shape
        self.tiles = torch.empty(n, C, 4, dtype=torch.float32, device=self.acc.device)
        self.globals = torch.empty(C, 4, dtype=torch.float32, device=self.acc.device)
        call("srmi_tile_stats_finalize", ptr(self.acc), n, C, self.ntimes, ptr(self.tiles), ptr(self.globals),
             stream_handle(stream))
        return self

    @classmethod
    def compute(cls, timeslices: Iterable[Union[torch.Tensor, Callable[[], torch.Tensor]]]) -> "NormStats":
        """The ``_compute_normalization`` loop: every item is a time slice's raw tiles
        [n, C, ty, tx] on the device, or a callable returning them (the form
        ``harness.train_timeslices`` takes)."""
        st = cls()
        for ts in timeslices:
            st.accumulate(ts() if callable(ts) else ts)
        return st.finalize()

    # ------------------------------------------------------------------ file
    def _need(self) -> torch.Tensor:
        if self.tiles is None:
            raise ValueError("NormStats: finalize() or load() first")
        return self.tiles

    def save(self, path: str, varnames: Sequence[str]) -> str:
        """``_write_norm_stats`` (raw.py:78-80): one variable per varname, dims
        ('tiles', 'stat'), coordinates tiles = 0 .. n-1 and stat = STATS."""
        from scipy.io import netcdf_file
        t = self._need().detach().cpu().numpy()
        if t.shape[1] != len(varnames):
            raise ValueError(f"{t.shape[1]} channels for {len(varnames)} variables")
        with netcdf_file(path, "w", version=2) as f:
            f.createDimension("tiles", t.shape[0])
            f.createDimension("stat", len(STATS))
            f.createDimension("string4", 4)
            tv = f.createVariable("tiles", np.int32, ("tiles",))
            tv[:] = np.arange(t.shape[0], dtype=np.int32)
            sv = f.createVariable("stat", "c", ("stat", "string4"))
            sv[:] = np.array([list(s.ljust(4, "\0")) for s in STATS], dtype="S1")
            for iv, v in enumerate(varnames):
                dv = f.createVariable(str(v), np.float32, ("tiles", "stat"))
                dv._FillValue = np.array([np.nan], dtype=np.float32)
                dv[:] = np.ascontiguousarray(t[:, iv])
        return path

    @classmethod
    def load(cls, path: str, varnames: Optional[Sequence[str]] = None,
             device: Optional[torch.device] = None) -> "NormStats":
        """``_read_norm_stats`` (raw.py:82-87).  varnames: the channel order (default:
        the file's).  ``.globals`` is ``globalize_norm`` of the stored fp32 rows, as
        ``global_norm_stats`` derives it from the file (raw.py:121-123)."""
        from scipy.io import netcdf_file
        with netcdf_file(path, "r", mmap=False) as f:
            names = [n for n, v in f.variables.items() if tuple(v.dimensions) == ("tiles", "stat") and n != "stat"]
            order = [b"".join(r.tolist()).decode().rstrip("\0") for r in f.variables["stat"][:]]
            if tuple(order) != STATS:
                raise ValueError(f"{path}: stat order {order} != {list(STATS)}")
            t = np.stack([np.array(f.variables[str(v)][:], dtype=np.float32) for v in (varnames or names)], axis=1)
        st = cls()
        st.tiles = torch.from_numpy(np.ascontiguousarray(t))
        if device is not None:
            st.tiles = st.tiles.to(device)
        st.globals = _globalize(st.tiles)
        return st

    # ------------------------------------------------------------------- use
    def for_grid(self, inv) -> "NormStats":
        """The statistics per GRID CELL (what TiledInference takes): inv[cell] = the
        kept-tile row of that cell or -1 (a cell whose tile get_tiles dropped gets NaN
        rows; tiled inference drops that tile too)."""
        t = self._need()
        inv = torch.as_tensor(np.asarray(inv.cpu() if hasattr(inv, "cpu") else inv), dtype=torch.long, device=t.device)
        out = NormStats()
        out.tiles = torch.full((inv.numel(),) + tuple(t.shape[1:]), float("nan"), dtype=t.dtype, device=t.device)
        keep = inv >= 0
        out.tiles[keep] = t[inv[keep]]
        out.globals = self.globals
        return out

    def offsets(self, norm: str, tile_range: Optional[Tuple[int, int]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(off [B, C], div [B, C]) of srmi's AFFINE mode for a dataset norm, B =
        the tiles of tile_range (default: all).  gnorm: mean, sqrt(mean var)
        (raw.py:189); gscale: min, max - min (:194-195); tnorm: rows tile_range of
        mean, sqrt(var) (:198); tscale: rows tile_range of min, max - min (positional;
        see the module docstring)."""
        if check_norm(norm) not in DATASET_NORMS:
            raise ValueError(f"{norm} takes its statistics from the tile, not from NormStats")
        t = self._need()
        a, b = tile_range if tile_range is not None else (0, t.shape[0])
        rows = t[a:b] if norm[0] == "t" else self.globals[None].expand(b - a, -1, -1)
        if norm.endswith("norm"):
            off, div = rows[..., 0], torch.sqrt(rows[..., 1])
        else:
            off, div = rows[..., 3], rows[..., 2] - rows[..., 3]
        return off.contiguous(), div.contiguous()

    def attrs(self, norm: str, tile_range: Optional[Tuple[int, int]] = None) -> Dict[str, torch.Tensor]:
        """The [B, C, 1, 1] statistics norm() records for a dataset norm (ATTR_KEYS)."""
        t = self._need()
        a, b = tile_range if tile_range is not None else (0, t.shape[0])
        rows = t[a:b]
        if norm == "tnorm":
            return {"mean": rows[..., 0, None, None].contiguous(),
                    "std": torch.sqrt(rows[..., 1])[..., None, None].contiguous()}
        if norm == "tscale":
            return {"max": rows[..., 2, None, None].contiguous(), "min": rows[..., 3, None, None].contiguous()}
        return {}


def _globalize(t: torch.Tensor) -> torch.Tensor:
    """globalize_norm (raw.py:23-30) of stored rows [n, C, 4] (file load only; the
    device path is srmi_tile_stats_finalize)."""
    d = t.double()
    g = torch.stack([d[..., 0].mean(0), d[..., 1].mean(0), d[..., 2].amax(0), d[..., 3].amin(0)], dim=-1)
    return g.float().contiguous()


def prep_norm(raw: torch.Tensor, norm: str, flip_index: int, scale: int, hr: torch.Tensor,
              lr: Optional[torch.Tensor], stats: Optional[NormStats], tile_range: Optional[Tuple[int, int]],
              stream=None, attrs: bool = True) -> Dict[str, torch.Tensor]:
    """One srmi_batch_prep_norm launch; returns norm()'s attrs (ATTR_KEYS) as
    [B, C, 1, 1] tensors ({} with attrs False).  Callers have validated norm /
    stats / shapes."""
    B, C, T, _ = raw.shape
    st = stream_handle(stream)
    f32 = dict(dtype=torch.float32, device=raw.device)
    if norm in DATASET_NORMS:
        tr = tile_range if tile_range is not None else (0, B)
        # the kernel reads off / div: statistics loaded from a file without device= are on
        # the host and are copied to the batch's device here (a no-op when they are there)
        off, div = (v.to(raw.device) for v in stats.offsets(norm, tr))
        if tuple(off.shape) != (B, C):
            raise ValueError(f"{norm}: statistics rows {tuple(off.shape)} for a batch of {B} x {C} (tile_range {tr})")
        call("srmi_batch_prep_norm", ptr(raw), B, C, T, int(flip_index), int(scale), MODES[norm], ptr(off), ptr(div),
             ptr(hr), ptr(lr), None, None, st)
        return {k: v.to(raw.device) for k, v in stats.attrs(norm, tr).items()} if attrs else {}
    a, b = (torch.empty(B, C, 1, 1, **f32), torch.empty(B, C, 1, 1, **f32)) if attrs else (None, None)
    call("srmi_batch_prep_norm", ptr(raw), B, C, T, int(flip_index), int(scale), MODES[norm], None, None, ptr(hr),
         ptr(lr), ptr(a), ptr(b), st)
    if not attrs:
        return {}
    if norm == "lnorm":
        return {"mean": a, "std": b}
    # lscale: the kernel reports min and the fp32 max - min; attrs['max'] (raw.py:184) is
    # the exact maximum, which min + (max - min) in fp32 need not give back
    acc = torch.empty(B, C, 4, dtype=torch.float64, device=raw.device)
    call("srmi_tile_stats", ptr(raw), B, C, T, T, ptr(acc), 1, st)
    return {"max": acc[..., 2, None, None].float(), "min": a}


def normalize_tiles(raw_tiles: torch.Tensor, norm: str = "lnorm", stats: Optional[NormStats] = None,
                    stream=None) -> torch.Tensor:
    """A whole time slice of raw tiles [n, C, T, T] -> the normalised tiles, no flip,
    no LR, tile_range (0, n): what ``harness.train_timeslices``' callables return.
    Every norm is per tile or global, so this equals normalising batch by batch."""
    check_norm(norm)
    if norm in DATASET_NORMS and stats is None:
        raise ValueError(f"norm {norm!r} needs the dataset statistics (stats=NormStats)")
    _check_tiles(raw_tiles, "normalize_tiles")
    if raw_tiles.shape[2] != raw_tiles.shape[3]:
        raise ValueError("normalize_tiles: tiles must be square (srmi_batch_prep_norm's layout)")
    n = raw_tiles.shape[0]
    hr = torch.empty_like(raw_tiles)
    if norm == "lnorm":  # srmi_batch_prep's launch holds 65535 tiles
        for a in range(0, n, LNORM_MAX_BATCH):
            b = min(n, a + LNORM_MAX_BATCH)
            prep_norm(raw_tiles[a:b], norm, 0, 2, hr[a:b], None, None, None, stream, attrs=False)
    else:
        prep_norm(raw_tiles, norm, 0, 2, hr, None, stats, (0, n), stream, attrs=False)
    return hr
