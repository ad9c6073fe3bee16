"""Empirical quantile mapping of a super-resolved field: fit and apply on the device.

No reference counterpart -- a deliberate extension, not a parity item.  ``srmi.distribution``
reports ``q_bias``, the tail-compression number: a network trained on RMSE pulls its output
towards the mean and under-fills the tails.  ``QuantileMap`` is the correction downscaling
practice answers that with: a monotone transfer function ``T = F_truth^-1 o F_model``,
calibrated on fields whose truth is known and applied to every later output.

Definition (``srmi_quantile_map_*``, include/srmi.h; tests/quantile_map_oracle.py restates it)
----------------------------------------------------------------------------------------------
``accumulate`` adds the histograms of a model output and of its truth, on a FIXED range of B
bins per channel (the distribution score's own bin, so the tables of many fields add), to the
object's int64 tables.  ``fit`` turns the two tables into the B + 3 knots of ``T`` at the bin
edges: knot j is the truth's piecewise-linear quantile at the model's cumulative count before
entry j; where that count falls on a stretch of empty truth bins the point of the stretch
nearest to the knot's own edge is taken (equal tables give the identity, any tables a
non-decreasing ``T``); knots with fewer than ``tail_count`` samples beyond them are replaced
by the constant-shift extrapolation of the last trusted one.  ``apply`` interpolates ``T``
linearly in fp32 and adds ``strength * (T(v) - v)`` to the field.

A flat stretch of ``T`` means source bins that were empty at fit time: every value that later
falls into them maps to one value.  A wider calibration set or fewer bins removes it.

Detail or value
---------------
``on="value"`` maps the field's values.  ``on="detail"`` (the default) maps ``v = x - base``
with ``base`` the interpolated coarse field: the value distribution of a region is dominated
by its large-scale gradient, which the coarse input already gives; the compressed tails are
those of the detail, which is far closer to stationary from region to region and season to
season.  In both modes the correction is ADDED to x: ``base`` only locates ``v``.

Everything runs on the device without global atomics or a host read, so ``accumulate``,
``fit`` and ``apply`` can be captured in a HIP graph.  There is no CPU path: an object on the
CPU holds tables (``from_histograms``, ``load_state_dict``) and refuses to launch.

Out of scope: a map that varies in space or with the season, and training through the map.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from ._lib import SRMI_ERR_ARG, call, load, ptr, stream_handle

MODES = ("detail", "value")
MAX_BINS, MAX_CHANNELS = 4096, 16


def check_ranges(value_range, channels: int) -> np.ndarray:
    """one (lo, hi) pair or one pair per channel -> fp32 [C, 2]; ValueError unless every pair
    is finite in fp32 with hi > lo and an fp32 difference that is finite too."""
    try:
        with np.errstate(over="ignore"):
            r = np.asarray(value_range, dtype=np.float64).astype(np.float32)
    except (TypeError, ValueError):
        raise ValueError(f"value_range {value_range!r}: one (lo, hi) pair or one pair per channel") from None
    if r.shape == (2,):
        r = np.tile(r, (channels, 1))
    if r.shape != (channels, 2):
        raise ValueError(f"value_range {value_range!r}: one (lo, hi) pair or {channels} of them")
    with np.errstate(over="ignore", invalid="ignore"):
        ok = np.isfinite(r).all() and (r[:, 1] > r[:, 0]).all() and np.isfinite(r[:, 1] - r[:, 0]).all()
    if not ok:
        raise ValueError(f"value_range {value_range!r}: finite fp32 numbers with hi > lo and a finite hi - lo are "
                         f"needed")
    return np.ascontiguousarray(r)


def accumulate_workspace(C_: int, H: int, W: int, bins: int) -> int:
    """srmi_quantile_map_accumulate_workspace (host only): the bytes, or ValueError where it
    returns SRMI_ERR_ARG."""
    n = C.c_size_t()
    rc = load().srmi_quantile_map_accumulate_workspace(int(C_), int(H), int(W), int(bins), C.byref(n))
    if rc == SRMI_ERR_ARG:
        raise ValueError(f"the quantile map needs C in 1 .. {MAX_CHANNELS}, H, W >= 1 with H W < 2^31 and bins in 2 .. "
                         f"{MAX_BINS}, got {(C_, H, W)}, bins {bins}")
    if rc:
        raise RuntimeError(f"srmi_quantile_map_accumulate_workspace: {rc}")
    return int(n.value)


class QuantileMap:
    def __init__(self, channels: int, value_range, bins: int = 256, on: str = "detail", tail_count: int = 16,
                 device: Optional[torch.device] = None):
        """channels: C in 1 .. 16; value_range: one (lo, hi) pair or one per channel, of the
        VALUES (on="value") or of the DETAIL (on="detail"), finite with hi > lo; bins: B in
        2 .. 4096; tail_count: an integer >= 0, the samples a knot needs beyond it on both
        sides to be trusted.  Owns the tables; the workspace and the output of ``apply`` are
        allocated for a given (H, W) on first use, and ``apply`` allocates nothing
        afterwards.  Bad arguments raise ValueError before anything is allocated."""
        Cn, B = int(channels), int(bins)
        if Cn != channels or not 1 <= Cn <= MAX_CHANNELS:
            raise ValueError(f"channels {channels!r}: an integer in 1 .. {MAX_CHANNELS}")
        if B != bins or not 2 <= B <= MAX_BINS:
            raise ValueError(f"bins {bins!r}: an integer in 2 .. {MAX_BINS}")
        if on not in MODES:
            raise ValueError(f"on {on!r}: one of {MODES}")
        if isinstance(tail_count, float) and not tail_count.is_integer() or int(tail_count) < 0:
            raise ValueError(f"tail_count {tail_count!r}: an integer >= 0")
        self._set_range(check_ranges(value_range, Cn))
        self.C, self.bins, self.on, self.tail_count = Cn, B, on, int(tail_count)
        d = torch.device(device) if device is not None else torch.device("cuda")
        if d.type == "cuda" and d.index is None:
            d = torch.device("cuda", torch.cuda.current_device())
        self.device = d
        M = B + 2
        self.hist = torch.zeros((Cn, 2, M), dtype=torch.int64, device=d)
        self.count = torch.zeros(Cn, dtype=torch.int64, device=d)
        self.knots = torch.zeros((Cn, M + 1), dtype=torch.float64, device=d)
        self.table = torch.zeros((Cn, M + 1), dtype=torch.float32, device=d)
        self.meta = torch.zeros((Cn, 4), dtype=torch.float32, device=d)
        self.workspace: Optional[torch.Tensor] = None
        self.out: Optional[torch.Tensor] = None
        self._ws_shape: Optional[Tuple[int, int]] = None
        self._empty = True  # the next accumulate overwrites the tables
        self.fitted = False

    def _set_range(self, r: np.ndarray) -> None:
        self.range = r
        self._range = (C.c_float * r.size)(*r.reshape(-1).tolist())

    # --------------------------------------------------------------------- pieces
    def _need_device(self, what: str) -> None:
        if self.device.type != "cuda":
            raise RuntimeError(f"QuantileMap.{what} runs on the GPU alone (there is no CPU path); this object is on "
                               f"{self.device}")

    def _check(self, name: str, t: torch.Tensor, shape=None) -> Tuple[int, int]:
        if (t.dim() != 3 or t.shape[0] != self.C or t.dtype != torch.float32 or not t.is_contiguous()
                or t.device != self.device or (shape is not None and tuple(t.shape) != tuple(shape))):
            want = (self.C, "H", "W") if shape is None else tuple(shape)
            raise ValueError(f"{name}: a contiguous fp32 {want} tensor on {self.device} is needed, got "
                             f"{tuple(t.shape)} {t.dtype} on {t.device}")
        return int(t.shape[1]), int(t.shape[2])

    def _base(self, base, what: str, shape) -> Optional[torch.Tensor]:
        if (base is not None) != (self.on == "detail"):
            raise ValueError(f"{what}: base is needed with on='detail' and refused with on='value' (this map is "
                             f"on={self.on!r})")
        if base is not None:
            self._check("base", base, shape)
        return base

    # ------------------------------------------------------------------------ API
    def reset(self) -> None:
        """Forget what was accumulated: the next ``accumulate`` overwrites the tables.
        Nothing is launched; a fitted table stays until the next ``fit``."""
        self._empty = True

    def accumulate(self, src: torch.Tensor, truth: torch.Tensor, base: Optional[torch.Tensor] = None) -> None:
        """Add the histograms of src (the model's output) and truth, [C, H, W] fp32 on the
        device, to the tables: of src - base and truth - base with on="detail" (base is then
        required), of the values with on="value" (base is then refused).  A pixel is used
        iff both binned values are finite, so NaN is the land mask.  The first call, and the
        first after ``reset``, overwrites the tables; later calls add."""
        self._need_device("accumulate")
        H, W = self._check("src", src)
        self._check("truth", truth, src.shape)
        base = self._base(base, "accumulate", src.shape)
        if self._ws_shape != (H, W):
            nbytes = accumulate_workspace(self.C, H, W, self.bins)
            self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._ws_shape = (H, W)
        call("srmi_quantile_map_accumulate", ptr(src), ptr(truth), ptr(base), self.C, H, W, self.bins, self._range,
             int(self._empty), ptr(self.workspace), self.workspace.numel(), ptr(self.hist), ptr(self.count),
             stream_handle())
        self._empty = False

    def fit(self) -> None:
        """The tables -> 'knots' [C, B + 3] fp64, 'table' (their fp32 rounding) and 'meta'
        [C, 4] fp32 = {lo, hi, the shift below the table, the shift above it}: one launch,
        nothing is read on the host.  Tables that were never filled (or an all-NaN channel)
        give the identity."""
        self._need_device("fit")
        if self._empty:
            self.hist.zero_()
            self.count.zero_()
            self._empty = False
        call("srmi_quantile_map_fit", ptr(self.hist), ptr(self.count), self.C, self.bins, self._range,
             self.tail_count, ptr(self.knots), ptr(self.table), ptr(self.meta), stream_handle())
        self.fitted = True

    def apply(self, x: torch.Tensor, base: Optional[torch.Tensor] = None, strength: float = 1.0,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x [C, H, W] fp32 on the device -> x + strength * (T(v) - v) with v = x - base
        (on="detail", base required) or v = x (on="value", base refused).  out: x itself (in
        place), another tensor of x's shape that overlaps neither x nor base, or None for this
        object's own output buffer (valid until the next call).  A NaN of v is written back
        as x's bits, so land stays land; +-Inf stays what it is.  strength in [0, 1];
        strength == 0 launches nothing and returns x, copied if out is another tensor.  It
        needs ``fit`` (or ``load_state_dict``) first and raises RuntimeError otherwise."""
        self._need_device("apply")
        if not self.fitted:
            raise RuntimeError("QuantileMap.apply: no table yet -- call fit() or load_state_dict() first")
        s = float(strength)
        if not (math.isfinite(s) and 0.0 <= s <= 1.0):
            raise ValueError(f"strength {strength!r}: a number in [0, 1]")
        H, W = self._check("x", x)
        base = self._base(base, "apply", x.shape)
        if out is not None:
            self._check("out", out, x.shape)
        if s == 0.0:
            if out is None or out is x or out.data_ptr() == x.data_ptr():
                return x
            out.copy_(x)
            return out
        if out is None:
            if self.out is None or tuple(self.out.shape) != tuple(x.shape):
                self.out = torch.empty_like(x)
            out = self.out
        call("srmi_quantile_map_apply", ptr(x), ptr(base), self.C, H, W, self.bins, ptr(self.table), ptr(self.meta),
             s, ptr(out), stream_handle())
        return out

    # ---------------------------------------------------------------------- state
    @classmethod
    def from_histograms(cls, hist_src, hist_truth, value_range, tail_count: int = 16,
                        device: Optional[torch.device] = None) -> "QuantileMap":
        """A value-mode map from DistributionScore.measure's 'hist_pred' and 'hist_truth'
        [C, B + 2].  They must have been measured with a FIXED ``value_range``, passed here
        again: a score without one bins every field on its own truth's range, and such tables
        neither add nor say where their bins lie -- value_range=None is refused.  The map is
        fitted when the device is a GPU."""
        if value_range is None:
            raise ValueError("from_histograms needs the fixed value_range the histograms were measured with; a "
                             "DistributionScore without one is refused")
        hs, ht = (torch.as_tensor(h).detach().to("cpu", torch.int64) for h in (hist_src, hist_truth))
        if hs.dim() != 2 or hs.shape != ht.shape or hs.shape[1] < 4:
            raise ValueError(f"hist_src, hist_truth: [C, B + 2] are needed, got {tuple(hs.shape)}, {tuple(ht.shape)}")
        if bool((hs < 0).any()) or bool((ht < 0).any()) or not torch.equal(hs.sum(1), ht.sum(1)):
            raise ValueError("hist_src, hist_truth: counts >= 0 with the same sum per channel are needed")
        qm = cls(hs.shape[0], value_range, bins=hs.shape[1] - 2, on="value", tail_count=tail_count, device=device)
        qm.hist.copy_(torch.stack([hs, ht], 1))
        qm.count.copy_(hs.sum(1))
        qm._empty = False
        if qm.device.type == "cuda":
            qm.fit()
        return qm

    def state_dict(self) -> Dict[str, object]:
        """{'hist' [C, 2, B + 2] int64, 'count' [C] int64, 'range' [C, 2] fp32 (numpy arrays),
        'bins', 'on', 'tail_count'} and, once fitted, 'knots' [C, B + 3] fp64 for the record:
        the table is re-derived from the integer tables, never loaded.  A host read."""
        hist = self.hist.cpu().numpy() if not self._empty else np.zeros(tuple(self.hist.shape), dtype=np.int64)
        count = self.count.cpu().numpy() if not self._empty else np.zeros(self.C, dtype=np.int64)
        sd = {"hist": hist, "count": count, "range": self.range.copy(), "bins": self.bins, "on": self.on,
              "tail_count": self.tail_count}
        if self.fitted:
            sd["knots"] = self.knots.cpu().numpy()
        return sd

    def load_state_dict(self, sd: Dict[str, object]) -> None:
        """The inverse: bins and the channel count must be this object's; range, on and
        tail_count are taken from the state.  On a GPU the table is fitted at once.  A
        RegionSuperResolver that holds this object fixed whether it passes a base when it was
        built (and captured): load only a state of the same ``on`` into such an object."""
        hist = np.asarray(sd["hist"], dtype=np.int64)
        count = np.asarray(sd["count"], dtype=np.int64)
        if int(sd["bins"]) != self.bins or hist.shape != tuple(self.hist.shape) or count.shape != (self.C,):
            raise ValueError(f"state of {hist.shape[0] if hist.ndim else '?'} channels and {sd['bins']} bins does not "
                             f"fit a map of {self.C} channels and {self.bins} bins")
        if sd["on"] not in MODES or int(sd["tail_count"]) < 0:
            raise ValueError(f"state: on {sd['on']!r}, tail_count {sd['tail_count']!r}")
        if (hist < 0).any() or not np.array_equal(hist.sum(2)[:, 0], hist.sum(2)[:, 1]):
            raise ValueError("state: counts >= 0 with the same sum in both tables of a channel are needed")
        self._set_range(check_ranges(sd["range"], self.C))
        self.on, self.tail_count = str(sd["on"]), int(sd["tail_count"])
        self.hist.copy_(torch.from_numpy(hist))
        self.count.copy_(torch.from_numpy(count))
        self._empty = False
        self.fitted = False
        if self.device.type == "cuda":
            self.fit()


def knot_edges(value_range, bins: int) -> np.ndarray:
    """The B + 3 positions the knots belong to, fp64 [C, B + 3] for value_range [C, 2]:
    srmi.distribution.bin_edges of each channel's pair."""
    from .distribution import bin_edges
    r = np.asarray(value_range, dtype=np.float32).reshape(-1, 2)
    return bin_edges(r[:, 0], r[:, 1], bins)
