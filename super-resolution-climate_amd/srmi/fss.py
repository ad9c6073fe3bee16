"""Fractions skill score of a super-resolved field: is the feature there, and how near?

No reference counterpart -- a deliberate extension, not a parity item.  Every point-wise score
(``score``'s RMSE, ``srmi.distribution.contingency``) pays the double penalty: a sharp front
drawn three pixels off is one miss plus one false alarm and scores worse than no front at all.
The fractions skill score (FSS, Roberts & Lean 2008) compares, for a threshold, the FRACTION of
event pixels in an n x n neighbourhood of the prediction and of the truth, for a ladder of n,
and reports the skilful scale: the smallest neighbourhood at which the prediction is useful --
the displacement counterpart of ``srmi.spectra.effective_resolution``.

Definition (``srmi_fss``, include/srmi.h; tests/fss_oracle.py restates it in numpy)
----------------------------------------------------------------------------------
Per channel: a pixel is used iff it is finite in both fields; the event is ``used and value >=
threshold`` (one fp32 comparison); Sp, St are the event counts of the prediction and of the
truth in the n x n window around a position, clipped to the plane (what lies outside or is not
used is "no event" in both: scipy.ndimage.uniform_filter's mode="constant", pysteps'
convention); over ALL positions ``num = sum (Sp - St)^2``, ``den = sum (Sp^2 + St^2)`` in int64
and ``fss = 1 - num / den``.  ``target = 0.5 + f_truth / 2`` is the usual bar, ``skilful_scale``
the smallest n that reaches it, ``afss = 2 ep et / (ep^2 + et^2)`` what fss tends to when the
window covers the plane.  All sums are integers, so every table is exact and the same bits from
run to run; three launches without global atomics or a host read, so ``measure`` can be
captured in a HIP graph.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import SRMI_ERR_ARG, call, load, ptr, stream_handle

DEFAULT_SCALES = (1, 3, 5, 9, 17, 33, 65)
MAX_THRESHOLDS, MAX_SCALES, MAX_SCALE = 8, 16, 255
# the output positions a workgroup of the windows launch owns (kFssTileH x kFssTileW of
# csrc/fss.hip): the workspace grows by 16 bytes per (channel, threshold, scale) and such
# rectangle, which the tests check this against
FSS_TILE = (512, 64)
# srmi_fss's launches (SRMI_FSS_*): 0 runs all three; a subset times a launch by itself
EVENTS, WINDOWS, FINISH = 1, 2, 4
FSS_DERIVED = ("f_pred", "f_truth", "bias", "target", "afss", "skilful_scale")  # derived's columns behind fss[N]


def check_scales(scales) -> Tuple[int, ...]:
    """The neighbourhood sizes as srmi_fss takes them -- 1 .. 16 whole numbers, each odd, in 1 ..
    255, strictly increasing -- or ValueError."""
    try:
        raw = list(scales)
    except TypeError:
        raise ValueError(f"scales {scales!r}: a sequence of odd whole numbers") from None
    if not 1 <= len(raw) <= MAX_SCALES:
        raise ValueError(f"scales {scales!r}: 1 .. {MAX_SCALES} neighbourhood sizes")
    out = []
    for n in raw:
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)):
            raise ValueError(f"scales {scales!r}: whole numbers are needed")
        n = int(n)
        if n < 1 or n > MAX_SCALE or n % 2 == 0 or (out and n <= out[-1]):
            raise ValueError(f"scales {scales!r}: each odd, in 1 .. {MAX_SCALE}, strictly increasing (even "
                             "neighbourhoods are out of scope)")
        out.append(n)
    return tuple(out)


def fss_workspace(C_: int, H: int, W: int, T: int, N: int) -> int:
    """srmi_fss_workspace (host only): the bytes, or ValueError where it returns SRMI_ERR_ARG."""
    n = C.c_size_t()
    rc = load().srmi_fss_workspace(int(C_), int(H), int(W), int(T), int(N), C.byref(n))
    if rc == SRMI_ERR_ARG:
        raise ValueError(f"the fractions skill score needs C, H, W >= 1 with H W < 2^31, 1 .. {MAX_THRESHOLDS} "
                         f"thresholds and 1 .. {MAX_SCALES} scales, got {(C_, H, W)}, {T} thresholds, {N} scales")
    if rc:
        raise RuntimeError(f"srmi_fss_workspace: {rc}")
    return int(n.value)


class FractionsSkillScore:
    def __init__(self, shape: Tuple[int, int, int], thresholds, scales: Sequence[int] = DEFAULT_SCALES,
                 device: Optional[torch.device] = None):
        """shape: (C, H, W) of the fields; thresholds: a sequence of T floats (the same for every
        channel), a [C, T] array, or a [C, T] fp32 tensor on the device, which is kept by
        reference and read at every ``measure`` (fill it on the device, e.g. from a quantile,
        without a host read), T in 1 .. 8, NaN allowed (no event); scales: 1 .. 16 odd
        neighbourhood sizes in 1 .. 255, strictly increasing.  Owns the workspace and the
        outputs: ``measure`` allocates nothing.  Bad arguments raise ValueError before anything
        is allocated."""
        Cn, H, W = (int(v) for v in shape)
        sc = check_scales(scales)
        d = torch.device(device) if device is not None else torch.device("cuda")
        if d.type == "cuda" and d.index is None:
            d = torch.device("cuda", torch.cuda.current_device())
        host = None
        if isinstance(thresholds, torch.Tensor):
            if (thresholds.dim() != 2 or thresholds.shape[0] != Cn or not 1 <= thresholds.shape[1] <= MAX_THRESHOLDS
                    or thresholds.dtype != torch.float32 or not thresholds.is_contiguous() or thresholds.device != d):
                raise ValueError(f"thresholds: a contiguous fp32 [{Cn}, 1 .. {MAX_THRESHOLDS}] tensor on {d} is needed, "
                                 f"got {tuple(thresholds.shape)} {thresholds.dtype} on {thresholds.device}")
            T = int(thresholds.shape[1])
        else:
            try:
                host = np.asarray(thresholds, dtype=np.float32)
            except (TypeError, ValueError):
                raise ValueError(f"thresholds {thresholds!r}: numbers are needed") from None
            if host.ndim == 1:
                host = np.tile(host[None], (max(Cn, 1), 1))
            if host.ndim != 2 or host.shape[0] != Cn or not 1 <= host.shape[1] <= MAX_THRESHOLDS:
                raise ValueError(f"thresholds: T or [{Cn}, T] numbers with T in 1 .. {MAX_THRESHOLDS} are needed, got "
                                 f"shape {host.shape}")
            T = int(host.shape[1])
        N = len(sc)
        nbytes = fss_workspace(Cn, H, W, T, N)
        if H * W * sc[-1] ** 4 > 2 ** 62:
            raise ValueError(f"H W n_max^4 = {H * W * sc[-1] ** 4} is above 2^62: the sums would leave int64")
        self.C, self.H, self.W, self.T, self.N, self.scales, self.device = Cn, H, W, T, N, sc, d
        self._scales = (C.c_int * N)(*sc)
        self.thresholds = thresholds if host is None else torch.tensor(np.ascontiguousarray(host), device=d)
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=d)
        self.num = torch.zeros((Cn, T, N), dtype=torch.int64, device=d)
        self.den = torch.zeros((Cn, T, N), dtype=torch.int64, device=d)
        self.events = torch.zeros((Cn, T, 2), dtype=torch.int64, device=d)
        self.used = torch.zeros(Cn, dtype=torch.int64, device=d)
        self.derived = torch.empty((Cn, T, N + len(FSS_DERIVED)), dtype=torch.float64, device=d)

    def measure(self, pred: torch.Tensor, truth: torch.Tensor, launches: int = 0) -> Dict[str, torch.Tensor]:
        """pred, truth [C, H, W] fp32 on the device (NaN / Inf allowed: they are the mask) ->
        device tensors, views of this object's buffers, valid until the next call: 'num', 'den'
        [C, T, N] int64; 'events_pred', 'events_truth' [C, T] int64; 'used' [C] int64; 'fss' [C,
        T, N] fp64 (NaN where no window holds an event); 'f_pred', 'f_truth' (the event
        frequencies), 'bias' (their ratio), 'target' (0.5 + f_truth / 2), 'afss' and
        'skilful_scale' (the smallest n with fss >= target, NaN when there is none) [C, T]
        fp64.  A channel without a used pixel has NaN in every fp64 value and 0 in every
        table.  launches: 0, or EVENTS | WINDOWS | FINISH bits to run some of the three launches
        alone (a diagnostic for timing: the later ones read what an earlier call left in the
        workspace)."""
        shape = (self.C, self.H, self.W)
        for name, t in (("pred", pred), ("truth", truth)):
            if (tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous()
                    or t.device != self.device):
                raise ValueError(f"{name}: a contiguous fp32 {shape} tensor on {self.device} is needed, got "
                                 f"{tuple(t.shape)} {t.dtype} on {t.device}")
        call("srmi_fss", ptr(pred), ptr(truth), self.C, self.H, self.W, ptr(self.thresholds), self.T, self._scales,
             self.N, ptr(self.workspace), self.workspace.numel(), ptr(self.num), ptr(self.den), ptr(self.events),
             ptr(self.used), ptr(self.derived), int(launches), stream_handle())
        N = self.N
        res = {"num": self.num, "den": self.den, "events_pred": self.events[:, :, 0],
               "events_truth": self.events[:, :, 1], "used": self.used, "fss": self.derived[:, :, :N]}
        for i, name in enumerate(FSS_DERIVED):
            res[name] = self.derived[:, :, N + i]
        return res
