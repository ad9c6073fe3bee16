"""The protocol of an auxiliary loss term of the training step, host side.

``LossTerm`` is what ``SpectralLoss`` (srmi.spectra), ``SSIMLoss`` (srmi.ssim) and
``GradientLoss`` (srmi.gradient) share, and what ``FusedTrainer`` drives for every term it is
given, in term order (DESIGN.md §1 "The loss-term protocol"):

    parts(pred, target, rows=...)        per micro-batch, after the forward
    (the all-reduce of gparts)           data parallel only
    finalize(base)                       total = base[0] + weight * L; base is the term before's
    add_dy(dy, pred, target, rows=...)   dy += weight * d L / d pred

A term owns a workspace for an [N, C, H, W] batch, sized by its ``*_workspace`` entry point,
and the per-plane parts and counts of a global batch of up to ``global_batch`` tiles.  Nothing
allocates or reads back after the constructor.

A subclass supplies ``name`` (its entry points are ``srmi_{name}_loss_*``, its output key is
``f"{name}_loss"``), ``record`` (the name its 4-float record also goes by: ``spec4``),
``DEFAULTS`` (its configuration's keys and defaults), ``check_config``, ``window`` (the
smallest plane side: a class attribute, or a key of the configuration), the extra scalar
arguments of its three calls (``_plan_args``, ``_parts_args``, ``_finalize_args``) and
``add_dy``.  Its constructor hands its configuration to ``LossTerm.__init__``, which keeps the
checked values as attributes, ``weight`` among them.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import torch

from ._lib import SRMI_ERR_ARG, call, load, ptr


class LossTerm:
    name: str = ""
    record: str = ""
    window: Optional[int] = None
    DEFAULTS: Dict[str, object] = {}

    @staticmethod
    def check_config(**cfg) -> Dict[str, object]:
        """The configuration (every key of DEFAULTS) as the constructor takes it, or ValueError
        naming the offending value."""
        raise NotImplementedError

    def _plan_args(self) -> tuple:
        """What ``srmi_{name}_loss_workspace`` takes between (nplanes, H, W) and the result."""
        return ()

    def _parts_args(self) -> tuple:
        """What ``srmi_{name}_loss_parts`` takes between (.., H, W) and parts."""
        raise NotImplementedError

    def _finalize_args(self) -> tuple:
        """What ``srmi_{name}_loss_from_parts`` takes between nplanes and base."""
        return (self.weight,)

    def _no_fit(self) -> str:
        """The ValueError text for planes the workspace entry point refuses."""
        return (f"{self.name} loss needs planes of H, W >= {self.window} (the window) with H W <= 2^24, got "
                f"{(self.H, self.W)}")

    def __init__(self, shape: Sequence[int], cfg: Dict[str, object], device: Optional[torch.device] = None,
                 global_batch: Optional[int] = None):
        for k, v in self.check_config(**cfg).items():  # weight, and what the term's calls take
            setattr(self, k, v)
        N, Cn, H, W = (int(v) for v in shape)
        if N < 1 or Cn < 1:
            raise ValueError(f"{self.name} loss over a batch {tuple(shape)}")
        self.N, self.C, self.H, self.W = N, Cn, H, W
        n = C.c_size_t()
        entry = f"srmi_{self.name}_loss_workspace"
        rc = getattr(load(), entry)(N * Cn, H, W, *self._plan_args(), C.byref(n))
        if rc == SRMI_ERR_ARG:
            raise ValueError(self._no_fit())
        if rc:
            raise RuntimeError(f"{entry}: {rc}")
        self.plane_bytes = int(n.value) // (N * Cn)
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        d = self.device
        self.workspace = torch.empty(int(n.value), dtype=torch.uint8, device=d)
        self.gcap = N if global_batch is None else int(global_batch)
        if self.gcap < N:
            raise ValueError(f"global batch {self.gcap} smaller than the batch {N}")
        # [parts | cparts] of the gb <= gcap tiles of a step, gb * C each (one all-reduce)
        self.gparts = torch.zeros(2 * self.gcap * Cn, dtype=torch.float32, device=d)
        self.gb = self.gcap
        self.term4 = torch.zeros(4, dtype=torch.float32, device=d)  # {S, Nused, the gradient's scale, L}
        setattr(self, self.record, self.term4)
        self.total = torch.zeros(1, dtype=torch.float32, device=d)

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def _rows(self, n: int, rows) -> int:
        r0 = 0 if rows is None else int(rows.start or 0) if isinstance(rows, slice) else int(rows)
        if isinstance(rows, slice) and rows.stop is not None and rows.stop - r0 != n:
            raise ValueError(f"rows {rows} for {n} tiles")
        if r0 < 0 or n < 1 or r0 + n > self.N:
            raise ValueError(f"tiles {r0} .. {r0 + n - 1} outside the batch of {self.N}")
        return r0

    def _check(self, name: str, t: torch.Tensor) -> None:
        if (t.dim() != 4 or tuple(t.shape[1:]) != (self.C, self.H, self.W) or t.dtype != torch.float32
                or not t.is_contiguous()):
            raise ValueError(f"{name}: a contiguous fp32 [n, {self.C}, {self.H}, {self.W}] tensor is needed, got "
                             f"{tuple(t.shape)} {t.dtype}")

    def _check_dy(self, dy: torch.Tensor, pred: torch.Tensor, target: torch.Tensor, rows) -> Tuple[int, int]:
        """(n, r0) of an ``add_dy`` over dy, pred and target [n, C, H, W]."""
        self._check("dy", dy)
        self._check("pred", pred)
        self._check("target", target)
        n = dy.shape[0]
        if pred.shape[0] != n or target.shape[0] != n:
            raise ValueError(f"dy of {n} tiles, pred of {pred.shape[0]}, target of {target.shape[0]}")
        return n, self._rows(n, rows)

    def set_global_batch(self, gb: int) -> None:
        """The tiles of this step's global batch (<= global_batch): where cparts begins."""
        if not 1 <= gb <= self.gcap:
            raise ValueError(f"global batch {gb} outside 1 .. {self.gcap}")
        self.gb = int(gb)

    def views(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(parts, cparts) of the step's global batch, gb * C each, adjacent."""
        n = self.gb * self.C
        return self.gparts[:n], self.gparts[n:2 * n]

    def parts(self, pred: torch.Tensor, target: torch.Tensor, rows=None, global_row: Optional[int] = None) -> None:
        """The sums and used counts of pred / target [n, C, H, W]: tiles rows .. rows + n - 1 of
        this object's batch (their part of the workspace), tiles global_row .. of the global
        batch (their rows of parts / cparts; default: the same)."""
        self._check("pred", pred)
        self._check("target", target)
        n = pred.shape[0]
        if target.shape[0] != n:
            raise ValueError(f"pred of {n} tiles, target of {target.shape[0]}")
        r0 = self._rows(n, rows)
        g0 = r0 if global_row is None else int(global_row)
        if g0 < 0 or g0 + n > self.gb:
            raise ValueError(f"tiles {g0} .. {g0 + n - 1} outside the global batch of {self.gb}")
        parts, cparts = self.views()
        ws = self.workspace[r0 * self.C * self.plane_bytes:]
        call(f"srmi_{self.name}_loss_parts", ptr(pred), ptr(target), n * self.C, self.H, self.W, *self._parts_args(),
             ptr(parts[g0 * self.C:]), ptr(cparts[g0 * self.C:]), ptr(ws), n * self.C * self.plane_bytes,
             self._stream())

    def finalize(self, base: torch.Tensor) -> Dict[str, torch.Tensor]:
        """term4 = {S, Nused, the gradient's scale, L} of the global batch's parts and counts
        and total = base[0] + weight * L; base (one device float: the finalised pixel loss,
        loss4[3:4], or the total of the term before this one) is only read."""
        parts, cparts = self.views()
        call(f"srmi_{self.name}_loss_from_parts", ptr(parts), ptr(cparts), self.gb * self.C, *self._finalize_args(),
             ptr(base), ptr(self.term4), ptr(self.total), self._stream())
        return {self.record: self.term4, "total": self.total, f"{self.name}_loss": self.term4[3:4]}

    def add_dy(self, dy: torch.Tensor, pred: torch.Tensor, target: torch.Tensor, rows=None) -> None:
        """dy [n, C, H, W] (tiles rows .. of the batch, holding the upstream gradient so far)
        += weight * term4[2] * d S / d pred."""
        raise NotImplementedError
