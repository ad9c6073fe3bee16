"""The horizontal gradient of a super-resolved field: a score and a loss term.

No reference counterpart -- a deliberate extension, not a parity item.  The spectra say at
which scales a field lacks amplitude, SSIM's ``cs`` says "too smooth" in a window statistic,
the histograms look at values.  ``GradientScore`` looks at what an oceanographer computes
first from SST, SSS or SSH: |grad f|, where the fronts are.

Definition (``srmi_gradient``, include/srmi.h; tests/gradient_oracle.py restates it in numpy)
---------------------------------------------------------------------------------------------
The Sobel derivative at unit scale on a plane f[H][W], differences before sums::

    dX(y, x) = f(y, x+1) - f(y, x-1)            dY(y, x) = f(y+1, x) - f(y-1, x)
    Gx(y, x) = ((dX(y-1, x) + dX(y+1, x)) + 2 dX(y, x)) / 8
    Gy(y, x) = ((dY(y, x-1) + dY(y, x+1)) + 2 dY(y, x)) / 8

at the valid positions 1 <= y <= H - 2, 1 <= x <= W - 2 only; a position is used iff the nine
pixels of its window are finite in both fields of that plane (NaN / Inf are the mask: a coast
costs a one-pixel rim).  ``gx = Gx / dx``, ``gy = Gy / dy`` with the grid spacing (dy, dx).  Per
channel over the used positions: ``mean_pred``, ``mean_truth`` (the mean magnitudes),
``sharpness`` = their ratio (below 1: too smooth), ``rmse_mag``, ``rmse_vec`` and ``cosine``
(1: every front points as the truth's does).  The magnitude maps, NaN where a position is not
used, go through ``srmi.distribution.DistributionScore`` for a contingency table of fronts
above a threshold.

``GradientLoss`` is the training-side companion (``srmi_gradient_loss_*``): the mean over the
used positions of sqrt(Gx[e]^2 + Gy[e]^2 + eps), e = pred - target, and its closed-form
gradient, the term ``FusedTrainer(gradient=...)`` adds to its loss.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import SRMI_ERR_ARG, call, load, ptr, stream_handle
from .loss_term import LossTerm
from .gradient_names import GRADIENT_STATS, GRADIENT_SUMS  # noqa: F401  (the one copy of the column order)

GRADIENT_WINDOW = 3
# the pixels a workgroup owns (kGradTileH x kGradTileW of csrc/gradient_common.hpp): the
# score's workspace is 64 bytes per rectangle, which the tests check this against
GRADIENT_TILE = (16, 64)


def check_spacing(spacing) -> Tuple[float, float]:
    """(inv_dy, inv_dx) as the kernel takes them, np.float32(1) / np.float32(d), or ValueError."""
    try:
        dy, dx = spacing
    except (TypeError, ValueError):
        raise ValueError(f"spacing {spacing!r}: a (dy, dx) pair of finite numbers > 0") from None
    inv = []
    for d in (dy, dx):
        if isinstance(d, bool) or not isinstance(d, (int, float, np.floating, np.integer)):
            raise ValueError(f"spacing {spacing!r}: a (dy, dx) pair of finite numbers > 0")
        with np.errstate(all="ignore"):
            d32 = np.float32(d)
            r = np.float32(1) / d32
        if not (np.isfinite(d32) and d32 > 0 and np.isfinite(r) and r > 0):
            raise ValueError(f"spacing {spacing!r}: a (dy, dx) pair of finite numbers > 0 (in fp32, with a finite "
                             "reciprocal)")
        inv.append(float(r))
    return inv[0], inv[1]


def gradient_workspace(C_: int, H: int, W: int) -> int:
    """srmi_gradient_workspace (host only): the bytes, or ValueError where it returns
    SRMI_ERR_ARG."""
    n = C.c_size_t()
    rc = load().srmi_gradient_workspace(int(C_), int(H), int(W), C.byref(n))
    if rc == SRMI_ERR_ARG:
        raise ValueError(f"the gradient score needs C >= 1 and H, W >= 3 (the window) with H W < 2^31, got {(C_, H, W)}")
    if rc:
        raise RuntimeError(f"srmi_gradient_workspace: {rc}")
    return int(n.value)


class GradientScore:
    def __init__(self, shape: Tuple[int, int, int], spacing=(1.0, 1.0), want_maps: bool = False,
                 device: Optional[torch.device] = None):
        """shape: (C, H, W) of the fields; spacing: the grid spacing (dy, dx), so the results
        are in the field's units per unit length; want_maps: also fill the two [C, H, W]
        magnitude maps.  Owns the workspace and the outputs: ``measure`` allocates nothing."""
        self.inv_dy, self.inv_dx = check_spacing(spacing)
        Cn, H, W = (int(v) for v in shape)
        nbytes = gradient_workspace(Cn, H, W)
        self.C, self.H, self.W = Cn, H, W
        d = torch.device(device) if device is not None else torch.device("cuda")
        if d.type == "cuda" and d.index is None:
            d = torch.device("cuda", torch.cuda.current_device())
        self.device = d
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=d)
        self.count = torch.zeros(Cn, dtype=torch.int64, device=d)
        self.sums = torch.empty((Cn, len(GRADIENT_SUMS)), dtype=torch.float64, device=d)
        self.stats = torch.empty((Cn, len(GRADIENT_STATS)), dtype=torch.float64, device=d)
        self.gmag_pred = torch.empty((Cn, H, W), dtype=torch.float32, device=d) if want_maps else None
        self.gmag_truth = torch.empty((Cn, H, W), dtype=torch.float32, device=d) if want_maps else None

    def measure(self, pred: torch.Tensor, truth: torch.Tensor) -> Dict[str, torch.Tensor]:
        """pred, truth [C, H, W] fp32 on the device (NaN / Inf allowed: they are the mask) ->
        device tensors, views of this object's buffers, valid until the next call: 'count' [C]
        int64 (the used positions); 'mean_pred', 'mean_truth', 'sharpness', 'rmse_mag',
        'rmse_vec', 'cosine' [C] fp64; 'sums' [C, 7] fp64 (srmi_gradient's, from which they are
        formed on the device); with want_maps 'gmag_pred', 'gmag_truth' [C, H, W] fp32, NaN
        where a position is not used, the one-pixel border included.  No used position: count
        0 and NaN in every fp64 value."""
        shape = (self.C, self.H, self.W)
        for name, t in (("pred", pred), ("truth", truth)):
            if (tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous()
                    or t.device != self.device):
                raise ValueError(f"{name}: a contiguous fp32 {shape} tensor on {self.device} is needed, got "
                                 f"{tuple(t.shape)} {t.dtype} on {t.device}")
        call("srmi_gradient", ptr(pred), ptr(truth), self.C, self.H, self.W, self.inv_dy, self.inv_dx,
             ptr(self.workspace), self.workspace.numel(), ptr(self.count), ptr(self.sums), ptr(self.stats),
             ptr(self.gmag_pred), ptr(self.gmag_truth), stream_handle())
        res = {"count": self.count, "sums": self.sums}
        for i, name in enumerate(GRADIENT_STATS):
            res[name] = self.stats[:, i]
        if self.gmag_pred is not None:
            res["gmag_pred"] = self.gmag_pred
            res["gmag_truth"] = self.gmag_truth
        return res


def check_gradient_loss_config(weight, eps) -> Tuple[float, float]:
    """(weight, eps) as the kernels take them -- weight finite and >= 0, eps finite and > 0,
    both also as fp32 -- or ValueError naming the offending value."""
    if isinstance(weight, bool) or not isinstance(weight, (int, float)):
        raise ValueError(f"gradient loss weight {weight!r}: finite and >= 0")
    weight = float(weight)
    if not (weight >= 0.0 and math.isfinite(weight)) or not math.isfinite(C.c_float(weight).value):
        raise ValueError(f"gradient loss weight {weight!r}: finite and >= 0")
    if isinstance(eps, bool) or not isinstance(eps, (int, float)):
        raise ValueError(f"gradient loss eps {eps!r}: finite and > 0")
    eps = float(eps)
    e32 = C.c_float(eps).value
    if not (eps > 0.0 and math.isfinite(eps)) or not (e32 > 0.0 and math.isfinite(e32)):
        raise ValueError(f"gradient loss eps {eps!r}: finite and > 0 (in fp32 too)")
    return weight, eps


class GradientLoss(LossTerm):
    """The gradient loss term of a training step (no reference counterpart; the definition is
    srmi.h's "gradient loss term", tests/gradient_oracle.py restates it in fp64): ``L_grad = S /
    Nused``, S the sum of sqrt(Gx[e]^2 + Gy[e]^2 + eps), e = pred - target, over the used
    positions of every plane of the global batch -- a position is used iff the nine pixels of
    its window are finite in pred and in target -- and Nused their number.  The mean is over
    positions, not over per-plane means.

    The object owns the workspace (the workgroups' partial sums) of an [N, C, H, W] batch and
    the per-plane parts of a global batch of ``global_batch`` tiles (default N), so the steps
    are, as in FusedTrainer and as SSIMLoss's:

        parts(pred, target, rows=...)        per micro-batch, after the forward
        finalize(base)                       once the parts of the global batch are in place
        add_dy(dy, pred, target, rows=...)   dy += weight * d L_grad / d pred

    (srmi.loss_term.LossTerm's protocol; finalize leaves grad4 = {S, Nused, 1 / Nused, L_grad}
    and total = base[0] + weight * L_grad, base the total of the terms before this one).
    Nothing allocates or reads back: all three can be captured, and every result is
    bit-identical from run to run and independent of how the batch is split over calls."""

    name, record, window = "gradient", "grad4", GRADIENT_WINDOW
    DEFAULTS = dict(weight=1.0, eps=1e-6)

    @staticmethod
    def check_config(weight, eps) -> Dict[str, object]:
        weight, eps = check_gradient_loss_config(weight, eps)
        return dict(weight=weight, eps=eps)

    def __init__(self, shape: Sequence[int], weight: float = 1.0, eps: float = 1e-6,
                 device: Optional[torch.device] = None, global_batch: Optional[int] = None):
        super().__init__(shape, dict(weight=weight, eps=eps), device, global_batch)

    def _parts_args(self):
        return (self.eps,)

    def add_dy(self, dy: torch.Tensor, pred: torch.Tensor, target: torch.Tensor, rows=None) -> None:
        """dy [n, C, H, W] (holding the upstream gradient so far) += weight * grad4[2] * dS / d
        pred, recomputed from pred / target (nothing ``parts`` stored is read; rows is checked
        only).  weight == 0, or a pixel that is not finite in pred and in target: its bits
        stay."""
        n, _ = self._check_dy(dy, pred, target, rows)
        call("srmi_gradient_loss_dy", ptr(pred), ptr(target), n * self.C, self.H, self.W, self.eps, self.weight,
             ptr(self.grad4), ptr(dy), self._stream())
