"""SSIM and PSNR of a super-resolved field, with a per-pixel map of structural agreement.

No reference counterpart -- a deliberate extension, not a parity item.  The reference (and
``RegionSuperResolver.score``) judges a field by its RMSE, which rewards smooth output;
``srmi.spectra`` says at which wavelengths a field fails.  ``SSIMScore`` gives the pair of
numbers every super-resolution paper reports (RCAN and EDSR among them), PSNR and SSIM, and
the one thing none of the other scores has: a map that shows WHERE the field is wrong.  Its
contrast-structure factor ``cs`` is the standard single number for over-smooth output.

Definition (``srmi_ssim``, include/srmi.h; tests/ssim_oracle.py restates it in numpy)
-------------------------------------------------------------------------------------
Wang, Bovik, Sheikh, Simoncelli 2004 in its Gaussian form -- scikit-image's
``structural_similarity(gaussian_weights=True, use_sample_covariance=False)`` -- per
channel of a prediction ``a`` and a truth ``b``, [C, H, W]: an 11-tap separable Gaussian
window (sigma 1.5) on the valid positions only (no padding); a position is used iff its 121
pixels are finite in both fields in that channel (NaN is the land mask, decided per
channel); ``L`` is the truth's max - min over its finite pixels unless ``data_range`` is
given; every moment is formed on ``a - r`` and ``b - r`` with the pivot ``r`` the middle of
the truth's range, so that fp32 keeps the variance of a field at 290 +- 1.5; ``ssim`` =
luminance x ``cs``, ``cs`` = (2 s_ab + C2) / (s_aa + s_bb + C2), averaged over the used
positions; ``mse`` over every pixel finite in both, the border included; ``psnr`` =
10 log10(L^2 / mse).

Everything runs on the device in three launches without atomics or a host read, so
``measure`` can be captured in a HIP graph and its result is bit-identical from run to run.

``SSIMLoss`` is the training-side companion (``srmi_ssim_loss_*``, no reference counterpart):
1 - the mean of the same ssim over the used positions of a batch, and its closed-form
gradient, the term ``FusedTrainer(ssim=...)`` adds to its pixel loss.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Sequence, Tuple

import torch

from ._lib import SRMI_ERR_ARG, call, load, ptr, stream_handle
from .loss_term import LossTerm


def ssim_workspace(C_: int, H: int, W: int) -> int:
    """srmi_ssim_workspace (host only): the bytes, or ValueError where it returns
    SRMI_ERR_ARG."""
    n = C.c_size_t()
    rc = load().srmi_ssim_workspace(int(C_), int(H), int(W), C.byref(n))
    if rc == SRMI_ERR_ARG:
        raise ValueError(f"SSIM needs C >= 1 and H, W >= 11 (the window) with H W < 2^31, got {(C_, H, W)}")
    if rc:
        raise RuntimeError(f"srmi_ssim_workspace: {rc}")
    return int(n.value)


class SSIMScore:
    def __init__(self, shape: Tuple[int, int, int], data_range: Optional[float] = None, want_map: bool = False,
                 device: Optional[torch.device] = None):
        """shape: (C, H, W) of the fields; data_range: L for every channel, the truth's own
        max - min per channel when None (or <= 0); want_map: also fill the [C, H, W] map.
        Owns the workspace and the outputs: ``measure`` allocates nothing."""
        Cn, H, W = (int(v) for v in shape)
        nbytes = ssim_workspace(Cn, H, W)
        dr = 0.0 if data_range is None else float(data_range)
        if not math.isfinite(dr):
            raise ValueError(f"data_range {data_range!r}: a finite number (<= 0 or None: from the truth)")
        self.C, self.H, self.W, self.data_range = Cn, H, W, dr
        d = torch.device(device) if device is not None else torch.device("cuda")
        if d.type == "cuda" and d.index is None:
            d = torch.device("cuda", torch.cuda.current_device())
        self.device = d
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=d)
        self.out = torch.empty((Cn, 4), dtype=torch.float32, device=d)
        self.count = torch.zeros((Cn, 2), dtype=torch.int64, device=d)
        self.psnr = torch.empty(Cn, dtype=torch.float32, device=d)
        self.map = torch.empty((Cn, H, W), dtype=torch.float32, device=d) if want_map else None

    def measure(self, pred: torch.Tensor, truth: torch.Tensor) -> Dict[str, torch.Tensor]:
        """pred, truth [C, H, W] fp32 on the device (NaN / Inf allowed: they are the mask) ->
        device tensors, views of this object's buffers, valid until the next call: 'ssim',
        'cs', 'mse', 'data_range', 'psnr' [C] fp32; 'nwin', 'npix' [C] int64; with want_map
        'map' [C, H, W] (ssim at the used positions, NaN on the border and where a window
        touches a non-finite pixel).  'psnr' = 10 log10(L^2 / mse) is formed on the device.
        No used position: 'ssim' and 'cs' are NaN."""
        shape = (self.C, self.H, self.W)
        for name, t in (("pred", pred), ("truth", truth)):
            if (tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous()
                    or t.device != self.device):
                raise ValueError(f"{name}: a contiguous fp32 {shape} tensor on {self.device} is needed, got "
                                 f"{tuple(t.shape)} {t.dtype} on {t.device}")
        call("srmi_ssim", ptr(pred), ptr(truth), self.C, self.H, self.W, self.data_range, ptr(self.workspace),
             self.workspace.numel(), ptr(self.out), ptr(self.count), ptr(self.map), stream_handle())
        L, mse = self.out[:, 3], self.out[:, 2]
        torch.mul(L, L, out=self.psnr)
        self.psnr.div_(mse).log10_().mul_(10.0)
        res = {"ssim": self.out[:, 0], "cs": self.out[:, 1], "mse": mse, "data_range": L, "psnr": self.psnr,
               "nwin": self.count[:, 0], "npix": self.count[:, 1]}
        if self.map is not None:
            res["map"] = self.map
        return res


SSIM_WINDOW = 11


def check_ssim_loss_config(weight, data_range) -> Tuple[float, float]:
    """(weight, data_range) as the kernels take them -- data_range 0.0 for None or <= 0, "the
    target's own range per plane" -- or ValueError naming the offending value."""
    if isinstance(weight, bool) or not isinstance(weight, (int, float)):
        raise ValueError(f"ssim loss weight {weight!r}: finite and >= 0")
    weight = float(weight)
    if not (weight >= 0.0 and math.isfinite(weight)) or not math.isfinite(C.c_float(weight).value):
        raise ValueError(f"ssim loss weight {weight!r}: finite and >= 0")
    if data_range is None:
        return weight, 0.0
    if isinstance(data_range, bool) or not isinstance(data_range, (int, float)):
        raise ValueError(f"ssim loss data_range {data_range!r}: a finite number (<= 0 or None: from the target)")
    dr = float(data_range)
    if not math.isfinite(dr) or not math.isfinite(C.c_float(dr).value):
        raise ValueError(f"ssim loss data_range {dr!r}: a finite number (<= 0 or None: from the target)")
    return weight, dr if dr > 0.0 else 0.0


class SSIMLoss(LossTerm):
    """The SSIM loss term of a training step (no reference counterpart; the definition is
    srmi.h's "SSIM loss term", tests/ssim_loss_oracle.py restates it in fp64): ``L_ssim = 1 -
    S / Nused``, S the sum of ``SSIMScore``'s ssim over the used positions of every plane of
    the global batch -- a position is used iff the 121 pixels of its window are finite in
    pred and in target, the range ``L`` and the pivot are the target plane's -- and Nused their
    number.  The mean is over positions, not over per-plane means.

    The object owns the workspace (the coefficient maps of the closed-form gradient) of an
    [N, C, H, W] batch and the per-plane parts of a global batch of ``global_batch`` tiles
    (default N), so the steps are, as in FusedTrainer and as SpectralLoss's:

        parts(pred, target, rows=...)        per micro-batch, after the forward
        finalize(base)                       once the parts of the global batch are in place
        add_dy(dy, pred, target, rows=...)   dy += weight * d L_ssim / d pred

    (srmi.loss_term.LossTerm's protocol; finalize leaves ssim4 = {S, Nused, 1 / Nused, L_ssim}
    and total = base[0] + weight * L_ssim, base the finalised pixel loss, loss4[3:4], or the
    total of the term before).
    Nothing allocates or reads back: all three can be captured, and every result is
    bit-identical from run to run and independent of how the batch is split over calls."""

    name, record, window = "ssim", "ssim4", SSIM_WINDOW
    DEFAULTS = dict(weight=1.0, data_range=None)

    @staticmethod
    def check_config(weight, data_range) -> Dict[str, object]:
        weight, data_range = check_ssim_loss_config(weight, data_range)
        return dict(weight=weight, data_range=data_range)

    def __init__(self, shape: Sequence[int], weight: float = 1.0, data_range: Optional[float] = None,
                 device: Optional[torch.device] = None, global_batch: Optional[int] = None):
        super().__init__(shape, dict(weight=weight, data_range=data_range), device, global_batch)

    def _parts_args(self):
        return (self.data_range,)

    def add_dy(self, dy: torch.Tensor, pred: torch.Tensor, target: torch.Tensor, rows=None) -> None:
        """dy [n, C, H, W] (tiles rows .. of the batch, holding the upstream gradient so far)
        += -weight * ssim4[2] * dS / d pred, from the coefficient maps ``parts`` left for these
        tiles and the same pred / target.  weight == 0, or a pixel that is not finite in pred
        and in target: its bits stay."""
        n, r0 = self._check_dy(dy, pred, target, rows)
        ws = self.workspace[r0 * self.C * self.plane_bytes:]
        call("srmi_ssim_loss_dy", ptr(ws), n * self.C * self.plane_bytes, ptr(pred), ptr(target), n * self.C, self.H,
             self.W, self.weight, ptr(self.ssim4), ptr(dy), self._stream())
