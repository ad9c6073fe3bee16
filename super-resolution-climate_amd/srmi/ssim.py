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
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Tuple

import torch

from ._lib import SRMI_ERR_ARG, call, load, ptr, stream_handle


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
