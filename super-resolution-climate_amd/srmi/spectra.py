"""The spectral score of a super-resolved field: windowed radial power spectra.

No reference counterpart -- a deliberate extension, not a parity item.  The reference
(and ``RegionSuperResolver.score``) judges a field by its RMSE, the quantity the network
is trained on, which rewards smooth output.  ``SpectralScore`` answers what a user of an
ocean super-resolution product asks first: down to which wavelength does the prediction
hold real variance, and where does it stop doing better than the baseline?

Definition (``srmi_spectra``, include/srmi.h; tests/spectra_oracle.py restates it in numpy)
----------------------------------------------------------------------------------------
The fields ``a`` (prediction) and ``b`` (truth), [C, H, W], are cut into windows of side
``P`` (a power of two, 16 .. 256) at stride ``Q`` by the overlap plan (origins
``min(i Q, L - P)``: the last window is shifted inward).  A window holding a non-finite
pixel of either field in any channel is skipped; ``nused`` counts the others.  Per used
window and channel each field has its own mean removed (fp64), is tapered by the
separable periodic Hann window and transformed; with ``W2 = sum (h h)^2`` the densities
``|Fa|^2``, ``|Fb|^2``, ``|Fa - Fb|^2`` and ``Re(Fa conj Fb)``, each over ``P^2 W2``, are
summed over the shells ``j = floor(|k| + 0.5)``, ``j = 0 .. P/2`` (the corners beyond are
dropped), and averaged over the used windows (Welch).

Everything runs on the device in three launches without atomics or a host read, so
``measure`` can be captured in a HIP graph and its result is bit-identical from run to
run.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import torch

from ._lib import SRMI_ERR_ARG, call, load, ptr, stream_handle

QUANTITIES = ("power_pred", "power_truth", "power_error", "cross")


def spectra_workspace(C_: int, H: int, W: int, P: int, Q: int) -> int:
    """srmi_spectra_workspace (host only): the bytes, or ValueError where it returns
    SRMI_ERR_ARG."""
    n = C.c_size_t()
    rc = load().srmi_spectra_workspace(int(C_), int(H), int(W), int(P), int(Q), C.byref(n))
    if rc == SRMI_ERR_ARG:
        raise ValueError(f"spectral window {P} (a power of two in 16 .. 256, <= min(H, W)) at stride {Q} (1 .. window) "
                         f"does not fit a field {(C_, H, W)}")
    if rc:
        raise RuntimeError(f"srmi_spectra_workspace: {rc}")
    return int(n.value)


class SpectralScore:
    def __init__(self, chw: Tuple[int, int, int], window: int = 256, stride: Optional[int] = None,
                 device: Optional[torch.device] = None):
        """chw: (C, H, W) of the fields; window: the side P; stride: Q, window // 2 when
        None.  Owns the workspace and the outputs: ``measure`` allocates nothing."""
        Cn, H, W = (int(v) for v in chw)
        P = int(window)
        Q = P // 2 if stride is None else int(stride)
        nbytes = spectra_workspace(Cn, H, W, P, Q)
        self.C, self.H, self.W, self.window, self.stride = Cn, H, W, P, Q
        self.K = P // 2 + 1
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        d = self.device
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=d)
        self.out = torch.empty((Cn, 4, self.K), dtype=torch.float32, device=d)
        self.nused = torch.zeros(1, dtype=torch.int32, device=d)
        self.ratios = torch.empty((3, Cn, self.K), dtype=torch.float32, device=d)
        self.wavenumber = torch.arange(self.K, dtype=torch.float32, device=d) / P  # cycles per pixel

    def measure(self, pred: torch.Tensor, truth: torch.Tensor) -> Dict[str, torch.Tensor]:
        """pred, truth [C, H, W] fp32 on the device (NaN / Inf allowed: their windows are
        skipped) -> device tensors, views of this object's buffers, valid until the next
        call: 'power_pred', 'power_truth', 'power_error', 'cross' [C, K]; 'nused' [1] int32;
        'wavenumber' [K] in cycles per pixel (j / P); and, formed on the device,
        'error_ratio' = Eee / Ebb, 'power_ratio' = Eaa / Ebb, 'coherence' = Cab^2 / (Eaa Ebb).
        No used window: every spectrum is NaN."""
        shape = (self.C, self.H, self.W)
        for name, t in (("pred", pred), ("truth", truth)):
            if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"{name}: a contiguous fp32 {shape} tensor is needed, got {tuple(t.shape)} {t.dtype}")
        call("srmi_spectra", ptr(pred), ptr(truth), self.C, self.H, self.W, self.window, self.stride,
             ptr(self.workspace), self.workspace.numel(), ptr(self.out), ptr(self.nused), stream_handle())
        Eaa, Ebb, Eee, Cab = self.out[:, 0], self.out[:, 1], self.out[:, 2], self.out[:, 3]
        torch.div(Eee, Ebb, out=self.ratios[0])
        torch.div(Eaa, Ebb, out=self.ratios[1])
        torch.mul(Cab, Cab, out=self.ratios[2])
        self.ratios[2].div_(Eaa).div_(Ebb)
        return {"power_pred": Eaa, "power_truth": Ebb, "power_error": Eee, "cross": Cab, "nused": self.nused,
                "wavenumber": self.wavenumber, "error_ratio": self.ratios[0], "power_ratio": self.ratios[1],
                "coherence": self.ratios[2]}


def effective_resolution(error_ratio, window: int, threshold: float = 0.5) -> Sequence[float]:
    """Host helper.  error_ratio [C, K] (a tensor or an array; K = window // 2 + 1): per
    channel the wavelength in pixels, window / j, of the first shell j >= 1 whose error
    ratio reaches ``threshold`` -- the scale below which the prediction's error is no
    longer small against the truth's variance.  2.0 (the Nyquist wavelength) when no shell
    does; a NaN ratio never reaches it."""
    import numpy as np
    r = error_ratio.detach().cpu().numpy() if isinstance(error_ratio, torch.Tensor) else np.asarray(error_ratio)
    P = int(window)
    if r.ndim != 2 or r.shape[1] != P // 2 + 1:
        raise ValueError(f"error_ratio {r.shape} is not [C, {P // 2 + 1}]")
    res = []
    for row in r:
        hit = [j for j in range(1, row.shape[0]) if row[j] >= threshold]
        res.append(P / hit[0] if hit else 2.0)
    return res
