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

``SpectralLoss`` is the training-side companion (``srmi_spectral_loss_*``, no reference
counterpart either): a Fourier-amplitude term over windows of 16, 32 or 64 pixels that
``FusedTrainer(spectral=...)`` adds to its pixel loss.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Sequence, Tuple

import torch

from ._lib import SRMI_ERR_ARG, call, load, ptr, stream_handle
from .loss_term import LossTerm

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


SPECTRAL_LOSS_WINDOWS = (16, 32, 64)


def check_spectral_loss_config(window, stride, eps, weight) -> Tuple[int, int, float, float]:
    """(window, stride, eps, weight) as the kernels take them, or ValueError naming the
    offending value."""
    if isinstance(window, bool) or int(window) != window or int(window) not in SPECTRAL_LOSS_WINDOWS:
        raise ValueError(f"spectral loss window {window!r}: one of {SPECTRAL_LOSS_WINDOWS}")
    P = int(window)
    if stride is None:
        stride = P // 2
    if isinstance(stride, bool) or int(stride) != stride or not 1 <= int(stride) <= P:
        raise ValueError(f"spectral loss stride {stride!r}: an integer in 1 .. the window ({P})")
    eps, weight = float(eps), float(weight)
    if not (eps > 0.0 and math.isfinite(eps)) or C.c_float(eps).value <= 0.0:
        raise ValueError(f"spectral loss eps {eps!r}: a finite fp32 value > 0")
    if not (weight >= 0.0 and math.isfinite(weight)):
        raise ValueError(f"spectral loss weight {weight!r}: finite and >= 0")
    return P, int(stride), eps, weight


class SpectralLoss(LossTerm):
    """The spectral loss term of a training step (no reference counterpart; the definition
    is srmi.h's "spectral loss term", tests/spectral_loss_oracle.py restates it in fp64):
    with d = pred - target on every window of side ``window`` at stride ``stride`` of every
    plane, tapered by the periodic Hann window and transformed, ``L_spec = sum sqrt(|D_k|^2
    / c + eps) / (Nused * window)`` over the bins of the windows that hold no non-finite
    pixel.  For a white error it is about 0.89 of the RMSE.

    The object owns the workspace (the per-window gradients) of an [N, C, H, W] batch and
    the per-plane parts of a global batch of ``global_batch`` tiles (default N), so the
    steps are, as in FusedTrainer:

        parts(pred, target, rows=...)   per micro-batch, after the forward
        finalize(base)                  once the parts of the global batch are in place
        add_dy(dy, rows=...)            dy += weight * d L_spec / d pred

    (srmi.loss_term.LossTerm's protocol; finalize leaves spec4 = {S, Nused, 1 / (Nused window),
    L_spec} and total = base[0] + weight * L_spec).

    Nothing allocates or reads back: all three can be captured, and every result is
    bit-identical from run to run and independent of how the batch is split over calls.
    The taper is 0 at its first point, so the first row and column of a plane get no
    spectral gradient (the last ones nearly none): the pixel loss covers them."""

    name, record = "spectral", "spec4"
    DEFAULTS = dict(weight=1.0, window=64, stride=32, eps=1e-12)

    @staticmethod
    def check_config(weight, window, stride, eps) -> Dict[str, object]:
        P, Q, eps, weight = check_spectral_loss_config(window, stride, eps, weight)
        return dict(weight=weight, window=P, stride=Q, eps=eps)

    def __init__(self, shape: Sequence[int], window: int = 64, stride: Optional[int] = 32, eps: float = 1e-12,
                 weight: float = 1.0, device: Optional[torch.device] = None, global_batch: Optional[int] = None):
        super().__init__(shape, dict(weight=weight, window=window, stride=stride, eps=eps), device, global_batch)

    def _plan_args(self):
        return self.window, self.stride

    def _parts_args(self):
        return self.window, self.stride, self.eps

    def _finalize_args(self):  # spec4[2] = 1 / (Nused window)
        return self.window, self.weight

    def _no_fit(self) -> str:
        return f"spectral loss window {self.window} at stride {self.stride} does not fit planes of {(self.H, self.W)}"

    def add_dy(self, dy: torch.Tensor, pred=None, target=None, rows=None) -> None:
        """dy [n, C, H, W] (tiles rows .. of the batch, holding the pixel loss's upstream
        gradient) += weight * spec4[2] * the used windows' gradients, which ``parts`` left in
        the workspace: pred and target are not read.  weight == 0, or no used window over a
        pixel: its bits stay."""
        self._check("dy", dy)
        n = dy.shape[0]
        r0 = self._rows(n, rows)
        ws = self.workspace[r0 * self.C * self.plane_bytes:]
        call("srmi_spectral_loss_dy", ptr(ws), n * self.C * self.plane_bytes, n * self.C, self.H, self.W, self.window,
             self.stride, self.weight, ptr(self.spec4), ptr(dy), self._stream())


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
