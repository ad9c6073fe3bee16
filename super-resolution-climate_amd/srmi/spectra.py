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


class SpectralLoss:
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
        finalize(loss4)                 once the parts of the global batch are in place
        add_dy(dy, rows=...)            dy += weight * d L_spec / d pred

    Nothing allocates or reads back: all three can be captured, and every result is
    bit-identical from run to run and independent of how the batch is split over calls.
    The taper is 0 at its first point, so the first row and column of a plane get no
    spectral gradient (the last ones nearly none): the pixel loss covers them."""

    def __init__(self, shape: Sequence[int], window: int = 64, stride: Optional[int] = 32, eps: float = 1e-12,
                 weight: float = 1.0, device: Optional[torch.device] = None, global_batch: Optional[int] = None):
        self.window, self.stride, self.eps, self.weight = check_spectral_loss_config(window, stride, eps, weight)
        N, Cn, H, W = (int(v) for v in shape)
        if N < 1 or Cn < 1:
            raise ValueError(f"spectral loss over a batch {tuple(shape)}")
        self.N, self.C, self.H, self.W = N, Cn, H, W
        n = C.c_size_t()
        rc = load().srmi_spectral_loss_workspace(N * Cn, H, W, self.window, self.stride, C.byref(n))
        if rc == SRMI_ERR_ARG:
            raise ValueError(f"spectral loss window {self.window} at stride {self.stride} does not fit planes of "
                             f"{(H, W)}")
        if rc:
            raise RuntimeError(f"srmi_spectral_loss_workspace: {rc}")
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
        self.spec4 = torch.zeros(4, dtype=torch.float32, device=d)
        self.total = torch.zeros(1, dtype=torch.float32, device=d)

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
        """The parts and counts of pred / target [n, C, H, W]: tiles rows .. rows + n - 1 of
        this object's batch (their part of the workspace), tiles global_row .. of the
        global batch (their rows of parts / cparts; default: the same)."""
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
        call("srmi_spectral_loss_parts", ptr(pred), ptr(target), n * self.C, self.H, self.W, self.window, self.stride,
             self.eps, ptr(parts[g0 * self.C:]), ptr(cparts[g0 * self.C:]), ptr(ws), n * self.C * self.plane_bytes,
             torch.cuda.current_stream(self.device).cuda_stream)

    def finalize(self, loss4: torch.Tensor) -> Dict[str, torch.Tensor]:
        """spec4 = {S, Nused, 1 / (Nused window), L_spec} of the global batch's parts and
        total = loss4[3] + weight * L_spec; loss4 (the finalised pixel loss) is only read."""
        parts, cparts = self.views()
        call("srmi_spectral_loss_from_parts", ptr(parts), ptr(cparts), self.gb * self.C, self.window, self.weight,
             ptr(loss4), ptr(self.spec4), ptr(self.total), torch.cuda.current_stream(self.device).cuda_stream)
        return {"spec4": self.spec4, "total": self.total, "spectral_loss": self.spec4[3:4]}

    def add_dy(self, dy: torch.Tensor, rows=None) -> None:
        """dy [n, C, H, W] (tiles rows .. of the batch, holding the pixel loss's upstream
        gradient) += weight * spec4[2] * the used windows' gradients.  weight == 0, or no
        used window over a pixel: its bits stay."""
        self._check("dy", dy)
        n = dy.shape[0]
        r0 = self._rows(n, rows)
        ws = self.workspace[r0 * self.C * self.plane_bytes:]
        call("srmi_spectral_loss_dy", ptr(ws), n * self.C * self.plane_bytes, n * self.C, self.H, self.W, self.window,
             self.stride, self.weight, ptr(self.spec4), ptr(dy), torch.cuda.current_stream(self.device).cuda_stream)


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
