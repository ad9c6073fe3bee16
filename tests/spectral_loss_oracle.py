"""numpy / torch fp64 restatement of the spectral loss term (srmi_spectral_loss_*,
srmi.spectra.SpectralLoss, FusedTrainer(spectral=...)), written the slow, obvious way.  The
reference has no counterpart, so this file is the definition.

p (prediction) and t (target) are [N, C, H, W].  A job is one window of side P of one plane,
the windows at the overlap plan's origins min(i Q, L - P) on both axes, row-major.  A job is
skipped when any pixel of its window is non-finite in p or in t (per plane).  Per used job

    d = p - t (in the inputs' precision, fp32 for the device's inputs)
    z = h(y) h(x) d,   h(q) = 0.5 - 0.5 cos(2 pi q / P)     (the mean is not removed)
    D = DFT2(z), unnormalised;  c = P^2 W2, W2 = sum (h(y) h(x))^2
    A_k = sqrt(|D_k|^2 / c + eps)                             for each of the P^2 bins

S = sum over the used jobs and their bins of A_k, L_spec = S / (Nused P), and 0 with a zero
gradient when no job is used.  With G_k = D_k / (c A_k) the gradient is the unnormalised
inverse transform of G, tapered again, overlap-added and divided by Nused P.

``dtype='float64'`` is the definition.  ``dtype='complex64'`` runs the two transforms of
every job in single precision through scipy.fft (everything else stays fp64): the fp32
arithmetic from which the device tests take their bars."""
import numpy as np
import scipy.fft
import torch

import land_train_oracle as lt
import overlap_oracle as oo

EPS = 1e-12


def hann(P: int) -> np.ndarray:
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(P) / P)


def windows(H: int, W: int, P: int, Q: int):
    """[(y0, x0)] of the plan, row-major."""
    if P not in (16, 32, 64) or P > min(H, W) or not 1 <= Q <= P:
        raise ValueError(f"window {P} stride {Q} on planes {(H, W)}")
    return [(int(y0), int(x0)) for y0 in oo.origins(H, P, Q) for x0 in oo.origins(W, P, Q)]


def used_jobs(p: np.ndarray, t: np.ndarray, P: int, Q: int) -> np.ndarray:
    """[N, C, nwin] bool: no pixel of the window is non-finite in p or in t."""
    N, C, H, W = p.shape
    ok = np.isfinite(p) & np.isfinite(t)
    return np.array([[[ok[n, c, y0:y0 + P, x0:x0 + P].all() for y0, x0 in windows(H, W, P, Q)] for c in range(C)]
                     for n in range(N)])


def loss_and_grad(p: np.ndarray, t: np.ndarray, P: int, Q: int, eps: float = EPS, dtype: str = "float64"):
    """-> dict(loss, grad [N, C, H, W] fp64 = d loss / d p (0 where no used job reaches),
    parts [N, C] = the planes' sums of A, counts [N, C] = their used jobs, S, nused)."""
    N, C, H, W = p.shape
    wins = windows(H, W, P, Q)
    used = used_jobs(p, t, P, Q)
    h = hann(P)
    h2 = h[:, None] * h[None, :]
    c = P * P * (h2 ** 2).sum()
    parts = np.zeros((N, C))
    grad = np.zeros((N, C, H, W))
    for n in range(N):
        for ch in range(C):
            for w, (y0, x0) in enumerate(wins):
                if not used[n, ch, w]:
                    continue
                d = (p[n, ch, y0:y0 + P, x0:x0 + P] - t[n, ch, y0:y0 + P, x0:x0 + P]).astype(np.float64)
                z = h2 * d
                if dtype == "complex64":
                    D = scipy.fft.fft2(z.astype(np.complex64)).astype(np.complex128)
                elif dtype == "float64":
                    D = np.fft.fft2(z)
                else:
                    raise ValueError(dtype)
                A = np.sqrt(np.abs(D) ** 2 / c + eps)
                parts[n, ch] += A.sum()
                G = D / (c * A)
                if dtype == "complex64":
                    g = (scipy.fft.ifft2(G.astype(np.complex64)).astype(np.complex128) * (P * P)).real
                else:
                    g = (np.fft.ifft2(G) * (P * P)).real
                grad[n, ch, y0:y0 + P, x0:x0 + P] += h2 * g
    counts = used.sum(axis=2).astype(np.float64)
    nused = int(counts.sum())
    S = float(parts.sum())
    if nused == 0:
        return dict(loss=0.0, grad=np.zeros_like(grad), parts=parts, counts=counts, S=0.0, nused=0)
    return dict(loss=S / (nused * P), grad=grad / (nused * P), parts=parts, counts=counts, S=S, nused=nused)


def loss_torch(p: torch.Tensor, t: torch.Tensor, P: int, Q: int, eps: float = EPS):
    """The same loss as a differentiable torch expression -> (loss, nused); t (and the
    choice of the used jobs) are data."""
    N, C, H, W = p.shape
    used = used_jobs(p.detach().numpy(), t.detach().numpy(), P, Q)
    h = torch.tensor(hann(P), dtype=p.dtype)
    h2 = h[:, None] * h[None, :]
    c = P * P * (h2 ** 2).sum()
    total = torch.zeros((), dtype=p.dtype)
    for n in range(N):
        for ch in range(C):
            for w, (y0, x0) in enumerate(windows(H, W, P, Q)):
                if used[n, ch, w]:
                    D = torch.fft.fft2(h2 * (p[n, ch, y0:y0 + P, x0:x0 + P] - t[n, ch, y0:y0 + P, x0:x0 + P]))
                    total = total + torch.sqrt((D.real ** 2 + D.imag ** 2) / c + eps).sum()
    nused = int(used.sum())
    if nused == 0:
        return total * 0.0, 0
    return total / (nused * P), nused


def train_step(model, hr: np.ndarray, scale: int, loss_fn: str = "l2", spectral=None):
    """land_train_oracle.train_step with the term: one step of `model` (its dtype) on hr
    [B, C, T, T] (NaN on land allowed) with loss = masked pixel loss + weight * L_spec ->
    (total, out, {reference key: gradient}, dict(pixel_loss, spectral_loss, nused))."""
    model.zero_grad()
    dtype = next(model.parameters()).dtype
    h = torch.tensor(hr, dtype=dtype)
    lr = lt.filled_lr(h, scale) if not np.isfinite(hr).all() else lt.ro.downsample(h, scale)
    out = model(lr)
    pixel, _ = lt.masked_loss(out, h, loss_fn)
    total, spec, nused = pixel, torch.zeros((), dtype=dtype), 0
    if spectral is not None:
        spec, nused = loss_torch(out, h, int(spectral.get("window", 64)), int(spectral.get("stride", 32)),
                                 float(spectral.get("eps", EPS)))
        total = pixel + float(spectral.get("weight", 1.0)) * spec
    total.backward()
    grads = {n.replace(".conv.", "."): p.grad.detach().clone() for n, p in model.named_parameters()}
    return (float(total.detach()), out.detach(), grads,
            dict(pixel_loss=float(pixel.detach()), spectral_loss=float(spec.detach()), nused=nused))
