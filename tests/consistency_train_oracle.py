"""fp64 oracle of training through the consistency correction (srmi.consistency.
ConsistencyLayer, FusedTrainer(consistent=K), TiledInference(consistent=K)), written the
slow, obvious way on top of consistency_oracle, land_train_oracle and oracle.rcan_oracle.
The reference has no counterpart, so this file is the definition.

``layer`` is the correction as differentiable torch code: K literal steps of x <- x + U(M (lr
- D x)) with F.interpolate, M the active mask of the first iterate (lr finite and every tap
of D finite), a constant of the graph.  Autograd's vector-Jacobian product of it is what the
device's three adjoint kernels must compute.

``adjoint`` is that product from dense matrices in numpy, with D, U and the clamped stencil G
of consistency_oracle: with E = M (I - G), J = I - U P M D, P = sum_{k < K} E^k, and

    q = U^T g;   t_0 = q, t_{k+1} = (I - G^T)(M t_k), Q = sum_{k < K} t_k;   g0 = g - D^T (M Q)

``adjoint_gather`` / ``adjoint_iterate`` / ``adjoint_apply`` are its three device steps, and
the ``abs_*`` functions the sums of the absolute terms the device tests take their bars from.
The adjoint is that of a FINITE field x (a network's output); lr may hold NaN.

Modes are 'bilinear' / 'bicubic'; arrays are [..., H, W]."""
import numpy as np
import torch
import torch.nn.functional as F

import consistency_oracle as co
import land_train_oracle as lt
import spectral_loss_oracle as slo
from oracle import rcan_oracle as ro


# ------------------------------------------------------------------ the layer, in torch
def layer(x: torch.Tensor, lr: torch.Tensor, s: int, umode: str, dmode: str, K: int) -> torch.Tensor:
    """x [N, C, h s, w s] (differentiable), lr [N, C, h, w] (data; NaN = unconstrained
    cell) -> x_K.  Non-finite pixels of x pass through untouched."""
    def D(v):
        return F.interpolate(v, scale_factor=1.0 / s, mode=dmode, align_corners=False)

    def U(v):
        return F.interpolate(v, scale_factor=float(s), mode=umode, align_corners=False)
    lr = lr.detach()
    finx = torch.isfinite(x.detach())
    xs = torch.where(finx, x, torch.zeros_like(x))
    # a cell is active iff lr is finite there and no tap of D meets a non-finite pixel
    active = torch.isfinite(lr) & ~_tap_hits(~finx, s, dmode)
    lrz = torch.where(active, lr, torch.zeros_like(lr))
    for _ in range(K):
        xs = xs + U(torch.where(active, lrz - D(xs), torch.zeros_like(lrz)))
    return torch.where(finx, xs, x)


def _tap_hits(bad: torch.Tensor, s: int, dmode: str) -> torch.Tensor:
    """[N, C, h, w] bool: some tap of D at that cell reads a True pixel of bad."""
    b = bad.numpy().astype(np.float64)
    H, W = b.shape[-2:]
    my = (co.interp_matrix(H, H // s, float(s), dmode) != 0).astype(np.float64)
    mx = (co.interp_matrix(W, W // s, float(s), dmode) != 0).astype(np.float64)
    return torch.from_numpy((my @ b @ mx.T) > 0)


# ------------------------------------------------------- the adjoint, dense, in numpy
def _mats(h: int, w: int, s: int, umode: str, dmode: str):
    g = co.du_coeffs(s, umode, dmode)
    return dict(Uy=co.interp_matrix(h, h * s, 1.0 / s, umode), Ux=co.interp_matrix(w, w * s, 1.0 / s, umode),
                Dy=co.interp_matrix(h * s, h, float(s), dmode), Dx=co.interp_matrix(w * s, w, float(s), dmode),
                Gy=co.du_stencil_matrix(h, g), Gx=co.du_stencil_matrix(w, g))


def adjoint_gather(g, s: int, umode: str):
    """q = U^T g: [..., h s, w s] -> [..., h, w]."""
    g = np.asarray(g, dtype=np.float64)
    h, w = g.shape[-2] // s, g.shape[-1] // s
    return co.interp_matrix(h, h * s, 1.0 / s, umode).T @ g @ co.interp_matrix(w, w * s, 1.0 / s, umode)


def abs_adjoint_gather(g, s: int, umode: str):
    """sum |w_y w_x g| over the pixels that reach each cell."""
    g = np.abs(np.asarray(g, dtype=np.float64))
    h, w = g.shape[-2] // s, g.shape[-1] // s
    return np.abs(co.interp_matrix(h, h * s, 1.0 / s, umode)).T @ g @ np.abs(co.interp_matrix(w, w * s, 1.0 / s, umode))


def tap_sum_adjoint_gather(g, s: int, umode: str):
    """sum |g| over the pixels with a tap on each cell (the weight-evaluation term's T)."""
    g = np.abs(np.asarray(g, dtype=np.float64))
    h, w = g.shape[-2] // s, g.shape[-1] // s
    my = (co.interp_matrix(h, h * s, 1.0 / s, umode) != 0).astype(np.float64)
    mx = (co.interp_matrix(w, w * s, 1.0 / s, umode) != 0).astype(np.float64)
    return my.T @ g @ mx


def adjoint_iterate(t, active, s: int, umode: str, dmode: str):
    """t <- M t - G^T (M t) on [..., h, w] (not masked afterwards)."""
    h, w = t.shape[-2:]
    g = co.du_coeffs(s, umode, dmode)
    v = np.where(active, t, 0.0)
    return v - co.du_stencil_matrix(h, g).T @ v @ co.du_stencil_matrix(w, g)


def abs_adjoint_iterate(t, active, s: int, umode: str, dmode: str):
    h, w = t.shape[-2:]
    g = np.abs(co.du_coeffs(s, umode, dmode))
    v = np.abs(np.where(active, t, 0.0))
    return v + co.du_stencil_matrix(h, g).T @ v @ co.du_stencil_matrix(w, g)


def adjoint_apply(g, Q, active, s: int, dmode: str):
    """g - D^T (M Q)."""
    g = np.asarray(g, dtype=np.float64)
    h, w = Q.shape[-2:]
    return g - co.interp_matrix(h * s, h, float(s), dmode).T @ np.where(active, Q, 0.0) @ co.interp_matrix(
        w * s, w, float(s), dmode)


def abs_adjoint_apply(g, Q, active, s: int, dmode: str):
    h, w = Q.shape[-2:]
    return np.abs(g) + np.abs(co.interp_matrix(h * s, h, float(s), dmode)).T @ np.abs(
        np.where(active, Q, 0.0)) @ np.abs(co.interp_matrix(w * s, w, float(s), dmode))


def adjoint(g, active, s: int, umode: str, dmode: str, K: int):
    """J^T g -> (g0, q, Q, [t_0 .. t_K])."""
    q = adjoint_gather(g, s, umode)
    ts, Q = [q], np.zeros_like(q)
    for _ in range(K):
        Q = Q + ts[-1]
        ts.append(adjoint_iterate(ts[-1], active, s, umode, dmode))
    return adjoint_apply(g, Q, active, s, dmode), q, Q, ts


def jacobian_dense(active2d, s: int, umode: str, dmode: str, K: int) -> np.ndarray:
    """J = I - U P M D of one [h s, w s] plane as a dense matrix (row-major pixels)."""
    active2d = np.asarray(active2d, bool)
    h, w = active2d.shape
    m = _mats(h, w, s, umode, dmode)
    Uk, Dk, Gk = np.kron(m["Uy"], m["Ux"]), np.kron(m["Dy"], m["Dx"]), np.kron(m["Gy"], m["Gx"])
    M = np.diag(active2d.reshape(-1).astype(np.float64))
    E = M @ (np.eye(h * w) - Gk)
    P, Ek = np.zeros((h * w, h * w)), np.eye(h * w)
    for _ in range(K):
        P = P + Ek
        Ek = E @ Ek
    return np.eye(h * s * w * s) - Uk @ P @ M @ Dk


# ---------------------------------------------------------------------- the train step
def train_step(model, hr: np.ndarray, scale: int, loss_fn: str = "l2", K: int = 2, umode: str = "bicubic",
               dmode: str = "bicubic", land: bool = False, spectral=None):
    """spectral_loss_oracle.train_step with the layer behind the model: one step of `model`
    (its dtype) on hr [B, C, T, T] (land: NaN on land) -> (total, out, {reference key:
    gradient}, dict(pixel_loss, spectral_loss, nused, lr: the LR batch the constraint is
    imposed against (NaN where a tap is dry), out0: the network's own output, g: d loss / d
    out, g0: d loss / d out0)).  K = 0 is the step without the layer."""
    model.zero_grad()
    dtype = next(model.parameters()).dtype
    h = torch.tensor(hr, dtype=dtype)
    lr = ro.downsample(h, scale, mode=dmode)
    if land:
        assert dmode == "bicubic"  # land_train_oracle's fill follows the bicubic taps
        lr_in = lt.filled_lr(h, scale)
    else:
        lr_in = lr
    out0 = model(lr_in)
    out0.retain_grad()
    out = layer(out0, lr, scale, umode, dmode, K) if K else out0 * 1.0
    out.retain_grad()
    pixel, _ = lt.masked_loss(out, h, loss_fn)
    total, spec, nused = pixel, torch.zeros((), dtype=dtype), 0
    if spectral is not None:
        spec, nused = slo.loss_torch(out, h, int(spectral.get("window", 64)), int(spectral.get("stride", 32)),
                                     float(spectral.get("eps", slo.EPS)))
        total = pixel + float(spectral.get("weight", 1.0)) * spec
    total.backward()
    grads = {n.replace(".conv.", "."): p.grad.detach().clone() for n, p in model.named_parameters()}
    return (float(total.detach()), out.detach(), grads,
            dict(pixel_loss=float(pixel.detach()), spectral_loss=float(spec.detach()), nused=nused,
                 lr=lr.detach().numpy(), out0=out0.detach().numpy(), g=out.grad.detach().numpy(),
                 g0=out0.grad.detach().numpy()))
