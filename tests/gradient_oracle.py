"""numpy / torch restatement of the gradient score (srmi_gradient, srmi.gradient.GradientScore)
and of the gradient loss term (srmi_gradient_loss_*, srmi.gradient.GradientLoss,
FusedTrainer(gradient=...)), written the obvious way.  The reference has no counterpart, so
this file is the definition (include/srmi.h, "the gradient score", "the gradient loss term").

The operator is the Sobel derivative at unit scale on a plane f[H][W], differences first:

    dX(y, x) = f(y, x+1) - f(y, x-1)            dY(y, x) = f(y+1, x) - f(y-1, x)
    Gx(y, x) = ((dX(y-1, x) + dX(y+1, x)) + 2 dX(y, x)) / 8
    Gy(y, x) = ((dY(y, x-1) + dY(y, x+1)) + 2 dY(y, x)) / 8

at the valid positions 1 <= y <= H - 2, 1 <= x <= W - 2 ([H - 2][W - 2] maps).  A position is
USED iff the nine pixels of its window are finite in both fields of the plane.

Score: gx = Gx inv_dx, gy = Gy inv_dy, |g| = sqrt(gx gx + gy gy); per plane over the used
positions n and the seven sums, from which mean_pred, mean_truth, sharpness, rmse_mag, rmse_vec
and cosine follow.  The sums are fp64 whatever ``dtype`` the gradients were formed in.

Loss: e = pred - target (0 where a pixel is not finite in both), a = Gx[e], b = Gy[e], phi =
sqrt(a a + b b + eps); S the sum of phi over the used positions of ALL planes, Nused their
number, L_grad = S / Nused (0, with a zero gradient, when Nused = 0): a mean over positions, not
over per-plane means.  With U = a / phi, V = b / phi (0 where a position is not used)

    dS / dpred (q) = (Gx^T U)(q) + (Gy^T V)(q) = -(Gx[U~] + Gy[V~])(q)

U~, V~ the maps zero-extended by two pixels on every side: the operator is antisymmetric.

``dtype=np.float64`` is the definition.  ``dtype=np.float32`` does the same operations in the
same order in single precision: the arithmetic from which the device tests take their bars."""
import numpy as np
import torch

import land_train_oracle as lt
import spectral_loss_oracle as slo
import ssim_loss_oracle as sl

EPS = 1e-6
from srmi.gradient_names import GRADIENT_STATS as STATS, GRADIENT_SUMS as SUMS  # noqa: E402  (srmi_gradient's column order)


def sobel(f: np.ndarray):
    """f [H, W] -> (Gx, Gy) [H - 2, W - 2] in f's dtype, the operation order of the definition."""
    dt = f.dtype.type
    with np.errstate(invalid="ignore", over="ignore"):
        dX = f[:, 2:] - f[:, :-2]    # [H, W - 2]: dX(y, x), x = 1 .. W - 2
        dY = f[2:, :] - f[:-2, :]    # [H - 2, W]: dY(y, x), y = 1 .. H - 2
        Gx = ((dX[:-2] + dX[2:]) + dt(2) * dX[1:-1]) / dt(8)
        Gy = ((dY[:, :-2] + dY[:, 2:]) + dt(2) * dY[:, 1:-1]) / dt(8)
    return Gx, Gy


def used_positions(fin: np.ndarray) -> np.ndarray:
    """fin [H, W] bool -> [H - 2, W - 2] bool: all nine pixels of the window are fin."""
    H, W = fin.shape
    u = np.ones((H - 2, W - 2), bool)
    for dy in range(3):
        for dx in range(3):
            u &= fin[dy:dy + H - 2, dx:dx + W - 2]
    return u


def inv_spacing(spacing):
    """(inv_dy, inv_dx) as fp32, formed as the Python side forms them."""
    return tuple(np.float32(1) / np.float32(d) for d in spacing)


def score_plane(p: np.ndarray, t: np.ndarray, spacing=(1.0, 1.0), dtype=np.float64) -> dict:
    """One plane p, t [H, W] -> dict(count, the seven SUMS (fp64), the six STATS (fp64; NaN when
    count is 0), gmag_pred / gmag_truth [H, W] (`dtype`, NaN where a position is not used))."""
    dt = np.dtype(dtype).type
    H, W = p.shape
    inv_dy, inv_dx = (dt(v) for v in inv_spacing(spacing))
    fin = np.isfinite(p) & np.isfinite(t)
    used = used_positions(fin)
    with np.errstate(invalid="ignore", over="ignore"):
        pGx, pGy = sobel(p.astype(dt))
        tGx, tGy = sobel(t.astype(dt))
        pgx, pgy, tgx, tgy = pGx * inv_dx, pGy * inv_dy, tGx * inv_dx, tGy * inv_dy
        p2 = pgx * pgx + pgy * pgy
        t2 = tgx * tgx + tgy * tgy
        pm, tm = np.sqrt(p2), np.sqrt(t2)
    u = used
    d = np.float64
    n = int(u.sum())
    vals = dict(sum_mag_pred=pm[u].astype(d).sum(), sum_mag_truth=tm[u].astype(d).sum(),
                sum_dmag2=((pm[u].astype(d) - tm[u].astype(d)) ** 2).sum(),
                sum_dvec2=((pgx[u].astype(d) - tgx[u].astype(d)) ** 2 + (pgy[u].astype(d) - tgy[u].astype(d)) ** 2).sum(),
                sum_dot=(pgx[u].astype(d) * tgx[u].astype(d) + pgy[u].astype(d) * tgy[u].astype(d)).sum(),
                sum_pred2=p2[u].astype(d).sum(), sum_truth2=t2[u].astype(d).sum())
    res = dict(count=n)
    gp = np.full((H, W), np.nan, dtype=dt)
    gt = np.full((H, W), np.nan, dtype=dt)
    gp[1:-1, 1:-1][u] = pm[u]
    gt[1:-1, 1:-1][u] = tm[u]
    res.update(gmag_pred=gp, gmag_truth=gt)
    if n == 0:
        res.update({k: np.nan for k in SUMS + STATS})
        return res
    res.update({k: float(v) for k, v in vals.items()})
    with np.errstate(invalid="ignore", divide="ignore"):
        mp, mt = vals["sum_mag_pred"] / n, vals["sum_mag_truth"] / n
        res.update(mean_pred=mp, mean_truth=mt, sharpness=np.float64(mp) / np.float64(mt),
                   rmse_mag=np.sqrt(vals["sum_dmag2"] / n), rmse_vec=np.sqrt(vals["sum_dvec2"] / n),
                   cosine=np.float64(vals["sum_dot"]) / np.sqrt(np.float64(vals["sum_pred2"]) * vals["sum_truth2"]))
    return res


def score(p: np.ndarray, t: np.ndarray, spacing=(1.0, 1.0), dtype=np.float64) -> dict:
    """p, t [C, H, W] -> the entries of score_plane stacked over the channels."""
    rows = [score_plane(p[c], t[c], spacing, dtype) for c in range(p.shape[0])]
    return {k: np.stack([np.asarray(r[k]) for r in rows]) for k in rows[0]}


def zero_extended(M: np.ndarray) -> np.ndarray:
    """[Hv, Wv] -> [Hv + 4, Wv + 4], M in the middle."""
    P = np.zeros((M.shape[0] + 4, M.shape[1] + 4), dtype=M.dtype)
    P[2:-2, 2:-2] = M
    return P


def plane_terms(a: np.ndarray, b: np.ndarray, eps=EPS, dtype=np.float64) -> dict:
    """One plane pred a, target b [H, W] -> dict(used [Hv, Wv], phi [Hv, Wv] (garbage where not
    used), U, V [Hv, Wv] (0 where not used), dS [H, W] (0 where the pixel is not finite in both),
    fin [H, W])."""
    dt = np.dtype(dtype).type
    fin = np.isfinite(a) & np.isfinite(b)
    used = used_positions(fin)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        e = np.where(fin, a.astype(dt) - b.astype(dt), dt(0))
        ga, gb = sobel(e)
        phi = np.sqrt((ga * ga + gb * gb) + dt(eps))
        U = np.where(used, ga / phi, dt(0))
        V = np.where(used, gb / phi, dt(0))
        gxu, _ = sobel(zero_extended(U))
        _, gyv = sobel(zero_extended(V))
        dS = -(gxu + gyv)
    return dict(used=used, phi=phi, U=U, V=V, dS=np.where(fin, dS, dt(0)), fin=fin)


def loss_and_grad(a: np.ndarray, b: np.ndarray, eps=EPS, dtype=np.float64) -> dict:
    """a, b [..., H, W] -> dict(loss, grad [..., H, W] fp64 = d L_grad / d a (0 where a pixel
    takes none), dS [..., H, W] (`dtype`: the unscaled dS / da), parts [...] fp64 = the planes'
    sums of phi, counts [...] = their used positions, S, nused, fin [..., H, W])."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.ndim < 2 or a.shape[-2] < 3 or a.shape[-1] < 3:
        raise ValueError(f"fields {a.shape} / {b.shape}: two [..., H >= 3, W >= 3] arrays")
    if not (np.isfinite(eps) and eps > 0):
        raise ValueError(f"eps {eps!r}")
    dt = np.dtype(dtype).type
    lead, (H, W) = a.shape[:-2], a.shape[-2:]
    a3, b3 = a.reshape((-1, H, W)), b.reshape((-1, H, W))
    n = a3.shape[0]
    parts, counts = np.zeros(n), np.zeros(n)
    dS = np.zeros((n, H, W), dtype=dt)
    fin = np.zeros((n, H, W), bool)
    for p in range(n):
        t = plane_terms(a3[p], b3[p], eps, dtype)
        parts[p] = t["phi"][t["used"]].astype(np.float64).sum()
        counts[p] = t["used"].sum()
        dS[p] = t["dS"]
        fin[p] = t["fin"]
    nused = int(counts.sum())
    S = float(parts.sum())
    shape = lead + (H, W)
    res = dict(parts=parts.reshape(lead), counts=counts.reshape(lead), dS=dS.reshape(shape), fin=fin.reshape(shape),
               nused=nused)
    if nused == 0:
        res.update(loss=0.0, S=0.0, grad=np.zeros(shape))
        return res
    scale = dt(1.0 / nused)
    res.update(loss=S / nused, S=S, grad=(scale * dS).astype(np.float64).reshape(shape))
    return res


def _sobel_torch(e: torch.Tensor):
    dX = e[:, 2:] - e[:, :-2]
    dY = e[2:, :] - e[:-2, :]
    return ((dX[:-2] + dX[2:]) + 2 * dX[1:-1]) / 8, ((dY[:, :-2] + dY[:, 2:]) + 2 * dY[:, 1:-1]) / 8


def loss_torch(p: torch.Tensor, t: torch.Tensor, eps=EPS):
    """The same loss as a differentiable torch expression in p's dtype -> (loss, nused); t and
    the choice of the used positions are data."""
    H, W = p.shape[-2:]
    p3 = p.reshape((-1, H, W))
    t3 = t.detach().reshape((-1, H, W)).to(p.dtype)
    zero = torch.zeros((), dtype=p.dtype)
    total = torch.zeros((), dtype=p.dtype)
    nused = 0
    for k in range(p3.shape[0]):
        fin_np = np.isfinite(p3[k].detach().numpy()) & np.isfinite(t3[k].numpy())
        used = torch.from_numpy(used_positions(fin_np))
        if not bool(used.any()):
            continue
        e = torch.where(torch.from_numpy(fin_np), p3[k] - t3[k], zero)
        a, b = _sobel_torch(e)
        phi = torch.sqrt(a * a + b * b + eps)
        total = total + phi[used].sum()
        nused += int(used.sum())
    if nused == 0:  # 0, with a zero gradient
        return torch.where(torch.isfinite(p3.detach()), p3, zero).sum() * 0.0, 0
    return total / nused, nused


def train_step(model, hr: np.ndarray, scale: int, loss_fn: str = "l2", gradient_cfg=None, ssim_cfg=None,
               spectral_cfg=None, consistent: int = 0, land: bool = False):
    """ssim_loss_oracle.train_step with the term behind the others: one step of `model` (its
    dtype) on hr [B, C, T, T] (NaN on land allowed) with loss = masked pixel loss (+ weight_spec
    * L_spec) (+ weight_ssim * L_ssim) + weight * L_grad -> (total, out, {reference key:
    gradient}, dict(pixel_loss, spectral_loss, ssim_loss, gradient_loss, nused (the gradient
    term's used positions), g = d loss / d out, g0 = d loss / d the network's own output))."""
    model.zero_grad()
    dtype = next(model.parameters()).dtype
    h = torch.tensor(hr, dtype=dtype)
    wet = bool(np.isfinite(hr).all())
    lr = lt.ro.downsample(h, scale)
    out0 = model(lr if wet else lt.filled_lr(h, scale))
    out0.retain_grad()
    if consistent:
        import consistency_train_oracle as cto
        out = cto.layer(out0, lr, scale, "bicubic", "bicubic", int(consistent))
    else:
        out = out0 * 1.0
    out.retain_grad()
    pixel, _ = lt.masked_loss(out, h, loss_fn)
    z = torch.zeros((), dtype=dtype)
    total, spec, ssim_l, grad_l, nused = pixel, z, z, z, 0
    if spectral_cfg is not None:
        spec, _ = slo.loss_torch(out, h, int(spectral_cfg.get("window", 64)), int(spectral_cfg.get("stride", 32)),
                                 float(spectral_cfg.get("eps", slo.EPS)))
        total = total + float(spectral_cfg.get("weight", 1.0)) * spec
    if ssim_cfg is not None:
        ssim_l, _ = sl.loss_torch(out, h, ssim_cfg.get("data_range"))
        total = total + float(ssim_cfg.get("weight", 1.0)) * ssim_l
    if gradient_cfg is not None:
        grad_l, nused = loss_torch(out, h, float(gradient_cfg.get("eps", EPS)))
        total = total + float(gradient_cfg.get("weight", 1.0)) * grad_l
    total.backward()
    grads = {n.replace(".conv.", "."): p.grad.detach().clone() for n, p in model.named_parameters()}
    return (float(total.detach()), out.detach(), grads,
            dict(pixel_loss=float(pixel.detach()), spectral_loss=float(spec.detach()), ssim_loss=float(ssim_l.detach()),
                 gradient_loss=float(grad_l.detach()), nused=nused, g=out.grad.detach().numpy(),
                 g0=out0.grad.detach().numpy()))
