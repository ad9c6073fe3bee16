"""numpy / torch restatement of the SSIM loss term (srmi_ssim_loss_*, srmi.ssim.SSIMLoss,
FusedTrainer(ssim=...)), written the obvious way on top of ssim_oracle.  The reference has no
counterpart, so this file is the definition (include/srmi.h, "the SSIM loss term").

a (prediction) and b (target) are [..., H, W]; every leading index is a plane.  Per plane
everything of ssim_oracle holds: the 11 fp32 taps g, G = g (x) g, valid positions only, a
position USED iff its 121 pixels are finite in a and in b, lo / hi the min / max of b's finite
pixels, L = hi - lo or data_range where data_range > 0, the pivot r = 0.5 lo + 0.5 hi (b's,
always), C1 = (0.01 L)^2, C2 = (0.03 L)^2.  A plane without a finite target pixel, or whose L
is 0 or not finite, contributes no position.  With a' = a - r, b' = b - r (0 where a pixel is
not finite in both):

    m_a = G * a', m_b = G * b', s_aa = G * a'^2 - m_a^2, s_bb likewise, s_ab = G * (a' b') - m_a m_b
    mu_a = m_a + r, mu_b = m_b + r
    D_l = mu_a^2 + mu_b^2 + C1, l = (2 mu_a mu_b + C1) / D_l
    D_c = s_aa + s_bb + C2,     cs = (2 s_ab + C2) / D_c,     ssim = l cs

S = the sum of ssim over the used positions of ALL planes, Nused their number, L_ssim = 1 - S /
Nused (0, with a zero gradient, when Nused = 0): a mean over positions, not over per-plane means.

Gradient (L and r depend on the target only).  At a used position B = -2 l cs / D_c, C = 2 l /
D_c, A = 2 cs (mu_b - mu_a l) / D_l - B m_a - C m_b; A = B = C = 0 elsewhere;

    dS / da (q) = (G^T * A)(q) + a'(q) (G^T * B)(q) + b'(q) (G^T * C)(q)

with G^T * the zero-extended ("full") correlation of an [H - 10][W - 10] map back onto [H][W],
and d L_ssim / da = -dS / da / Nused.  A pixel that is not finite in both a and b takes no
gradient (the device does not write it).

``dtype=np.float64`` is the definition.  ``dtype=np.float32`` does the same arithmetic in single
precision (ssim_oracle's fp32 forward, then the coefficients, the separable correlations and
the combination in fp32): the fp32 arithmetic from which the device tests take their bars.  The
sums over positions are fp64 in both."""
import numpy as np
import torch
import torch.nn.functional as F

import land_train_oracle as lt
import spectral_loss_oracle as slo
import ssim_oracle as so

R = so.RADIUS


def plane_ok(r, L) -> bool:
    """A plane contributes positions iff its target has a finite pixel and a range that is
    finite and not 0."""
    return bool(np.isfinite(r) and np.isfinite(L) and L > 0)


def plane_range(b_plane: np.ndarray, data_range=None):
    """(r, L) of one target plane in ITS dtype (fp32 for the device's inputs), as ssim_oracle
    forms them."""
    r, L, _, _ = so.pivot_and_range(b_plane)
    if data_range is not None and data_range > 0:
        L = b_plane.dtype.type(data_range)
    return r, L


def full_correlation(M: np.ndarray, g: np.ndarray) -> np.ndarray:
    """M [Hv, Wv] -> [Hv + 10, Wv + 10]: out(q) = sum_k sum_l g[k] g[l] M(qy - k, qx - l), M
    zero outside; separable, in M's dtype."""
    P = np.zeros((M.shape[0] + 4 * R, M.shape[1] + 4 * R), dtype=M.dtype)
    P[2 * R:2 * R + M.shape[0], 2 * R:2 * R + M.shape[1]] = M
    return so._valid(P, g[::-1].copy())


def plane_terms(a: np.ndarray, b: np.ndarray, data_range=None, dtype=np.float64) -> dict:
    """One plane a, b [H, W] -> dict(used [Hv, Wv] bool, ssim [Hv, Wv] (dtype; garbage where
    not used), A, B, C [Hv, Wv] (0 where not used), pa, pb [H, W], fin [H, W], r, L)."""
    dt = np.dtype(dtype).type
    g = so.taps().astype(dt)
    r, L = plane_range(b, data_range)
    fin = np.isfinite(a) & np.isfinite(b)
    used = so.window_bad_count(~fin) == 0
    if not plane_ok(r, L):
        used = np.zeros_like(used)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        pa = np.where(fin, a.astype(dt) - dt(r), dt(0))
        pb = np.where(fin, b.astype(dt) - dt(r), dt(0))
        ma, mb = so._valid(pa, g), so._valid(pb, g)
        saa = so._valid(pa * pa, g) - ma * ma
        sbb = so._valid(pb * pb, g) - mb * mb
        sab = so._valid(pa * pb, g) - ma * mb
        Ld = dt(L)
        C1, C2 = (dt(0.01) * Ld) ** 2, (dt(0.03) * Ld) ** 2
        Dc = saa + sbb + C2
        cs = (dt(2) * sab + C2) / Dc
        mua, mub = ma + dt(r), mb + dt(r)
        Dl = mua * mua + mub * mub + C1
        l = (dt(2) * mua * mub + C1) / Dl
        s = l * cs
        Bc = -dt(2) * s / Dc
        Cc = dt(2) * l / Dc
        Ac = dt(2) * cs * (mub - mua * l) / Dl - Bc * ma - Cc * mb
    z = dt(0)
    return dict(used=used, ssim=s, A=np.where(used, Ac, z), B=np.where(used, Bc, z), C=np.where(used, Cc, z), pa=pa,
                pb=pb, fin=fin, r=r, L=L)


def loss_and_grad(a: np.ndarray, b: np.ndarray, data_range=None, dtype=np.float64) -> dict:
    """a, b [..., H, W] -> dict(loss, grad [..., H, W] fp64 = d L_ssim / d a (0 where a pixel
    takes none), dS [..., H, W] (`dtype`: the unscaled dS / da), parts [...] fp64 = the planes'
    sums of ssim, counts [...] = their used positions, S, nused, ssim [..., Hv, Wv] (`dtype`,
    NaN where a position is not used), fin [..., H, W])."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.ndim < 2 or a.shape[-2] < so.NTAPS or a.shape[-1] < so.NTAPS:
        raise ValueError(f"fields {a.shape} / {b.shape}: two [..., H >= 11, W >= 11] arrays")
    if data_range is not None and not np.isfinite(data_range):
        raise ValueError(f"data_range {data_range!r}")
    dt = np.dtype(dtype).type
    lead, (H, W) = a.shape[:-2], a.shape[-2:]
    a3, b3 = a.reshape((-1, H, W)), b.reshape((-1, H, W))
    n = a3.shape[0]
    g = so.taps().astype(dt)
    parts, counts = np.zeros(n), np.zeros(n)
    dS = np.zeros((n, H, W), dtype=dt)
    smap = np.full((n, H - 2 * R, W - 2 * R), np.nan, dtype=dt)
    fin = np.zeros((n, H, W), bool)
    for p in range(n):
        t = plane_terms(a3[p], b3[p], data_range, dtype)
        used = t["used"]
        parts[p] = t["ssim"][used].astype(np.float64).sum()
        counts[p] = used.sum()
        smap[p][used] = t["ssim"][used]
        fin[p] = t["fin"]
        d = full_correlation(t["A"], g) + t["pa"] * full_correlation(t["B"], g) + t["pb"] * full_correlation(t["C"], g)
        dS[p] = np.where(t["fin"], d, dt(0))
    nused = int(counts.sum())
    S = float(parts.sum())
    shape = lead + (H, W)
    res = dict(parts=parts.reshape(lead), counts=counts.reshape(lead), dS=dS.reshape(shape),
               ssim=smap.reshape(lead + smap.shape[1:]), fin=fin.reshape(shape), nused=nused)
    if nused == 0:
        res.update(loss=0.0, S=0.0, grad=np.zeros(shape))
        return res
    scale = dt(-1.0 / nused)
    res.update(loss=1.0 - S / nused, S=S, grad=(scale * dS).astype(np.float64).reshape(shape))
    return res


def loss_torch(p: torch.Tensor, t: torch.Tensor, data_range=None):
    """The same loss as a differentiable torch expression (a dense 11 x 11 window through
    F.conv2d, in p's dtype) -> (loss, nused); t, r, L and the choice of the used positions are
    data.  t is taken as fp32 for r and L, as the device's target is."""
    H, W = p.shape[-2:]
    p3 = p.reshape((-1, H, W))
    t_np = t.detach().numpy().reshape((-1, H, W))
    p_np = p.detach().numpy().reshape((-1, H, W))
    g = torch.tensor(so.taps().astype(np.float64), dtype=p.dtype)
    G = (g[:, None] * g[None, :])[None, None]
    total = torch.zeros((), dtype=p.dtype)
    nused = 0

    def win(x):
        return F.conv2d(x[None, None], G)[0, 0]
    for k in range(p3.shape[0]):
        b32 = t_np[k].astype(np.float32)
        r, L = plane_range(b32, data_range)
        if not plane_ok(r, L):
            continue
        fin_np = np.isfinite(p_np[k]) & np.isfinite(t_np[k])
        used = torch.from_numpy(so.window_bad_count(~fin_np) == 0)
        if not bool(used.any()):
            continue
        fin = torch.from_numpy(fin_np)
        zero = torch.zeros((), dtype=p.dtype)
        r, L = float(r), float(L)
        pa = torch.where(fin, p3[k] - r, zero)
        pb = torch.where(fin, torch.tensor(t_np[k], dtype=p.dtype) - r, zero)
        ma, mb = win(pa), win(pb)
        saa, sbb, sab = win(pa * pa) - ma * ma, win(pb * pb) - mb * mb, win(pa * pb) - ma * mb
        C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
        mua, mub = ma + r, mb + r
        s = (2 * mua * mub + C1) / (mua * mua + mub * mub + C1) * (2 * sab + C2) / (saa + sbb + C2)
        total = total + s[used].sum()
        nused += int(used.sum())
    if nused == 0:  # 0, with a zero gradient
        return torch.where(torch.isfinite(p3.detach()), p3, torch.zeros((), dtype=p.dtype)).sum() * 0.0, 0
    return 1.0 - total / nused, nused


def train_step(model, hr: np.ndarray, scale: int, loss_fn: str = "l2", ssim_cfg=None, spectral_cfg=None,
               consistent: int = 0, land: bool = False):
    """spectral_loss_oracle.train_step with the term: one step of `model` (its dtype) on hr [B,
    C, T, T] (NaN on land allowed) with loss = masked pixel loss (+ weight_spec * L_spec) +
    weight * L_ssim -> (total, out, {reference key: gradient}, dict(pixel_loss, spectral_loss,
    ssim_loss, nused (the SSIM term's used positions), g = d loss / d out, g0 = d loss / d the
    network's own output)).  consistent = K > 0 puts consistency_train_oracle's layer behind the
    model, as FusedTrainer(consistent=K) does; g and g0 are the same without it."""
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
    total, spec, ssim_l, nused = pixel, torch.zeros((), dtype=dtype), torch.zeros((), dtype=dtype), 0
    if spectral_cfg is not None:
        spec, _ = slo.loss_torch(out, h, int(spectral_cfg.get("window", 64)), int(spectral_cfg.get("stride", 32)),
                                 float(spectral_cfg.get("eps", slo.EPS)))
        total = total + float(spectral_cfg.get("weight", 1.0)) * spec
    if ssim_cfg is not None:
        ssim_l, nused = loss_torch(out, h, ssim_cfg.get("data_range"))
        total = total + float(ssim_cfg.get("weight", 1.0)) * ssim_l
    total.backward()
    grads = {n.replace(".conv.", "."): p.grad.detach().clone() for n, p in model.named_parameters()}
    return (float(total.detach()), out.detach(), grads,
            dict(pixel_loss=float(pixel.detach()), spectral_loss=float(spec.detach()), ssim_loss=float(ssim_l.detach()),
                 nused=nused, g=out.grad.detach().numpy(), g0=out0.grad.detach().numpy()))
