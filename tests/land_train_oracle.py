"""numpy / torch fp64 restatement of training on tiles with land (srmi_tiles_dry,
srmi_batch_prep_masked, srmi_tile_loss_parts_masked / srmi_loss_from_parts_masked,
srmi_loss_dy_masked, FusedTrainer(land=True)), written the slow, obvious way on top of
land_oracle and oracle.rcan_oracle.  The reference has no counterpart: it never trains on
a tile that touches land.

NaN in the HR tile is the mask ("wet" = finite).  A train step: downsample the HR batch
(NaN propagates: an LR pixel is dry iff one of its taps is), fill every LR plane with
land_oracle.fill, run the model on the filled LR, take the loss over the elements where
prediction and target are both finite, backward."""
import numpy as np
import torch

import land_oracle as lo
from oracle import rcan_oracle as ro

LNORM, LSCALE, AFFINE = lo.LNORM, lo.LSCALE, lo.AFFINE
CHARBONNIER_EPS = 1e-6


# ------------------------------------------------------------------ the shared fixture
def land_mask(T: int, k: int) -> np.ndarray:
    """[T, T] bool, True = dry, of tile k >= 1: a sinusoidal coast xx > 0.55 T + 0.2 T
    sin(7 yy / T) (transposed and reversed on even tiles), a 5 x 5 lake inside the land,
    one dry pixel in the open sea, a 9 x 17 island."""
    yy, xx = np.mgrid[0:T, 0:T]
    dry = xx > 0.55 * T + 0.2 * T * np.sin(7.0 * yy / T)
    y0, x0 = T // 8, T - 6  # inside the land: the coast stays left of 0.75 T (T >= 32)
    assert dry[y0:y0 + 5, x0:x0 + 5].all()
    dry[y0:y0 + 5, x0:x0 + 5] = False  # the lake
    assert not dry[T // 2, T // 8]
    dry[T // 2, T // 8] = True  # the dry pixel in the open sea
    iy, ix = (3 * T) // 4 - min(9, T // 4) // 2, T // 4 - min(17, T // 4) // 2
    dry[iy:iy + min(9, T // 4), ix:ix + min(17, T // 4)] = True  # the island
    if k % 2 == 0:
        dry = dry.T[::-1, ::-1].copy()
    return dry


def land_batch(B: int, C: int, T: int, seed: int) -> np.ndarray:
    """ro.synthetic_hr(B, C, T, seed) with land (NaN, the same mask in every channel) in
    every tile but tile 0, which stays all wet."""
    hr = ro.synthetic_hr(B, C, T, seed).copy()
    for k in range(1, B):
        hr[k, :, land_mask(T, k)] = np.nan
    return hr


def check_conditions(hr: np.ndarray, scale: int) -> None:
    """What every comparison needs of its input: each tile's LR planes keep a finite
    pixel (the fill has something to start from), and no wet plane is constant."""
    dry = lr_dry(~np.isfinite(hr), scale)
    assert (~dry).any(axis=(2, 3)).all(), "an LR plane without a finite pixel"
    for b in range(hr.shape[0]):
        for c in range(hr.shape[1]):
            w = hr[b, c][np.isfinite(hr[b, c])]
            assert w.size >= 2 and w.max() > w.min(), f"constant wet plane: tile {b} channel {c}"


# ------------------------------------------------------------------------ the keep flags
def keep_flags(region: np.ndarray, ty: int, tx: int, min_wet: int):
    """region [C, H, W] -> (bad [C, gy*gx] int32: the same flag in every channel's row,
    1 iff some channel of the tile has fewer than min_wet finite pixels; nwet [C, gy*gx])."""
    C, H, W = region.shape
    gy, gx = H // ty, W // tx
    nwet = np.zeros((C, gy * gx), np.int32)
    for c in range(C):
        for t in range(gy * gx):
            y0, x0 = (t // gx) * ty, (t % gx) * tx
            nwet[c, t] = np.isfinite(region[c, y0:y0 + ty, x0:x0 + tx]).sum()
    bad = (nwet < min_wet).any(axis=0).astype(np.int32)
    return np.broadcast_to(bad, (C, gy * gx)).copy(), nwet


def get_tiles(region: np.ndarray, ty: int, tx: int, min_wet: int):
    """srmi.llc.get_tiles with the threshold -> (tiles [n, C, ty, tx], ids [n])."""
    C, H, W = region.shape
    gy, gx = H // ty, W // tx
    bad, _ = keep_flags(region, ty, tx, min_wet)
    keep = np.flatnonzero(bad.ravel() == 0)
    n = keep.size // C
    planes = []
    for j in keep[:n * C]:
        c, t = divmod(int(j), gy * gx)
        y0, x0 = (t // gx) * ty, (t % gx) * tx
        planes.append(region[c, y0:y0 + ty, x0:x0 + tx])
    return np.array(planes, region.dtype).reshape(n, C, ty, tx), keep[:n]


# ------------------------------------------------------------------------- masked prep
def flip(x: np.ndarray, f: int) -> np.ndarray:
    """xyflip (batch.py:37-49) of [..., T, T]: bit 0 flips x, bit 1 flips y, bit 2 swaps."""
    if f & 1:
        x = x[..., :, ::-1]
    if f & 2:
        x = x[..., ::-1, :]
    if f & 4:
        x = np.swapaxes(x, -1, -2)
    return x


def prep(raw: np.ndarray, mode: int, flip_index: int, off=None, div=None):
    """raw [B, C, T, T] (the dtype it is given; the tests hand in float64) -> (hr: the
    statistics over each plane's wet pixels, normalised, flipped, NaN kept; off [B, C];
    div [B, C]; nwet [B, C])."""
    B, C = raw.shape[:2]
    wet = np.isfinite(raw)
    o = np.full((B, C), np.nan, raw.dtype)
    d = np.full((B, C), np.nan, raw.dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        for b in range(B):
            for c in range(C):
                w = raw[b, c][wet[b, c]]
                if mode == AFFINE:
                    o[b, c], d[b, c] = off[b, c], div[b, c]
                elif w.size:
                    if mode == LNORM:
                        o[b, c] = w.mean()
                        d[b, c] = np.sqrt(((w - o[b, c]) ** 2).mean())
                    else:
                        o[b, c], d[b, c] = w.min(), w.max() - w.min()
        hr = np.where(wet, (raw - o[:, :, None, None]) / d[:, :, None, None], np.nan)
    return np.ascontiguousarray(flip(hr, flip_index)), o, d, wet.sum(axis=(2, 3)).astype(np.int32)


# ------------------------------------------------------------------------- the LR side
def lr_dry(dry_hr: np.ndarray, scale: int) -> np.ndarray:
    """[..., T, T] bool -> [..., T/s, T/s]: an LR pixel is dry iff any (clamped) tap of its
    4 x 4 window at y s + s/2 - 2 is."""
    T = dry_hr.shape[-1]
    t = T // scale
    out = np.zeros(dry_hr.shape[:-2] + (t, t), bool)
    for y in range(t):
        ys = np.clip(np.arange(4) + y * scale + scale // 2 - 2, 0, T - 1)
        for x in range(t):
            xs = np.clip(np.arange(4) + x * scale + scale // 2 - 2, 0, T - 1)
            out[..., y, x] = dry_hr[..., ys[:, None], xs[None, :]].any(axis=(-1, -2))
    return out


def filled_lr(hr: torch.Tensor, scale: int) -> torch.Tensor:
    """downsample (NaN propagates) -> land_oracle.fill per plane, in hr's dtype; a
    constant of the graph (the fill is not differentiated: hr is data)."""
    lr = ro.downsample(hr.detach(), scale).numpy()
    out = np.empty_like(lr)
    for b in range(lr.shape[0]):
        for c in range(lr.shape[1]):
            out[b, c] = lo.fill(lr[b, c], np.isfinite(lr[b, c]), lr.dtype)[0]
    return torch.from_numpy(out)


# ------------------------------------------------------------------------- masked loss
def masked_loss(pred: torch.Tensor, target: torch.Tensor, loss_fn: str = "l2"):
    """(single_product_loss over the elements where both are finite, their count)."""
    both = torch.isfinite(pred) & torch.isfinite(target)
    d = pred[both] - target[both]
    if loss_fn == "l2":
        return torch.sqrt((d ** 2).mean()), int(both.sum())
    if loss_fn == "charbonnier":
        return torch.mean(torch.sqrt(d ** 2 + CHARBONNIER_EPS)), int(both.sum())
    raise Exception("Unknown single-product loss function {}".format(loss_fn))


def masked_dy(pred: np.ndarray, target: np.ndarray, loss_fn: str = "l2") -> np.ndarray:
    """d loss / d pred in closed form, 0 where either is not finite.  RMSE: (p - t) /
    (count L); Charbonnier: d / sqrt(d^2 + eps) / count."""
    p, t = np.asarray(pred, np.float64), np.asarray(target, np.float64)
    both = np.isfinite(p) & np.isfinite(t)
    n = both.sum()
    d = np.where(both, p - np.where(both, t, 0), 0.0)
    if loss_fn == "l2":
        return d / (n * np.sqrt((d ** 2).sum() / n))
    return np.where(both, d / np.sqrt(d ** 2 + CHARBONNIER_EPS) / n, 0.0)


# ---------------------------------------------------------------------- the train step
def train_step(model, hr: np.ndarray, scale: int, loss_fn: str = "l2"):
    """One masked step of `model` (its dtype) on hr [B, C, T, T] with NaN on land ->
    (loss, out, {reference key: gradient})."""
    model.zero_grad()
    dtype = next(model.parameters()).dtype
    h = torch.tensor(hr, dtype=dtype)
    out = model(filled_lr(h, scale))
    loss, _ = masked_loss(out, h, loss_fn)
    loss.backward()
    grads = {n.replace(".conv.", "."): p.grad.detach().clone() for n, p in model.named_parameters()}
    return float(loss), out.detach(), grads


def interp_loss(hr: np.ndarray, scale: int, loss_fn: str = "l2") -> float:
    """The interp-baseline metric: loss(target, upsample(filled LR)) over the wet target."""
    h = torch.tensor(hr, dtype=torch.float64)
    return float(masked_loss(h, ro.upsample(filled_lr(h, scale), scale), loss_fn)[0])
