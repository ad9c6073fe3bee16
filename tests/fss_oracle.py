"""The fractions skill score's oracle: include/srmi.h's definition ("the fractions skill
score") restated in numpy with an integral image, every sum int64.  The device's tables are
held to it exactly."""
import numpy as np

MAX_T, MAX_N, MAX_SCALE = 8, 16, 255
DERIVED = ("f_pred", "f_truth", "bias", "target", "afss", "skilful_scale")


def check_scales(scales):
    s = [int(n) for n in scales]
    if not 1 <= len(s) <= MAX_N or any(n != m for n, m in zip(s, scales)):
        raise ValueError(f"scales {scales!r}: 1 .. {MAX_N} whole numbers")
    if any(n < 1 or n > MAX_SCALE or n % 2 == 0 for n in s) or any(b <= a for a, b in zip(s, s[1:])):
        raise ValueError(f"scales {scales!r}: odd, in 1 .. {MAX_SCALE}, strictly increasing")
    return s


def window_counts(ind, n):
    """ind [H, W] of 0 / 1 -> int64 [H, W]: the sum of ind over rows y - h .. y + h and columns
    x - h .. x + h clipped to the plane, h = (n - 1) / 2, by an integral image."""
    H, W = ind.shape
    h = (n - 1) // 2
    ii = np.zeros((H + 1, W + 1), dtype=np.int64)
    ii[1:, 1:] = ind.astype(np.int64).cumsum(0).cumsum(1)
    y0 = np.clip(np.arange(H) - h, 0, H)[:, None]
    y1 = np.clip(np.arange(H) + h + 1, 0, H)[:, None]
    x0 = np.clip(np.arange(W) - h, 0, W)[None, :]
    x1 = np.clip(np.arange(W) + h + 1, 0, W)[None, :]
    return ii[y1, x1] - ii[y0, x1] - ii[y1, x0] + ii[y0, x0]


def events(pred, truth, thresholds):
    """(used [C, H, W] bool, Ip, It [C, T, H, W] bool): one fp32 comparison per field."""
    pred, truth = np.asarray(pred, dtype=np.float32), np.asarray(truth, dtype=np.float32)
    thr = np.asarray(thresholds, dtype=np.float32)
    if thr.ndim == 1:
        thr = np.tile(thr[None], (pred.shape[0], 1))
    used = np.isfinite(pred) & np.isfinite(truth)
    with np.errstate(invalid="ignore"):
        ip = used[:, None] & (pred[:, None] >= thr[:, :, None, None])
        it = used[:, None] & (truth[:, None] >= thr[:, :, None, None])
    return used, ip, it


def fss(pred, truth, thresholds, scales):
    """pred, truth [C, H, W]; thresholds [C, T] (or [T], the same for every channel); scales a
    sequence of odd n -> dict of 'num', 'den' [C, T, N] int64, 'events_pred', 'events_truth' [C,
    T] int64, 'used' [C] int64, 'fss' [C, T, N] fp64 and the DERIVED entries [C, T] fp64."""
    pred = np.asarray(pred, dtype=np.float32)
    Cn = pred.shape[0]
    thr = np.asarray(thresholds, dtype=np.float32)
    if thr.ndim == 1:
        thr = np.tile(thr[None], (Cn, 1))
    if thr.ndim != 2 or thr.shape[0] != Cn or not 1 <= thr.shape[1] <= MAX_T:
        raise ValueError(f"thresholds {thr.shape}: [C, T] with T in 1 .. {MAX_T}")
    scales = check_scales(scales)
    T, N = thr.shape[1], len(scales)
    used, ip, it = events(pred, truth, thr)
    num = np.zeros((Cn, T, N), dtype=np.int64)
    den = np.zeros((Cn, T, N), dtype=np.int64)
    for c in range(Cn):
        for t in range(T):
            for k, n in enumerate(scales):
                sp, st = window_counts(ip[c, t], n), window_counts(it[c, t], n)
                num[c, t, k] = ((sp - st) ** 2).sum()
                den[c, t, k] = (sp ** 2 + st ** 2).sum()
    res = dict(num=num, den=den, events_pred=ip.sum((2, 3)).astype(np.int64),
               events_truth=it.sum((2, 3)).astype(np.int64), used=used.sum((1, 2)).astype(np.int64))
    res.update(derive(num, den, res["events_pred"], res["events_truth"], res["used"], scales))
    return res


def derive(num, den, ep, et, used, scales):
    """The fp64 values srmi_fss forms from the integer tables."""
    sc = np.asarray(scales, dtype=np.float64)
    ep, et, nu = ep.astype(np.float64), et.astype(np.float64), used.astype(np.float64)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(den == 0, np.nan, 1.0 - num.astype(np.float64) / den.astype(np.float64))
        f_pred, f_truth, bias = ep / nu, et / nu, ep / et
        target = 0.5 + f_truth / 2.0
        afss = 2.0 * ep * et / (ep * ep + et * et)
        ok = f >= target[..., None]
    skilful = np.where(ok.any(-1), sc[np.argmax(ok, -1)], np.nan)
    out = dict(fss=f, f_pred=f_pred, f_truth=f_truth, bias=bias, target=target, afss=afss, skilful_scale=skilful)
    empty = used == 0
    for v in out.values():
        v[empty] = np.nan
    return out


def contingency(pred, truth, thresholds):
    """hits, misses, false alarms [C, T] int64 of the same event."""
    _, ip, it = events(pred, truth, np.asarray(thresholds, dtype=np.float32))
    return ((ip & it).sum((2, 3)).astype(np.int64), (~ip & it).sum((2, 3)).astype(np.int64),
            (ip & ~it).sum((2, 3)).astype(np.int64))
