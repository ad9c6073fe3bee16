"""numpy restatement of empirical quantile mapping (srmi_quantile_map_accumulate / _fit /
_apply, srmi.quantile_map.QuantileMap).  The reference has no counterpart, so this oracle is
the definition (include/srmi.h, "quantile mapping") written the obvious way.

accumulate is integer work on the distribution score's own bin (distribution_oracle.bin_index);
fit is an integer search per knot and one fp64 interpolation; apply is fp32 with every
operation rounded on its own, which numpy does by construction.  The device is held to the
tables and to the mapped field bit for bit, and to the fp64 knots within a few roundings.
"""
import numpy as np

from distribution_oracle import bin_index, scale_of


def ranges_of(value_range, C):
    """one (lo, hi) pair or one per channel -> fp32 [C, 2]"""
    r = np.asarray(value_range, dtype=np.float32)
    if r.shape == (2,):
        r = np.tile(r, (C, 1))
    assert r.shape == (C, 2) and np.isfinite(r).all() and (r[:, 1] > r[:, 0]).all()
    with np.errstate(over="ignore"):
        assert np.isfinite(r[:, 1] - r[:, 0]).all()  # the scale's divisor, in fp32
    return r


def edges(lo, hi, bins: int) -> np.ndarray:
    """edge[j] = lo + (j - 1) w for j = 0 .. B + 2 in fp64, edge[B + 1] = hi exactly."""
    lo, hi = np.float64(np.float32(lo)), np.float64(np.float32(hi))
    w = (hi - lo) / np.float64(bins)
    e = lo + np.arange(-1, bins + 2, dtype=np.float64) * w
    e[bins + 1] = hi
    return e


def accumulate(src, truth, base, bins: int, value_range, hist=None, count=None):
    """src, truth, base (or None) [C, H, W] fp32 -> (hist [C, 2, B + 2], count [C]) int64, added
    to the given tables when there are any."""
    a, b = np.asarray(src, dtype=np.float32), np.asarray(truth, dtype=np.float32)
    assert a.shape == b.shape and a.ndim == 3
    Cn, B = a.shape[0], int(bins)
    rg = ranges_of(value_range, Cn)
    with np.errstate(invalid="ignore", over="ignore"):
        if base is not None:
            z = np.asarray(base, dtype=np.float32)
            a, b = a - z, b - z  # one fp32 subtraction each
    assert a.dtype == np.float32 and b.dtype == np.float32
    h = np.zeros((Cn, 2, B + 2), dtype=np.int64)
    n = np.zeros(Cn, dtype=np.int64)
    for c in range(Cn):
        used = np.isfinite(a[c]) & np.isfinite(b[c])
        n[c] = int(used.sum())
        if n[c]:
            h[c, 0] = np.bincount(bin_index(a[c][used], rg[c, 0], rg[c, 1], B), minlength=B + 2)
            h[c, 1] = np.bincount(bin_index(b[c][used], rg[c, 0], rg[c, 1], B), minlength=B + 2)
    if hist is not None:
        h, n = h + np.asarray(hist, dtype=np.int64), n + np.asarray(count, dtype=np.int64)
    return h, n


def fit_channel(ha, hb, lo, hi, bins: int, tail_count: int = 0) -> np.ndarray:
    """The knots T [B + 3] fp64 of one channel from its two int64 tables [B + 2]."""
    ha, hb = np.asarray(ha, dtype=np.int64), np.asarray(hb, dtype=np.int64)
    B, M = int(bins), int(bins) + 2
    assert ha.shape == (M,) and hb.shape == (M,) and (ha >= 0).all() and (hb >= 0).all()
    ca = np.concatenate([[0], np.cumsum(ha)]).astype(np.int64)
    cb = np.concatenate([[0], np.cumsum(hb)]).astype(np.int64)
    N = int(ca[M])
    assert int(cb[M]) == N
    e = edges(lo, hi, B)
    if N == 0:
        return e.copy()
    w = (np.float64(np.float32(hi)) - np.float64(np.float32(lo))) / np.float64(B)
    T = np.empty(M + 1, dtype=np.float64)
    for j in range(M + 1):
        a = int(ca[j])
        k0 = int(np.searchsorted(cb, a, side="left"))  # the smallest k with cb[k] >= a
        if int(cb[k0]) != a:  # cb[k0 - 1] < a < cb[k0]
            k = k0 - 1
            T[j] = e[k] + w * np.float64(a - int(cb[k])) / np.float64(int(cb[k0]) - int(cb[k]))
        else:
            k1 = int(np.searchsorted(cb, a, side="right")) - 1  # the largest k with cb[k] <= a
            left = -np.inf if a == 0 else e[k0]
            right = np.inf if a == N else e[k1]
            T[j] = min(max(e[j], left), right)
    t = int(tail_count)
    assert t >= 0
    trusted = np.nonzero((ca >= t) & (N - ca >= t))[0]
    if trusted.size == 0:
        return e.copy()
    j0, j1 = int(trusted[0]), int(trusted[-1])
    out = T.copy()
    out[:j0] = e[:j0] + (T[j0] - e[j0])
    out[j1 + 1:] = e[j1 + 1:] + (T[j1] - e[j1])
    return out


def fit(hist, bins: int, value_range, tail_count: int = 0):
    """hist [C, 2, B + 2] -> (knots [C, B + 3] fp64, table fp32, meta [C, 4] fp32)"""
    hist = np.asarray(hist, dtype=np.int64)
    Cn, B = hist.shape[0], int(bins)
    rg = ranges_of(value_range, Cn)
    knots = np.stack([fit_channel(hist[c, 0], hist[c, 1], rg[c, 0], rg[c, 1], B, tail_count) for c in range(Cn)])
    return knots, knots.astype(np.float32), meta_of(knots, rg, B)


def meta_of(knots, rg, bins: int) -> np.ndarray:
    meta = np.empty((knots.shape[0], 4), dtype=np.float32)
    for c in range(knots.shape[0]):
        e = edges(rg[c, 0], rg[c, 1], bins)
        meta[c] = rg[c, 0], rg[c, 1], np.float32(knots[c, 0] - e[0]), np.float32(knots[c, -1] - e[-1])
    return meta


def apply(x, base, table, meta, bins: int, strength=1.0) -> np.ndarray:
    """x, base (or None) [C, H, W] fp32, table [C, B + 3] fp32, meta [C, 4] fp32 -> out fp32, each
    operation an fp32 one rounded on its own."""
    x = np.asarray(x, dtype=np.float32)
    table, meta = np.asarray(table, dtype=np.float32), np.asarray(meta, dtype=np.float32)
    B, M = int(bins), int(bins) + 2
    s = np.float32(strength)
    out = np.empty_like(x)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(x.shape[0]):
            lo, hi, slo, shi = meta[c]
            scale = scale_of(lo, hi, B)
            xc = x[c]
            v = xc - np.asarray(base[c], dtype=np.float32) if base is not None else xc
            u = (v - lo) * scale + np.float32(1.0)
            assert v.dtype == np.float32 and u.dtype == np.float32
            mid = ~np.isnan(v) & ~(u < 0) & ~(u >= np.float32(M))
            k = np.minimum(np.where(mid, u, np.float32(0.0)).astype(np.int64), M - 1)
            f = u - k.astype(np.float32)
            t = table[c]
            y = t[k] + f * (t[k + 1] - t[k])
            o = xc + s * (y - v)
            o = np.where(u < 0, xc + s * slo, o)
            o = np.where(u >= np.float32(M), xc + s * shi, o)
            assert o.dtype == np.float32
            ob = o.view(np.int32).copy()
            nanv = np.isnan(v)
            ob[nanv] = xc.view(np.int32)[nanv]  # the same bits
            out[c] = ob.view(np.float32)
    return out


def w1_samples(a, b) -> float:
    """Wasserstein-1 distance of two equally large samples: the mean gap of the sorted values,
    fp64."""
    a, b = np.sort(np.asarray(a, dtype=np.float64).ravel()), np.sort(np.asarray(b, dtype=np.float64).ravel())
    assert a.size == b.size
    return float(np.abs(a - b).mean())
