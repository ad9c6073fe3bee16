"""numpy restatement of the distribution score (srmi_distribution,
srmi.distribution.DistributionScore).  The reference has no counterpart, so this oracle is
the definition (include/srmi.h, "the distribution score") written the obvious way.

The bin of a value is formed in ``np.float32`` with exactly the operations of the
definition -- one subtraction and one division for the scale, one subtraction, one
multiplication and a truncation for the bin -- and everything else in int64 / fp64.  Nothing
here is approximate: the device is held to these tables bit for bit.
"""
import numpy as np

MAX_PROBS = 16
DEFAULT_PROBS = (0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99, 0.999)


def scale_of(lo, hi, n: int) -> np.float32:
    """fp32(n) / (hi - lo), each operation rounded once in fp32; 0 unless hi > lo."""
    lo, hi = np.float32(lo), np.float32(hi)
    if not hi > lo:
        return np.float32(0.0)
    return np.float32(np.float32(n) / np.float32(hi - lo))


def bin_index(x: np.ndarray, lo, hi, n: int) -> np.ndarray:
    """x fp32 (finite) -> int64 index into the n + 2 entries {under, n bins, over}."""
    x = np.asarray(x, dtype=np.float32)
    lo, hi = np.float32(lo), np.float32(hi)
    scale = scale_of(lo, hi, n)
    inside = (x >= lo) & (x <= hi)
    d = np.where(inside, x, lo).astype(np.float32) - lo  # fp32 subtraction
    assert d.dtype == np.float32
    t = d * scale  # fp32 multiplication
    assert t.dtype == np.float32
    k = 1 + np.minimum(t.astype(np.int64), n - 1)  # truncation, then the integer clamp
    k = np.where(x == hi, n, k)
    k = np.where(x < lo, 0, k)
    k = np.where(x > hi, n + 1, k)
    return k.astype(np.int64)


def bin_index_fp64(x: np.ndarray, lo, hi, n: int) -> np.ndarray:
    """The same bins from fp64 positions: the independent computation the CPU test compares
    with (np.histogram's own arithmetic)."""
    x = np.asarray(x, dtype=np.float64)
    lo, hi = float(lo), float(hi)
    t = (x - lo) * (n / (hi - lo)) if hi > lo else np.zeros_like(x)
    k = 1 + np.minimum(np.floor(np.clip(t, 0, n)).astype(np.int64), n - 1)
    k = np.where(x == hi, n, k)
    k = np.where(x < lo, 0, k)
    k = np.where(x > hi, n + 1, k)
    return k.astype(np.int64)


def derive(ha: np.ndarray, hb: np.ndarray, lo, hi, bins: int, probs=DEFAULT_PROBS):
    """The derived values of one channel from its two int64 tables [bins + 2]: (pss, w1,
    under, over, q_a [nprobs], q_b [nprobs]), fp64."""
    ha, hb = np.asarray(ha, dtype=np.int64), np.asarray(hb, dtype=np.int64)
    n = int(ha.sum())
    assert int(hb.sum()) == n
    probs = np.asarray(probs, dtype=np.float64).reshape(-1)
    if n == 0:
        nan = np.float64(np.nan)
        return nan, nan, nan, nan, np.full(len(probs), np.nan), np.full(len(probs), np.nan)
    lo, hi = np.float64(np.float32(lo)), np.float64(np.float32(hi))
    w = (hi - lo) / np.float64(bins)
    nd = np.float64(n)
    ca, cb = np.cumsum(ha), np.cumsum(hb)
    pss = np.float64(int(np.minimum(ha, hb).sum())) / nd
    w1 = w * np.float64(int(np.abs(ca - cb).sum())) / nd
    under, over = np.float64(ha[0]) / nd, np.float64(ha[bins + 1]) / nd

    def quantiles(h, c):
        out = np.empty(len(probs), dtype=np.float64)
        for i, p in enumerate(probs):
            r = np.float64(p) * nd
            k = int(np.searchsorted(c.astype(np.float64), r, side="left"))  # the smallest k with cum[k] >= r
            prev = np.float64(c[k - 1]) if k > 0 else np.float64(0.0)
            left = lo + np.float64(k - 1) * w
            out[i] = left + w * (r - prev) / np.float64(h[k])
        return out

    return pss, w1, under, over, quantiles(ha, ca), quantiles(hb, cb)


def distribution(pred: np.ndarray, truth: np.ndarray, bins: int = 256, joint: int = 32, probs=DEFAULT_PROBS,
                 value_range=None):
    """pred, truth [C, H, W] -> the dict of DistributionScore.measure as numpy arrays
    ('derived' [C, 4 + 2 nprobs] beside its named parts)."""
    a = np.asarray(pred, dtype=np.float32)
    b = np.asarray(truth, dtype=np.float32)
    assert a.shape == b.shape and a.ndim == 3
    assert 2 <= bins <= 4096 and 0 <= joint <= 64
    probs = np.asarray(probs, dtype=np.float64).reshape(-1)
    assert len(probs) <= MAX_PROBS and ((probs > 0) & (probs < 1)).all()
    Cn, B, J, P = a.shape[0], bins, joint, len(probs)
    hist = np.zeros((Cn, 2, B + 2), dtype=np.int64)
    jt = np.zeros((Cn, J, J), dtype=np.int64)
    rng = np.zeros((Cn, 2), dtype=np.float32)
    count = np.zeros(Cn, dtype=np.int64)
    derived = np.zeros((Cn, 4 + 2 * P), dtype=np.float64)
    for c in range(Cn):
        used = np.isfinite(a[c]) & np.isfinite(b[c])
        xa, xb = a[c][used], b[c][used]
        count[c] = xa.size
        if value_range is not None:
            lo, hi = np.float32(value_range[0]), np.float32(value_range[1])
            assert np.isfinite(lo) and np.isfinite(hi) and hi > lo
        elif xa.size:
            lo, hi = xb.min(), xb.max()
        else:
            lo = hi = np.float32(np.nan)
        rng[c] = lo, hi
        if xa.size:
            ka, kb = bin_index(xa, lo, hi, B), bin_index(xb, lo, hi, B)
            hist[c, 0] = np.bincount(ka, minlength=B + 2)
            hist[c, 1] = np.bincount(kb, minlength=B + 2)
            if J:
                ja = np.clip(bin_index(xa, lo, hi, J) - 1, 0, J - 1)
                jb = np.clip(bin_index(xb, lo, hi, J) - 1, 0, J - 1)
                jt[c] = np.bincount(ja * J + jb, minlength=J * J).reshape(J, J)
        pss, w1, under, over, qa, qb = derive(hist[c, 0], hist[c, 1], lo, hi, B, probs)
        derived[c, :4] = pss, w1, under, over
        derived[c, 4:4 + P] = qa
        derived[c, 4 + P:] = qb
    return {"hist_pred": hist[:, 0], "hist_truth": hist[:, 1], "joint": jt, "lo": rng[:, 0], "hi": rng[:, 1],
            "count": count, "pss": derived[:, 0], "w1": derived[:, 1], "under": derived[:, 2], "over": derived[:, 3],
            "q_pred": derived[:, 4:4 + P], "q_truth": derived[:, 4 + P:],
            "q_bias": derived[:, 4:4 + P] - derived[:, 4 + P:], "derived": derived}
