"""The ensemble score's oracle: include/srmi.h's definition ("the ensemble score") restated in
numpy.  ``pixel_terms`` follows the header's fp64 order operation by operation (numpy's float64
elementwise operations round each once, as the device does), so the per-pixel values, the
tables and the CRPS map are held to it exactly; ``sums`` adds with math.fsum, the correctly
rounded sum, which the device's fixed-order sums are held to within the a-priori bound of any
summation order; ``derive`` is the finish launch's stated order, applied to whatever sums and
tables it is given."""
import math

import numpy as np

MIN_K, MAX_K, MAX_B = 2, 8, 16
SUMS = ("crps", "crps_fair", "a", "b", "var", "e2", "abs_e", "s", "s_abs_e")
DERIVED = ("crps", "crps_fair", "rmse_mean", "spread_rms", "ssr", "spread_error_corr", "outliers",
           "outliers_expected", "reliability_index")


def tree(t):
    """t[0] + .. + t[K - 1] added pairwise in ascending j: ((t0 + t1) + (t2 + t3)) + ((t4 + t5)
    + (t6 + t7)) with the terms j >= K left out, in the dtype of the terms."""
    K = len(t)
    s01 = t[0] + t[1] if K > 1 else t[0]
    s23 = (t[2] + t[3] if K > 3 else t[2]) if K > 2 else None
    s45 = (t[4] + t[5] if K > 5 else t[4]) if K > 4 else None
    s67 = (t[6] + t[7] if K > 7 else t[6]) if K > 6 else None
    s03 = s01 + s23 if K > 2 else s01
    s47 = (s45 + s67 if K > 6 else s45) if K > 4 else None
    return s03 + s47 if K > 4 else s03


def check_edges(edges, Cn):
    e = np.asarray(edges, dtype=np.float32)
    if e.ndim == 1:
        e = np.tile(e[None], (Cn, 1))
    if e.ndim != 2 or e.shape[0] != Cn or e.shape[1] > MAX_B - 1:
        raise ValueError(f"edges {e.shape}: [C, B - 1] with B in 1 .. {MAX_B}")
    return e


def pixel_terms(members, truth, edges=()):
    """members [K, C, H, W], truth [C, H, W] fp32; edges [C, B - 1] (or [B - 1]) -> dict of [C,
    H, W] arrays: 'used' bool; 'a', 'b', 'crps', 'crps_fair', 'mean', 'var', 'e', 's' fp64;
    'rank', 'bin' int64; 'tied' bool.  Where a pixel is not used the fp64 values are NaN and
    the integers 0."""
    m32, y32 = np.asarray(members, dtype=np.float32), np.asarray(truth, dtype=np.float32)
    K, Cn = m32.shape[0], m32.shape[1]
    if not MIN_K <= K <= MAX_K or y32.shape != m32.shape[1:]:
        raise ValueError(f"members {m32.shape}, truth {y32.shape}")
    ed = check_edges(edges, Cn)
    used = np.isfinite(y32) & np.isfinite(m32).all(0)
    m = np.where(used[None], m32, np.float32(0)).astype(np.float64)
    y = np.where(used, y32, np.float32(0)).astype(np.float64)
    dK = np.float64(K)
    a = tree([np.abs(m[j] - y) for j in range(K)])
    b = np.zeros_like(y)
    for j in range(K):
        for l in range(j + 1, K):
            b = b + np.abs(m[j] - m[l])
    aK = a / dK
    crps = aK - b / np.float64(K * K)
    fair = aK - b / np.float64(K * (K - 1))
    mean = tree([m[j] for j in range(K)]) / dK
    dev = [m[j] - mean for j in range(K)]
    var = tree([d * d for d in dev]) / dK
    e = mean - y
    s = np.sqrt(var)
    with np.errstate(invalid="ignore"):
        rank = sum(((m32[j] < y32) & used).astype(np.int64) for j in range(K))
        tied = np.any(m32 == y32[None], axis=0) & used
        sf = s.astype(np.float32)
        bins = sum(((sf >= ed[:, i, None, None]) & used).astype(np.int64) for i in range(ed.shape[1])) \
            if ed.shape[1] else np.zeros(y.shape, dtype=np.int64)
    out = dict(a=a, b=b, crps=crps, crps_fair=fair, mean=mean, var=var, e=e, s=s)
    out = {k: np.where(used, v, np.nan) for k, v in out.items()}
    out.update(used=used, rank=rank, tied=tied, bin=bins)
    return out


def crps_map(terms):
    """[C, H, W] fp32: (float)crps, NaN where the pixel is not used."""
    return terms["crps"].astype(np.float32)


def tables(terms, K, B):
    """The integer tables, int64: 'used' [C], 'rank_hist' [C, K + 1], 'tied' [C], 'bin_count'
    [C, B]."""
    used = terms["used"]
    Cn = used.shape[0]
    hist = np.zeros((Cn, K + 1), dtype=np.int64)
    cnt = np.zeros((Cn, B), dtype=np.int64)
    for c in range(Cn):
        hist[c] = np.bincount(terms["rank"][c][used[c]], minlength=K + 1)
        cnt[c] = np.bincount(terms["bin"][c][used[c]], minlength=B)
    return dict(used=used.sum((1, 2)).astype(np.int64), rank_hist=hist,
                tied=terms["tied"].sum((1, 2)).astype(np.int64), bin_count=cnt)


def sum_terms(terms, B):
    """Per channel the list of the 9 + 2 B term arrays (used pixels only) that ``sums`` adds:
    SUMS, then per bin var and e^2."""
    used = terms["used"]
    out = []
    for c in range(used.shape[0]):
        u = used[c]
        s, e, var = terms["s"][c][u], terms["e"][c][u], terms["var"][c][u]
        ae, e2 = np.abs(e), e * e
        cols = [terms["crps"][c][u], terms["crps_fair"][c][u], terms["a"][c][u], terms["b"][c][u], var, e2, ae, s,
                s * ae]
        bn = terms["bin"][c][u]
        for b in range(B):
            cols += [var[bn == b], e2[bn == b]]
        out.append(cols)
    return out


def sums(terms, B):
    """[C, 9 + 2 B] fp64: math.fsum of every column of sum_terms."""
    return np.array([[math.fsum(col.tolist()) for col in cols] for cols in sum_terms(terms, B)], dtype=np.float64)


def derive(sums_, tabs, K):
    """The fp64 values the finish launch forms from the sums [C, 9 + 2 B] and the tables, in its
    stated order: dict of DERIVED [C] and 'bin_spread', 'bin_rmse' [C, B]."""
    S = np.asarray(sums_, dtype=np.float64)
    B = (S.shape[1] - len(SUMS)) // 2
    n = tabs["used"].astype(np.float64)
    hist = tabs["rank_hist"].astype(np.float64)
    nb = tabs["bin_count"].astype(np.float64)
    f = np.float64(K + 1) / np.float64(K - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        mse, mvar = S[:, 5] / n, S[:, 4] / n
        rmse = np.sqrt(mse)
        out = dict(crps=S[:, 0] / n, crps_fair=S[:, 1] / n, rmse_mean=rmse, spread_rms=np.sqrt(mvar),
                   ssr=np.sqrt(f * mvar) / rmse)
        ms, ma = S[:, 7] / n, S[:, 6] / n
        cov = S[:, 8] / n - ms * ma
        vs, va = mvar - ms * ms, mse - ma * ma
        out["spread_error_corr"] = cov / np.sqrt(vs * va)
        out["outliers"] = (tabs["rank_hist"][:, 0] + tabs["rank_hist"][:, K]).astype(np.float64) / n
        out["outliers_expected"] = np.full(n.shape, np.float64(2.0) / np.float64(K + 1))
        u = np.float64(1.0) / np.float64(K + 1)
        ri = np.zeros_like(n)
        for r in range(K + 1):
            ri = ri + np.abs(hist[:, r] / n[:] - u)
        out["reliability_index"] = ri
        out["bin_spread"] = np.sqrt(f * (S[:, len(SUMS)::2] / nb))
        out["bin_rmse"] = np.sqrt(S[:, len(SUMS) + 1::2] / nb)
    empty = tabs["used"] == 0
    for v in out.values():
        v[empty] = np.nan
    return out


def score(members, truth, edges=()):
    """Everything at once: the tables, 'sums', the derived values and 'crps_map'."""
    m = np.asarray(members, dtype=np.float32)
    K, Cn = m.shape[0], m.shape[1]
    B = check_edges(edges, Cn).shape[1] + 1
    terms = pixel_terms(m, truth, edges)
    tabs = tables(terms, K, B)
    S = sums(terms, B)
    out = dict(tabs, sums=S, crps_map=crps_map(terms))
    out.update(derive(S, tabs, K))
    return out
