"""numpy restatement of the SSIM / PSNR score (srmi_ssim, srmi.ssim.SSIMScore).  The
reference has no counterpart, so this oracle is the definition (include/srmi.h, "the SSIM
score") written the obvious way: Wang, Bovik, Sheikh, Simoncelli 2004 in its Gaussian form,
the quantity of scikit-image's ``structural_similarity(gaussian_weights=True,
use_sample_covariance=False)``, on valid positions only.

``dtype=np.float64`` is the definition.  ``dtype=np.float32`` does the same arithmetic in
single precision -- the pivoted inputs, the taps, every product and every partial sum are
rounded to fp32; separable, the horizontal pass then the vertical one, taps in ascending
order -- and is the fp32 reference arithmetic from which the device tests take their bars.
The means over the used positions and the mean square error are fp64 sums in both.

The taps are fp32 values in both (normalised in fp64, then rounded: the definition's).
``round_taps=False`` keeps them fp64, which is what scipy's gaussian_filter uses: the CPU
tests use it to pin the formula against scipy to 1e-12.
"""
import numpy as np

RADIUS = 5
NTAPS = 2 * RADIUS + 1
SIGMA = 1.5


def taps(round_taps: bool = True) -> np.ndarray:
    """g[k] ~ exp(-(k - 5)^2 / (2 1.5^2)), sum 1 in fp64, then rounded to fp32 (returned as
    fp64 values when round_taps is False)."""
    k = np.arange(NTAPS, dtype=np.float64)
    g = np.exp(-((k - RADIUS) ** 2) / (2.0 * SIGMA * SIGMA))
    g /= g.sum()
    return g.astype(np.float32) if round_taps else g


def _valid(x: np.ndarray, g: np.ndarray) -> np.ndarray:
    """x [H, W] -> [H - 10, W - 10]: the separable window over the valid positions, in x's
    dtype (numpy rounds every product and every sum to it)."""
    H, W = x.shape
    h = np.zeros((H, W - 2 * RADIUS), dtype=x.dtype)
    for k in range(NTAPS):
        h = h + g[k] * x[:, k:k + W - 2 * RADIUS]
    v = np.zeros((H - 2 * RADIUS, W - 2 * RADIUS), dtype=x.dtype)
    for k in range(NTAPS):
        v = v + g[k] * h[k:k + H - 2 * RADIUS]
    return v


def window_bad_count(bad: np.ndarray) -> np.ndarray:
    """bad [H, W] bool -> [H - 10, W - 10] int64: the bad pixels in each 11 x 11 window."""
    H, W = bad.shape
    s = np.zeros((H + 1, W + 1), dtype=np.int64)
    s[1:, 1:] = bad.astype(np.int64).cumsum(0).cumsum(1)
    n = NTAPS
    return s[n:, n:] - s[:-n, n:] - s[n:, :-n] + s[:-n, :-n]


def pivot_and_range(b_plane: np.ndarray):
    """(r, L, lo, hi) of one truth plane in ITS dtype's arithmetic: lo / hi the min / max of
    the finite pixels, L = hi - lo, r = 0.5 lo + 0.5 hi (halving is exact, so one rounding and
    no overflow).  No finite pixel: all NaN."""
    dt = b_plane.dtype.type
    fin = b_plane[np.isfinite(b_plane)]
    if fin.size == 0:
        nan = dt(np.nan)
        return nan, nan, nan, nan
    lo, hi = fin.min(), fin.max()
    return dt(dt(0.5) * lo + dt(0.5) * hi), dt(hi - lo), lo, hi


def ssim(a: np.ndarray, b: np.ndarray, data_range=None, dtype=np.float64, round_taps: bool = True,
         full: bool = False) -> dict:
    """a (prediction), b (truth) [C, H, W] (fp32 as the device takes them; fp64 accepted) ->
    {'ssim', 'cs', 'mse', 'data_range' [C] fp64; 'nwin', 'npix' [C] int64; 'psnr' [C] fp64;
    'map' [C, H, W] of `dtype`: ssim at the used positions, NaN elsewhere}; with full=True
    also 'cs_map', 'mu_a', 'mu_b' (the means with the pivot added back), same layout."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.ndim != 3 or a.shape[1] < NTAPS or a.shape[2] < NTAPS:
        raise ValueError(f"fields {a.shape} / {b.shape}: two [C, H >= 11, W >= 11] arrays")
    if data_range is not None and not np.isfinite(data_range):
        raise ValueError(f"data_range {data_range!r}")
    dt = np.dtype(dtype).type
    C, H, W = a.shape
    g = taps(round_taps).astype(dt)
    R = RADIUS
    out = {k: np.full(C, np.nan) for k in ("ssim", "cs", "mse", "data_range", "psnr")}
    out["nwin"], out["npix"] = np.zeros(C, np.int64), np.zeros(C, np.int64)
    maps = {k: np.full((C, H, W), np.nan, dtype=dt) for k in ("map", "cs_map", "mu_a", "mu_b")}
    for c in range(C):
        r, L, _, _ = pivot_and_range(b[c])
        if data_range is not None and data_range > 0:
            L = b.dtype.type(data_range)
        fin = np.isfinite(a[c]) & np.isfinite(b[c])
        d = a[c][fin].astype(np.float64) - b[c][fin].astype(np.float64)
        out["npix"][c] = int(fin.sum())
        with np.errstate(invalid="ignore", divide="ignore"):
            out["mse"][c] = np.float64((d * d).sum()) / np.float64(fin.sum())
        out["data_range"][c] = L
        used = window_bad_count(~fin) == 0
        out["nwin"][c] = int(used.sum())
        # the pivoted fields, rounded to the working precision; 0 where a pixel is not usable
        # (such a pixel only reaches windows that are not used)
        with np.errstate(invalid="ignore", over="ignore"):
            pa = np.where(fin, a[c].astype(dt) - dt(r), dt(0))
            pb = np.where(fin, b[c].astype(dt) - dt(r), dt(0))
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            ma, mb = _valid(pa, g), _valid(pb, g)
            saa = _valid(pa * pa, g) - ma * ma
            sbb = _valid(pb * pb, g) - mb * mb
            sab = _valid(pa * pb, g) - ma * mb
            Ld = dt(L)
            C1, C2 = (dt(0.01) * Ld) ** 2, (dt(0.03) * Ld) ** 2
            cs = (dt(2) * sab + C2) / (saa + sbb + C2)
            mua, mub = ma + dt(r), mb + dt(r)
            s = (dt(2) * mua * mub + C1) / (mua * mua + mub * mub + C1) * cs
            nw = np.float64(used.sum())
            out["ssim"][c] = s[used].astype(np.float64).sum() / nw
            out["cs"][c] = cs[used].astype(np.float64).sum() / nw
            out["psnr"][c] = 10.0 * np.log10(np.float64(L) ** 2 / out["mse"][c])
        for k, v in (("map", s), ("cs_map", cs), ("mu_a", mua), ("mu_b", mub)):
            maps[k][c, R:H - R, R:W - R] = np.where(used, v, dt(np.nan))
    out["map"] = maps["map"]
    if full:
        out.update({k: maps[k] for k in ("cs_map", "mu_a", "mu_b")})
    return out
