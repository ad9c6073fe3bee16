"""The numpy oracle of the SSIM score (tests/ssim_oracle.py) pinned on its own: against
scipy's Gaussian filter, on fields with a known answer, and on the mask.

Two of the checks are stated with care, because the plain statement does not hold:

* The definition rounds the 11 taps to fp32 (the device holds them so).  scipy's
  gaussian_filter(sigma=1.5, truncate=3.5) uses the same 11 taps in fp64.  The oracle with
  ``round_taps=False`` must match scipy to 1e-12 (the formula, the separable window, the
  crop, the pivot); the taps of the definition must be exactly those fp64 taps rounded to
  fp32; and the score with the rounded taps stays within 1e-6 of the unrounded one (each tap
  moves by at most 2^-25 relative, the windows' sums by as much, and ssim is a ratio of such
  sums with every term positive in the denominators).  Constant fields are pinned the same
  way: exactly with the fp64 taps, and with the definition's taps to the bound that their
  sum, 1 + d instead of 1, sets.
* ssim is not invariant under a common shift of both fields -- its luminance factor reads
  the absolute means -- but cs is, and the means move with the shift.  So a field at
  290 +- 1.5 and the same field minus 290 must give the same cs map, means that differ by
  290, and an ssim map that equals luminance(means + 290) x cs of the shifted pair, each to
  1e-12: the pivot is harmless in fp64.
"""
import numpy as np
import pytest
import scipy.ndimage

import ssim_oracle as so


def fields(shape, seed=0, mean=5.0, std=2.0, noise=0.4, dtype=np.float64):
    rng = np.random.default_rng(seed)
    b = mean + std * rng.standard_normal(shape)
    a = b + noise * rng.standard_normal(shape)
    return a.astype(dtype), b.astype(dtype)


def scipy_ssim(a, b, L):
    """The textbook formula on one plane, no pivot, scipy's window; cropped by 5."""
    def G(x):
        return scipy.ndimage.gaussian_filter(x, sigma=1.5, truncate=3.5)[5:-5, 5:-5]
    mua, mub = G(a), G(b)
    saa, sbb, sab = G(a * a) - mua * mua, G(b * b) - mub * mub, G(a * b) - mua * mub
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    cs = (2 * sab + C2) / (saa + sbb + C2)
    return (2 * mua * mub + C1) / (mua * mua + mub * mub + C1) * cs, cs


def test_taps_are_scipys_rounded_to_fp32():
    delta = np.zeros(31)
    delta[15] = 1.0
    k = scipy.ndimage.gaussian_filter1d(delta, sigma=1.5, truncate=3.5)
    assert np.count_nonzero(k) == 11 and np.count_nonzero(k[10:21]) == 11
    g64 = so.taps(round_taps=False)
    assert g64.dtype == np.float64 and np.allclose(k[10:21], g64, rtol=1e-15, atol=0)
    assert abs(g64.sum() - 1.0) < 1e-15
    g = so.taps()
    assert g.dtype == np.float32 and np.array_equal(g, g64.astype(np.float32))
    assert np.array_equal(g, g[::-1])


def test_interior_matches_scipy_gaussian_filter():
    a, b = fields((2, 40, 56), seed=1)
    res = so.ssim(a, b, round_taps=False, full=True)
    for c in range(2):
        L = b[c].max() - b[c].min()
        assert res["data_range"][c] == L
        s, cs = scipy_ssim(a[c], b[c], L)
        got, got_cs = res["map"][c, 5:-5, 5:-5], res["cs_map"][c, 5:-5, 5:-5]
        print(f"channel {c}: ssim {np.abs(got - s).max():.2e}, cs {np.abs(got_cs - cs).max():.2e} off scipy")
        assert np.abs(got - s).max() <= 1e-12 and np.abs(got_cs - cs).max() <= 1e-12
        assert abs(res["ssim"][c] - s.mean()) <= 1e-12 and abs(res["cs"][c] - cs.mean()) <= 1e-12
        assert np.isnan(res["map"][c, :5]).all() and np.isnan(res["map"][c, :, -5:]).all()
        assert res["nwin"][c] == 30 * 46 and res["npix"][c] == 40 * 56
        assert np.isclose(res["mse"][c], ((a[c] - b[c]) ** 2).mean(), rtol=1e-13)
        assert np.isclose(res["psnr"][c], 10 * np.log10(L * L / res["mse"][c]), rtol=1e-13)
    # the definition's fp32 taps: the same score to 1e-6 (module docstring)
    rounded = so.ssim(a, b)
    assert np.nanmax(np.abs(rounded["map"] - res["map"])) <= 1e-6
    assert np.abs(rounded["ssim"] - res["ssim"]).max() <= 1e-6


def test_constant_fields():
    p, q, L = 3.0, 3.5, 2.0
    a, b = np.full((1, 20, 23), p), np.full((1, 20, 23), q)
    res = so.ssim(a, b, data_range=L, round_taps=False, full=True)
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    want = (2 * p * q + C1) / (p * p + q * q + C1)
    assert res["data_range"][0] == L
    assert abs(res["ssim"][0] - want) <= 1e-12 and abs(res["cs"][0] - 1.0) <= 1e-12
    assert np.abs(res["cs_map"][0, 5:-5, 5:-5] - 1.0).max() <= 1e-12
    assert np.isclose(res["mse"][0], 0.25, rtol=1e-14)
    # the definition's fp32 taps sum to 1 + d, not 1: a constant a - r = p - q then has the
    # "variance" (p - q)^2 ((1 + d)^2 - (1 + d)^4), about -2 d (p - q)^2, which cs sees over C2
    d = so.taps().astype(np.float64).sum() - 1.0
    tol = 2.0 * (2.0 * abs(d) * (p - q) ** 2 / C2) + 1e-12
    rounded = so.ssim(a, b, data_range=L)
    print(f"taps sum to 1 {d:+.2e}: cs off 1 by {abs(rounded['cs'][0] - 1.0):.2e}, bound {tol:.2e}")
    assert 0 < abs(d) < 11 * 2.0 ** -25 and tol < 1e-5
    assert abs(rounded["ssim"][0] - want) <= tol and abs(rounded["cs"][0] - 1.0) <= tol
    # no data_range: L = 0 and flat windows, cs = 0 / 0 (not special-cased)
    flat = so.ssim(a, a)
    assert flat["data_range"][0] == 0.0 and np.isnan(flat["cs"][0]) and flat["nwin"][0] == 10 * 13


def test_ssim_of_a_field_with_itself_is_one():
    a, _ = fields((2, 24, 31), seed=2)
    res = so.ssim(a, a)
    assert np.abs(res["ssim"] - 1.0).max() <= 1e-12 and np.abs(res["cs"] - 1.0).max() <= 1e-12
    assert (res["mse"] == 0.0).all() and np.isinf(res["psnr"]).all()
    r32 = so.ssim(a.astype(np.float32), a.astype(np.float32), dtype=np.float32)
    assert r32["map"].dtype == np.float32 and np.abs(r32["ssim"] - 1.0).max() <= 1e-6


def test_pivot_is_harmless_in_fp64():
    a, b = fields((1, 30, 34), seed=3, mean=290.0, std=1.5, noise=0.3)
    a0, b0 = a - 290.0, b - 290.0
    L = float(b.max() - b.min())
    hi, lo = so.ssim(a, b, data_range=L, full=True), so.ssim(a0, b0, data_range=L, full=True)
    v = np.s_[0, 5:-5, 5:-5]
    assert np.abs(hi["cs_map"][v] - lo["cs_map"][v]).max() <= 1e-12
    assert abs(hi["cs"][0] - lo["cs"][0]) <= 1e-12
    assert np.abs(hi["mu_a"][v] - 290.0 - lo["mu_a"][v]).max() <= 1e-12 * 290
    assert np.abs(hi["mu_b"][v] - 290.0 - lo["mu_b"][v]).max() <= 1e-12 * 290
    C1 = (0.01 * L) ** 2
    ma, mb = lo["mu_a"][v] + 290.0, lo["mu_b"][v] + 290.0
    want = (2 * ma * mb + C1) / (ma * ma + mb * mb + C1) * lo["cs_map"][v]
    assert np.abs(hi["map"][v] - want).max() <= 1e-12
    # and the unpivoted textbook formula agrees as far as its own cancellation allows:
    # E[x^2] - mu^2 at 290 loses 290^2 eps = 2e-11 of a variance of 2.25
    s, _ = scipy_ssim(a[0], b[0], L)
    assert np.abs(so.ssim(a, b, data_range=L, round_taps=False)["map"][v] - s).max() <= 1e-10


def test_one_nan_removes_exactly_its_windows():
    a, b = fields((2, 40, 56), seed=4)
    base = so.ssim(a, b)
    for where in ("a", "b"):
        a2, b2 = a.copy(), b.copy()
        (a2 if where == "a" else b2)[1, 17, 23] = np.nan
        res = so.ssim(a2, b2)
        assert res["nwin"][1] == base["nwin"][1] - 121 and res["npix"][1] == base["npix"][1] - 1
        assert res["nwin"][0] == base["nwin"][0] and res["npix"][0] == base["npix"][0]
        gone = np.isnan(res["map"][1]) & ~np.isnan(base["map"][1])
        yy, xx = np.nonzero(gone)
        assert gone.sum() == 121 and yy.min() == 12 and yy.max() == 22 and xx.min() == 18 and xx.max() == 28
        keep = ~np.isnan(res["map"][1])
        if where == "a":  # the truth's range is untouched: the other positions keep their bits
            assert np.array_equal(res["map"][1][keep], base["map"][1][keep])
            assert np.array_equal(res["map"][0], base["map"][0], equal_nan=True)
        assert np.isfinite(res["ssim"]).all()


def test_a_channel_without_a_finite_pixel():
    a, b = fields((2, 24, 31), seed=5)
    base = so.ssim(a, b)
    for where in ("a", "b", "both"):
        a2, b2 = a.copy(), b.copy()
        if where in ("a", "both"):
            a2[0] = np.nan
        if where in ("b", "both"):
            b2[0] = np.inf
        res = so.ssim(a2, b2)
        assert res["nwin"][0] == 0 and res["npix"][0] == 0
        assert np.isnan(res["ssim"][0]) and np.isnan(res["cs"][0]) and np.isnan(res["mse"][0])
        assert np.isnan(res["map"][0]).all()
        for k in ("ssim", "cs", "mse", "nwin", "npix", "data_range"):
            assert res[k][1] == base[k][1], k
        assert np.array_equal(res["map"][1], base["map"][1], equal_nan=True)


def test_fp32_mode_is_close_and_refusals():
    a, b = fields((1, 37, 70), seed=6, mean=290.0, std=1.5, noise=0.3, dtype=np.float32)
    o64, o32 = so.ssim(a, b), so.ssim(a, b, dtype=np.float32)
    e32 = np.nanmax(np.abs(o32["map"].astype(np.float64) - o64["map"]))
    print(f"e32 on a 290 +- 1.5 field: {e32:.3e}")
    assert 0 < e32 < 1e-5 and o32["nwin"][0] == o64["nwin"][0] == 27 * 60
    assert o64["data_range"][0] == np.float32(b.max()) - np.float32(b.min())
    with pytest.raises(ValueError):
        so.ssim(a[:, :10], b[:, :10])
    with pytest.raises(ValueError):
        so.ssim(a, b, data_range=float("nan"))


def test_save_ssim_round_trips(tmp_path):
    from srmi.results import load_ssim, save_ssim
    a, b = fields((2, 24, 31), seed=7, dtype=np.float32)
    a[1, 12, 15] = np.nan
    res = so.ssim(a, b, dtype=np.float32)
    score = {k: res[k].astype(np.float32) for k in ("ssim", "cs", "mse", "psnr", "data_range")}
    score.update(nwin=res["nwin"], npix=res["npix"], map=res["map"])
    path = save_ssim(str(tmp_path / "ssim.nc"), score, ["SST", "SSS"])
    back, names = load_ssim(path)
    assert names == ["SST", "SSS"]
    for k in ("ssim", "cs", "mse", "psnr", "data_range", "map"):
        assert back[k].dtype == np.float32 and np.array_equal(back[k], score[k], equal_nan=True), k
    for k in ("nwin", "npix"):
        assert back[k].dtype == np.int64 and np.array_equal(back[k], score[k]), k
    del score["map"]
    back, _ = load_ssim(save_ssim(path, score, ["SST", "SSS"]))
    assert "map" not in back and np.array_equal(back["nwin"], res["nwin"])
    with pytest.raises(ValueError):
        save_ssim(path, {"ssim": score["ssim"]}, ["SST", "SSS"])
    with pytest.raises(ValueError):
        save_ssim(path, score, ["SST"])
