"""The ensemble score's oracle (tests/ensemble_score_oracle.py) against the identities of its
definition (include/srmi.h, "the ensemble score") and the statistics of exchangeable draws; the
argument checks, the workspace's documented size, the netCDF round trip and the bindings; no
GPU."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import ensemble_score_oracle as eo
from srmi.ensemble_score import ENS_DERIVED, ENS_SPAN, ENS_SUMS, EnsembleScore, ensemble_workspace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("srmi_ensemble_score_workspace", "srmi_ensemble_score")
E_ARG, E_SHAPE = -10001, -10002
U = 2.0 ** -53


def draws(seed, K=8, shape=(1, 300, 517), scale=1.0):
    """Members and truth iid N(0, 1) fp32 (the members times ``scale``)."""
    rng = np.random.default_rng(seed)
    m = (scale * rng.standard_normal((K,) + shape)).astype(np.float32)
    y = rng.standard_normal(shape).astype(np.float32)
    return m, y


def test_the_tree_is_the_blends_pairwise_order():
    rng = np.random.default_rng(3)
    t = [np.float64(v) for v in rng.standard_normal(8) * 10.0 ** rng.integers(-8, 8, 8)]
    assert eo.tree(t[:2]) == t[0] + t[1] and eo.tree(t[:3]) == (t[0] + t[1]) + t[2]
    assert eo.tree(t[:5]) == ((t[0] + t[1]) + (t[2] + t[3])) + t[4]
    assert eo.tree(t[:6]) == ((t[0] + t[1]) + (t[2] + t[3])) + (t[4] + t[5])
    assert eo.tree(t[:7]) == ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + t[6])
    assert eo.tree(t) == ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]))


@pytest.mark.parametrize("K", [2, 3, 4, 8])
def test_identical_members(K):
    rng = np.random.default_rng(K)
    one = rng.standard_normal((2, 9, 11)).astype(np.float32)
    y = rng.standard_normal((2, 9, 11)).astype(np.float32)
    m = np.repeat(one[None], K, 0)
    t = eo.pixel_terms(m, y)
    assert np.all(t["b"] == 0.0)
    assert np.array_equal(t["crps"], t["crps_fair"])
    d = np.abs(one.astype(np.float64) - y.astype(np.float64))
    if K in (2, 4, 8):  # the tree of K equal terms is K times the term exactly
        assert np.array_equal(t["crps"], d) and np.all(t["var"] == 0.0) and np.all(t["s"] == 0.0)
    else:
        assert np.allclose(t["crps"], d, rtol=4 * U, atol=0) and np.all(t["var"] <= (4 * U * np.abs(one)) ** 2)
    assert set(np.unique(t["rank"])) <= {0, K}
    tabs = eo.tables(t, K, 1)
    assert np.array_equal(tabs["rank_hist"][:, 1:K], np.zeros((2, K - 1), dtype=np.int64))
    assert np.array_equal(tabs["rank_hist"].sum(1), tabs["used"]) and np.all(tabs["used"] == 99)
    r = eo.score(m, y)
    assert np.allclose(r["crps"], d.mean((1, 2)), rtol=1e-14)


def test_a_member_equal_to_the_truth_is_tied_and_does_not_raise_the_rank():
    m = np.array([-1.0, 0.5, 0.5, 2.0], dtype=np.float32).reshape(4, 1, 1, 1)
    y = np.array([[[0.5]]], dtype=np.float32)
    t = eo.pixel_terms(m, y)
    assert t["rank"][0, 0, 0] == 1 and t["tied"][0, 0, 0]
    y2 = np.array([[[0.6]]], dtype=np.float32)
    t2 = eo.pixel_terms(m, y2)
    assert t2["rank"][0, 0, 0] == 3 and not t2["tied"][0, 0, 0]
    tabs = eo.tables(t, 4, 1)
    assert tabs["tied"][0] == 1 and tabs["rank_hist"][0].tolist() == [0, 1, 0, 0, 0]
    # by hand: a = 1.5 + 0 + 0 + 1.5, b = 1.5 + 1.5 + 3 + 0 + 1.5 + 1.5
    assert t["a"][0, 0, 0] == 3.0 and t["b"][0, 0, 0] == 9.0
    assert t["crps"][0, 0, 0] == 3.0 / 4 - 9.0 / 16 and t["crps_fair"][0, 0, 0] == 3.0 / 4 - 9.0 / 12
    assert t["mean"][0, 0, 0] == 0.5 and t["var"][0, 0, 0] == (2.25 + 0 + 0 + 2.25) / 4


def test_nan_and_inf_are_the_mask_and_an_empty_channel_is_nan_with_zero_tables():
    m, y = draws(11, K=3, shape=(2, 7, 9))
    y[0, 0, 0], y[0, 1, 1] = np.nan, np.inf
    m[1, 0, 2, 2], m[2, 0, 0, 0] = -np.inf, np.nan
    y[1] = np.nan
    ed = np.array([[0.5, 1.0], [0.5, np.nan]], dtype=np.float32)
    r = eo.score(m, y, ed)
    assert r["used"].tolist() == [7 * 9 - 3, 0]
    assert np.isnan(r["crps_map"][0, 0, 0]) and np.isnan(r["crps_map"][0, 1, 1]) and np.isnan(r["crps_map"][0, 2, 2])
    assert np.isfinite(r["crps_map"][0]).sum() == 60 and np.isnan(r["crps_map"][1]).all()
    for k in ("rank_hist", "tied", "bin_count", "sums"):
        assert not r[k][1].any(), k
    for k in eo.DERIVED + ("bin_spread", "bin_rmse"):
        assert np.isnan(r[k][1]).all(), k
    assert np.isfinite(r["crps"][0]) and r["bin_count"][0].sum() == 60


def test_a_nan_edge_never_counts():
    m, y = draws(5, K=4, shape=(1, 20, 20))
    t = eo.pixel_terms(m, y, np.array([[np.nan, 0.0, np.nan]], dtype=np.float32))
    assert set(np.unique(t["bin"])) == {1}
    t = eo.pixel_terms(m, y, np.array([[0.8]], dtype=np.float32))
    assert np.array_equal(t["bin"][0], (t["s"][0].astype(np.float32) >= np.float32(0.8)).astype(np.int64))


@pytest.mark.parametrize("seed", range(5))
def test_exchangeable_draws(seed):
    """Truth and members from one distribution: a flat rank histogram, the fair CRPS of N(0, 1)
    against a draw of it, 1 / sqrt(pi), and a spread-skill ratio of 1."""
    K = 8
    m, y = draws(seed)
    terms = eo.pixel_terms(m, y)
    tabs = eo.tables(terms, K, 1)
    S = eo.sums(terms, 1)
    d = eo.derive(S, tabs, K)
    n = tabs["used"][0]
    assert n == 300 * 517
    h = tabs["rank_hist"][0].astype(np.float64)
    chi2 = float(((h - n / (K + 1)) ** 2 / (n / (K + 1))).sum())
    print(f"seed {seed}: chi2 {chi2:.2f}, crps_fair - 1/sqrt(pi) {d['crps_fair'][0] - 1 / math.sqrt(math.pi):+.2e}, "
          f"ssr {d['ssr'][0]:.4f}")
    assert chi2 < 26.12  # the 0.999 quantile of chi^2 at 8 degrees of freedom
    assert abs(d["crps_fair"][0] - 1 / math.sqrt(math.pi)) < 5e-3
    assert abs(d["ssr"][0] - 1.0) < 0.01
    # crps - crps_fair = b / (K (K - 1)) - b / K^2 = b / (K^2 (K - 1)): per pixel as exactly as fp64
    # has it -- each score is a rounded difference of a / K and a rounded quotient no larger than it
    # (the triangle inequality), so each is off by at most 2 u a / K and their rounded difference by
    # one u more
    u = terms["used"]
    crps, fair, a, b = (terms[k][u] for k in ("crps", "crps_fair", "a", "b"))
    assert np.all(crps >= fair)
    assert np.all(np.abs((crps - fair) - b / (K * K * (K - 1))) <= 6 * U * (a / K))
    assert abs((S[0, 0] - S[0, 1]) - S[0, 3] / (K * K * (K - 1))) <= 8 * U * S[0, 2] / K
    assert abs(d["outliers"][0] - d["outliers_expected"][0]) < 0.01 and d["outliers_expected"][0] == 2.0 / 9.0


def test_an_under_dispersed_ensemble():
    K = 8
    m, y = draws(0, scale=0.5)
    r = eo.score(m, y, (0.3, 0.5))
    assert r["ssr"][0] < 0.6  # about 0.5 by construction
    h = r["rank_hist"][0]
    assert h[0] > h[1:K].max() and h[K] > h[1:K].max() and 3 <= 1 + int(np.argmin(h[1:K])) <= 5  # a U
    assert r["outliers"][0] > 2.0 / (K + 1) + 0.1
    assert r["reliability_index"][0] > 0.2
    # the reliability table: every bin's rmse is above its spread
    assert np.all(r["bin_rmse"][0] > r["bin_spread"][0])
    assert r["bin_count"][0].sum() == r["used"][0] and np.all(r["bin_count"][0] > 0)


def test_sums_and_derived_agree_with_plain_numpy():
    m, y = draws(7, K=5, shape=(2, 31, 17))
    y = y + 0.3
    ed = np.array([0.6, 0.8, 1.0], dtype=np.float32)
    r = eo.score(m, y, ed)
    md, yd = m.astype(np.float64), y.astype(np.float64)
    mean, sd = md.mean(0), md.std(0)
    assert np.allclose(r["rmse_mean"], np.sqrt(((mean - yd) ** 2).mean((1, 2))), rtol=1e-12)
    assert np.allclose(r["spread_rms"], np.sqrt((sd ** 2).mean((1, 2))), rtol=1e-12)
    a = np.abs(md - yd[None]).mean(0)
    b = np.abs(md[:, None] - md[None]).sum((0, 1)) / 2
    assert np.allclose(r["crps"], (a - b / 25).mean((1, 2)), rtol=1e-12)
    assert np.allclose(r["crps_fair"], (a - b / 20).mean((1, 2)), rtol=1e-12)
    for c in range(2):
        cc = np.corrcoef(sd[c].ravel(), np.abs(mean[c] - yd[c]).ravel())[0, 1]
        assert abs(r["spread_error_corr"][c] - cc) < 1e-9
    assert np.allclose(r["ssr"], np.sqrt(6 / 4 * (sd ** 2).mean((1, 2))) / r["rmse_mean"], rtol=1e-12)
    assert np.array_equal(r["bin_count"].sum(1), r["used"])
    assert np.allclose(r["sums"][:, 9::2].sum(1), r["sums"][:, 4], rtol=1e-13)


def test_argument_checks_of_the_library():
    lib = __import__("srmi._lib", fromlist=["load"]).load()
    n = C.c_size_t(0)
    ws = lib.srmi_ensemble_score_workspace
    for bad in ((1, 1, 8, 8, 1), (9, 1, 8, 8, 1), (4, 1, 8, 8, 0), (4, 1, 8, 8, 17), (4, 0, 8, 8, 1), (4, 1, 0, 8, 1),
                (4, 1, 8, 0, 1), (4, 1, -3, 8, 1)):
        assert ws(*bad, C.byref(n)) == E_ARG, bad
    assert ws(4, 1, 8, 8, 1, None) == E_ARG
    assert ws(4, 1, 1 << 16, 1 << 15, 1, C.byref(n)) == E_SHAPE  # H W = 2^31
    assert ws(4, 1, 1 << 16, (1 << 15) - 1, 1, C.byref(n)) == 0
    assert ws(8, 2, 4096, 4096, 16, C.byref(n)) == 0 and n.value > 0
    # srmi_ensemble_score refuses before it launches anything: no device is touched
    fn = lib.srmi_ensemble_score
    p = 1 << 20  # stands for a buffer: never dereferenced by a refused call
    assert ws(4, 2, 8, 8, 3, C.byref(n)) == 0
    good = dict(members=p, truth=p, K=4, C=2, H=8, W=8, edges=p, B=3, workspace=p, bytes=n.value, counts=p, sums=p,
                derived=p, crps_map=None, launches=0, stream=None)

    def rc(**kw):
        a = dict(good, **kw)
        return fn(*a.values())
    for name in ("members", "truth", "edges", "workspace", "counts", "sums", "derived"):
        assert rc(**{name: None}) == E_ARG, name
    assert rc(workspace=p + 8) == E_ARG and rc(bytes=n.value - 1) == E_ARG and rc(launches=4) == E_ARG
    for kw in (dict(K=1), dict(K=9), dict(B=0), dict(B=17), dict(C=0), dict(H=0), dict(W=0)):
        assert rc(**kw) == E_ARG, kw
    assert rc(H=1 << 16, W=1 << 15) == E_SHAPE


def test_the_workspace_grows_as_documented():
    """Per channel and span of ENS_SPAN pixels of a plane: 9 + 2 B doubles (their block rounded up
    to 16 bytes) and K + 3 + B uint32."""
    def expect(K, Cn, H, W, B):
        blocks = -(-(H * W) // ENS_SPAN)
        return -(-(Cn * (9 + 2 * B) * blocks * 8) // 16) * 16 + Cn * (K + 3 + B) * blocks * 4
    for args in ((2, 1, 1, 1, 1), (8, 2, 37, 53, 16), (4, 1, 64, 64, 10), (4, 1, 64, 65, 10), (4, 3, 1, ENS_SPAN + 1, 2),
                 (3, 2, ENS_SPAN + 1, 1, 1), (8, 2, 300, 517, 10), (5, 1, 2 * ENS_SPAN, 3, 7)):
        assert ensemble_workspace(*args) == expect(*args), args
    assert ENS_SPAN == 4096 and len(ENS_SUMS) == 9 and ENS_SUMS == eo.SUMS and ENS_DERIVED == eo.DERIVED


def test_argument_checks_of_the_python_layer():
    # the constructor refuses before it touches a device
    for shape, ed in (((1, 2, 8, 8), []), ((9, 2, 8, 8), []), ((4, 0, 8, 8), []), ((4, 2, 0, 8), []),
                      ((4, 2, 8, -1), []), ((4, 2, 8), []), ((4, 1, 1 << 16, 1 << 15), []), ((4, 2, 8, 8), [0.1] * 16),
                      ((4, 2, 8, 8), np.zeros((3, 2))), ((4, 2, 8, 8), "x"), ((4, 2, 8, 8), np.zeros((2, 2, 2)))):
        with pytest.raises(ValueError):
            EnsembleScore(shape, ed, device="cuda:0")
    import torch
    for ed in (torch.zeros((2, 3), dtype=torch.float64), torch.zeros((3, 3)), torch.zeros(3), torch.zeros((2, 16))):
        with pytest.raises(ValueError, match="edges"):  # a host tensor is not on the device either
            EnsembleScore((4, 2, 8, 8), ed, device="cuda:0")
    for bad in ((1, 1, 8, 8, 1), (4, 1, 8, 8, 17), (4, 1, 1 << 16, 1 << 15, 1)):
        with pytest.raises(ValueError):
            ensemble_workspace(*bad)


def test_save_and_load_round_trip(tmp_path):
    from srmi.results import load_ensemble_score, save_ensemble_score
    m, y = draws(8, K=4, shape=(2, 12, 15))
    y[1] = np.nan  # an empty channel: NaN survives
    ed = np.array([[0.5, 0.7, np.nan], [0.1, 0.2, 0.3]], dtype=np.float32)
    r = dict(eo.score(m, y, ed), edges=ed)
    r["rank_hist"][0, 2] = (1 << 60) + 12345  # above 2^53: the tables are kept as integers
    path = save_ensemble_score(str(tmp_path / "e.nc"), r, ["SST", "SSS"])
    back, names = load_ensemble_score(path)
    assert names == ["SST", "SSS"]
    assert back["edges"].dtype == np.float32 and np.array_equal(back["edges"], ed, equal_nan=True)
    for k in ("used", "rank_hist", "tied", "bin_count"):
        assert back[k].dtype == np.int64 and np.array_equal(back[k], r[k]), k
    for k in eo.DERIVED + ("bin_spread", "bin_rmse", "sums"):
        assert back[k].dtype == np.float64 and np.array_equal(back[k], r[k], equal_nan=True), k
    assert back["crps_map"].dtype == np.float32 and np.array_equal(back["crps_map"], r["crps_map"], equal_nan=True)
    # one bin: no edges; no map
    r1 = dict(eo.score(m, y), edges=np.zeros((2, 0), dtype=np.float32))
    del r1["crps_map"]
    back, _ = load_ensemble_score(save_ensemble_score(str(tmp_path / "e1.nc"), r1, ["a", "b"]))
    assert back["edges"].shape == (2, 0) and "crps_map" not in back and np.array_equal(back["bin_count"], r1["bin_count"])
    with pytest.raises(ValueError, match="lacks"):
        save_ensemble_score(str(tmp_path / "bad.nc"), {"used": r["used"]}, ["SST", "SSS"])
    with pytest.raises(ValueError, match="sums"):
        save_ensemble_score(str(tmp_path / "bad.nc"), dict(r, sums=r["sums"][:, :5]), ["SST", "SSS"])


def test_symbols_are_declared_and_bound():
    from srmi import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "srmi.h")).read()
    for name in SYMBOLS:
        assert name in _lib.EXPORTED and hasattr(lib, name) and f"int {name}(" in header
    from srmi import results
    from srmi.superres import RegionSuperResolver
    assert hasattr(RegionSuperResolver, "score_ensemble")
    assert hasattr(results, "save_ensemble_score") and hasattr(results, "load_ensemble_score")
    import inspect
    assert inspect.signature(RegionSuperResolver.__init__).parameters["members"].default is False
