"""The quantile map's definition (tests/quantile_map_oracle.py) against the properties that
make it a quantile map, the host side of srmi.quantile_map and the result file, on the CPU.

The calibration bars are conditions of the issue, not measurements: on truth ~ N(0, 1), pred =
0.7 truth + 0.1 noise + 0.05, N = 2^14, range (-4, 4), B = 256, tail_count = 16, the mapped
prediction's W1 (sorted samples, fp64) falls at least 10 x in sample and at least 5 x on a
fresh draw.  Measured with this oracle: x 130 and x 46.
"""
import numpy as np
import pytest
import torch

import distribution_oracle as do
import quantile_map_oracle as qo
from srmi.quantile_map import QuantileMap, knot_edges
from srmi.results import load_quantile_map, save_quantile_map


def tables(rng, B, kind):
    """a table [B + 2] of one of the awkward kinds"""
    M = B + 2
    if kind == "random":
        return rng.integers(0, 50, M)
    if kind == "sparse":  # most bins empty
        return rng.integers(0, 50, M) * (rng.random(M) < 0.2)
    if kind == "one-bin":
        h = np.zeros(M, dtype=np.int64)
        h[int(rng.integers(0, M))] = 1000
        return h
    if kind == "zeros-at-the-ends":
        h = rng.integers(1, 50, M)
        h[:max(1, M // 4)] = 0
        h[-max(1, M // 3):] = 0
        return h
    if kind == "outer-only":
        h = np.zeros(M, dtype=np.int64)
        h[0], h[-1] = 7, 5
        return h
    if kind == "empty":  # N == 0
        return np.zeros(M, dtype=np.int64)
    raise AssertionError(kind)


KINDS = ("random", "sparse", "one-bin", "zeros-at-the-ends", "outer-only", "empty")


def same_sum(rng, ha, hb):
    """hb with ha's sum: the difference goes to (or comes from) random entries of hb"""
    hb = hb.astype(np.int64).copy()
    d = int(ha.sum() - hb.sum())
    while d != 0:
        k = int(rng.integers(0, hb.size))
        if d > 0:
            hb[k] += d
            d = 0
        else:
            take = min(-d, int(hb[k]))
            hb[k] -= take
            d += take
    return hb


@pytest.mark.parametrize("B", [2, 64, 4096])
def test_equal_tables_give_the_identity_exactly(B):
    rng = np.random.default_rng(B)
    for lo, hi in ((-4.0, 4.0), (271.35, 305.1), (0.0, 1e-3)):
        e = qo.edges(lo, hi, B)
        assert np.array_equal(e, knot_edges([[lo, hi]], B)[0]) and e[B + 1] == np.float64(np.float32(hi))
        for kind in KINDS:
            h = tables(rng, B, kind)
            for tail in (0, 16):
                T = qo.fit_channel(h, h, lo, hi, B, tail)
                assert np.array_equal(T, e), (B, kind, tail)
        assert np.array_equal(qo.fit_channel(np.zeros(B + 2), np.zeros(B + 2), lo, hi, B, 0), e)  # N == 0


@pytest.mark.parametrize("B", [2, 16, 64, 256, 4096])
def test_the_knots_never_decrease(B):
    rng = np.random.default_rng(100 + B)
    n = 0
    for ka in KINDS:
        for kb in KINDS:
            for tail in (0, 3, 16, 10 ** 6):
                ha = tables(rng, B, ka)
                hb = same_sum(rng, ha, tables(rng, B, kb))
                T = qo.fit_channel(ha, hb, -1.0, 3.0, B, tail)
                assert T.shape == (B + 3,) and np.isfinite(T).all()
                assert (np.diff(T) >= 0).all(), (B, ka, kb, tail, int((np.diff(T) < 0).sum()))
                n += 1
    assert n == 144
    # N == 0 on both sides, named: the identity, which does not decrease
    T = qo.fit_channel(np.zeros(B + 2), np.zeros(B + 2), -1.0, 3.0, B, 16)
    assert np.array_equal(T, qo.edges(-1.0, 3.0, B)) and (np.diff(T) >= 0).all()


def test_tail_count_moves_only_the_untrusted_knots_by_the_stated_shifts():
    B, lo, hi = 64, -4.0, 4.0
    rng = np.random.default_rng(7)
    truth = rng.standard_normal(4096).astype(np.float32)
    pred = (0.7 * truth + 0.05).astype(np.float32)
    hist, _ = qo.accumulate(pred[None, None], truth[None, None], None, B, (lo, hi))
    ha, hb = hist[0]
    e = qo.edges(lo, hi, B)
    T0 = qo.fit_channel(ha, hb, lo, hi, B, 0)
    ca = np.concatenate([[0], np.cumsum(ha)])
    N = int(ca[-1])
    for tail in (1, 16, 200):
        T = qo.fit_channel(ha, hb, lo, hi, B, tail)
        trusted = (ca >= tail) & (N - ca >= tail)
        j0, j1 = np.nonzero(trusted)[0][[0, -1]]
        assert 0 < j0 < j1 < B + 2 and trusted[j0:j1 + 1].all()
        assert np.array_equal(T[trusted], T0[trusted])
        assert np.array_equal(T[:j0], e[:j0] + (T0[j0] - e[j0]))
        assert np.array_equal(T[j1 + 1:], e[j1 + 1:] + (T0[j1] - e[j1]))
    assert np.array_equal(qo.fit_channel(ha, hb, lo, hi, B, N), e)  # no knot has N samples on both sides


def calibration(seed, n=2 ** 14):
    rng = np.random.default_rng(seed)
    truth = rng.standard_normal(n)
    pred = 0.7 * truth + 0.1 * rng.standard_normal(n) + 0.05
    return pred.astype(np.float32).reshape(1, 128, n // 128), truth.astype(np.float32).reshape(1, 128, n // 128)


def test_the_map_calibrates_a_compressed_prediction():
    B, rng_, tail = 256, (-4.0, 4.0), 16
    pred, truth = calibration(11)
    hist, count = qo.accumulate(pred, truth, None, B, rng_)
    assert count[0] == 2 ** 14
    knots, table, meta = qo.fit(hist, B, rng_, tail)
    before = qo.w1_samples(pred, truth)
    after = qo.w1_samples(qo.apply(pred, None, table, meta, B), truth)
    pred2, truth2 = calibration(12)
    before2 = qo.w1_samples(pred2, truth2)
    after2 = qo.w1_samples(qo.apply(pred2, None, table, meta, B), truth2)
    print(f"W1 in sample {before:.4f} -> {after:.5f} (x {before / after:.0f}), fresh draw {before2:.4f} -> "
          f"{after2:.5f} (x {before2 / after2:.0f})")
    assert after * 10 <= before
    assert after2 * 5 <= before2


def test_the_detail_map_corrects_the_detail_and_adds_it_to_the_field():
    """on="detail": the table is fitted and read on x - base, the correction is added to x."""
    B, rng_ = 64, (-4.0, 4.0)
    pred, truth = calibration(13, 2 ** 12)
    base = (290.0 + np.linspace(0, 5, pred.size)).astype(np.float32).reshape(pred.shape)
    with_base = ((pred + base).astype(np.float32), (truth + base).astype(np.float32))
    hist, count = qo.accumulate(*with_base, base, B, rng_)
    dsrc, dtruth = with_base[0] - base, with_base[1] - base
    hist0, count0 = qo.accumulate(dsrc, dtruth, None, B, rng_)
    assert np.array_equal(hist, hist0) and np.array_equal(count, count0)
    _, table, meta = qo.fit(hist, B, rng_, 4)
    out = qo.apply(with_base[0], base, table, meta, B)
    mapped = qo.apply(dsrc, None, table, meta, B)
    assert np.array_equal(out, with_base[0] + (mapped - dsrc))


def test_strength_nan_and_infinities():
    B, rng_ = 16, (-2.0, 2.0)
    pred, truth = calibration(14, 2 ** 12)
    hist, _ = qo.accumulate(pred, truth, None, B, rng_)
    _, table, meta = qo.fit(hist, B, rng_, 4)
    x = pred.copy()
    full, half, none = (qo.apply(x, None, table, meta, B, s) for s in (1.0, 0.5, 0.0))
    assert np.array_equal(none, x)
    assert np.allclose(half - x, 0.5 * (full - x), rtol=0, atol=2e-7) and np.abs(full - x).max() > 0.1
    x = pred.copy()
    flat = x.reshape(-1)
    nan_bits = np.array([0x7fc00000, 0xffc00001, 0x7f800001, 0x7fffffff], dtype=np.uint32).view(np.float32)
    flat[:4] = nan_bits
    flat[4], flat[5], flat[6], flat[7] = np.inf, -np.inf, 3e38, -3e38
    flat[8], flat[9] = 2.0, -2.0  # exactly hi and lo
    out = qo.apply(x, None, table, meta, B).reshape(-1)
    assert np.array_equal(out[:4].view(np.uint32), nan_bits.view(np.uint32))
    assert out[4] == np.inf and out[5] == -np.inf
    assert out[6] == np.float32(3e38) + meta[0, 3] and out[7] == np.float32(-3e38) + meta[0, 2]
    assert np.isfinite(out[8:]).all()
    # a NaN only in the base passes x through, bits and all
    base = np.zeros_like(x)
    base.reshape(-1)[20] = np.nan
    outb = qo.apply(x, base, table, meta, B).reshape(-1)
    assert outb[20].view(np.uint32) == flat[20].view(np.uint32) and outb[21] == out[21]


def test_accumulate_adds_and_masks():
    B, rng_ = 16, [(289.0, 291.0), (-1.0, 1.0)]
    rng = np.random.default_rng(3)
    a = (rng.standard_normal((2, 20, 30)) + np.array([290.0, 0.0])[:, None, None]).astype(np.float32)
    b = (rng.standard_normal((2, 20, 30)) + np.array([290.0, 0.0])[:, None, None]).astype(np.float32)
    a[0, 3, 4] = np.nan
    b[1, 5, 6] = np.inf
    h1, n1 = qo.accumulate(a, b, None, B, rng_)
    assert n1.tolist() == [599, 599] and (h1.sum(2) == 599).all()
    for c in range(2):
        used = np.isfinite(a[c]) & np.isfinite(b[c])
        assert np.array_equal(h1[c, 0], np.bincount(do.bin_index(a[c][used], *rng_[c], B), minlength=B + 2))
    h2, n2 = qo.accumulate(b, a, None, B, rng_, h1, n1)
    assert np.array_equal(h2[:, 0], h1[:, 0] + h1[:, 1]) and np.array_equal(h2[:, 1], h2[:, 0]) and (n2 == 1198).all()


def test_save_and_load_round_trip(tmp_path):
    B, rng_ = 32, [(289.0, 291.0), (-1.0, 1.0)]
    rng = np.random.default_rng(4)
    a = (rng.standard_normal((2, 20, 30)) * 0.3 + np.array([290.0, 0.0])[:, None, None]).astype(np.float32)
    b = (rng.standard_normal((2, 20, 30)) * 0.4 + np.array([290.0, 0.0])[:, None, None]).astype(np.float32)
    hist, count = qo.accumulate(a, b, None, B, rng_)
    knots, _, _ = qo.fit(hist, B, rng_, 5)
    sd = {"hist": hist, "count": count, "range": qo.ranges_of(rng_, 2), "bins": B, "on": "detail", "tail_count": 5,
          "knots": knots}
    path = save_quantile_map(str(tmp_path / "qm.nc"), sd, ["SST", "SSS"])
    back, names = load_quantile_map(path)
    assert names == ["SST", "SSS"] and back["bins"] == B and back["on"] == "detail" and back["tail_count"] == 5
    for k in ("hist", "count"):
        assert back[k].dtype == np.int64 and np.array_equal(back[k], sd[k]), k
    assert back["range"].dtype == np.float32 and np.array_equal(back["range"], sd["range"])
    assert np.array_equal(back["knots"], knots)
    assert np.array_equal(back["edges"], np.stack([qo.edges(*r, B) for r in rng_]))
    # the state loads into an object (on the CPU: tables only), and an unfitted state has no knots
    qm = QuantileMap(2, (0.0, 1.0), bins=B, on="value", device="cpu")
    qm.load_state_dict(back)
    assert qm.on == "detail" and qm.tail_count == 5 and np.array_equal(qm.range, sd["range"]) and not qm.fitted
    assert np.array_equal(qm.hist.numpy(), hist) and np.array_equal(qm.state_dict()["count"], count)
    del sd["knots"]
    back2, _ = load_quantile_map(save_quantile_map(str(tmp_path / "qm2.nc"), qm, ["SST", "SSS"]))
    assert "knots" not in back2 and np.array_equal(back2["hist"], hist)
    with pytest.raises(ValueError):
        save_quantile_map(str(tmp_path / "bad.nc"), sd, ["SST"])
    with pytest.raises(ValueError):
        save_quantile_map(str(tmp_path / "bad.nc"), {"hist": hist}, ["SST", "SSS"])
    with pytest.raises(ValueError):
        QuantileMap(2, (0.0, 1.0), bins=16, device="cpu").load_state_dict(back)


@pytest.mark.parametrize("kw", [dict(channels=0), dict(channels=17), dict(channels=1.5), dict(bins=1), dict(bins=4097),
                                dict(on="both"), dict(tail_count=-1), dict(tail_count=1.5),
                                dict(value_range=(1.0, 1.0)), dict(value_range=(2.0, 1.0)),
                                dict(value_range=(float("nan"), 1.0)), dict(value_range=(0.0, float("inf"))),
                                dict(value_range=(0.0, 1e39)), dict(value_range=(-3e38, 3e38)), dict(value_range=[(0.0, 1.0)] * 3),
                                dict(value_range=(0.0, 1.0, 2.0)), dict(value_range=None)],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()).replace(" ", ""))
def test_bad_arguments_are_refused_before_anything_is_allocated(kw, monkeypatch):
    def no_alloc(*a, **k):
        raise AssertionError("allocated before the arguments were checked")
    monkeypatch.setattr(torch, "zeros", no_alloc)
    monkeypatch.setattr(torch, "empty", no_alloc)
    args = dict(channels=2, value_range=(0.0, 1.0), bins=16, on="detail", tail_count=4, device="cpu")
    args.update(kw)
    with pytest.raises(ValueError):
        QuantileMap(**args)


def test_a_cpu_object_holds_tables_and_refuses_to_launch():
    qm = QuantileMap(1, (0.0, 1.0), bins=8, on="value", device="cpu")
    x = torch.zeros((1, 4, 4))
    for call in (lambda: qm.accumulate(x, x), qm.fit, lambda: qm.apply(x)):
        with pytest.raises(RuntimeError):
            call()


def test_from_histograms_on_oracle_histograms():
    B, rng_ = 64, (285.0, 295.0)
    rng = np.random.default_rng(9)
    truth = (290.0 + 1.5 * rng.standard_normal((2, 64, 96))).astype(np.float32)
    pred = (290.0 + 0.7 * (truth - 290.0) + 0.1).astype(np.float32)
    o = do.distribution(pred, truth, bins=B, joint=0, value_range=rng_)
    qm = QuantileMap.from_histograms(o["hist_pred"], torch.tensor(o["hist_truth"]), rng_, tail_count=8, device="cpu")
    sd = qm.state_dict()
    hist, count = qo.accumulate(pred, truth, None, B, rng_)
    assert qm.on == "value" and qm.bins == B and qm.C == 2 and qm.tail_count == 8
    assert np.array_equal(sd["hist"], hist) and np.array_equal(sd["count"], count) and "knots" not in sd
    assert np.array_equal(sd["range"], qo.ranges_of(rng_, 2))
    # the map those tables give brings the prediction's quantiles onto the truth's
    _, table, meta = qo.fit(sd["hist"], B, sd["range"], qm.tail_count)
    after = do.distribution(qo.apply(pred, None, table, meta, B), truth, bins=B, joint=0, value_range=rng_)
    assert np.abs(after["q_bias"]).max() < 0.25 * np.abs(o["q_bias"]).max()
    with pytest.raises(ValueError):
        QuantileMap.from_histograms(o["hist_pred"], o["hist_truth"], None, device="cpu")  # a score without a range
    with pytest.raises(ValueError):
        QuantileMap.from_histograms(o["hist_pred"], o["hist_truth"][:, :-1], rng_, device="cpu")
    bad = o["hist_truth"].copy()
    bad[0, 5] += 1
    with pytest.raises(ValueError):
        QuantileMap.from_histograms(o["hist_pred"], bad, rng_, device="cpu")
