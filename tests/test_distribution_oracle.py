"""The distribution score's definition (tests/distribution_oracle.py) against independent
computations, the two host helpers of srmi.distribution and the result file, on the CPU.

The oracle forms a value's bin in fp32 with the three operations of the definition.
np.histogram forms it in fp64.  The two disagree on the few pixels that sit within an fp32
rounding of a bin edge; the first test counts them and requires them to be at most 1e-4 of
the pixels, and requires the oracle's tables to BE np.histogram's once those pixels are
moved.  Those pixels are why the device is held to the fp32 definition, not to np.histogram.
"""
import numpy as np
import pytest

import distribution_oracle as do
from srmi.distribution import bin_edges, contingency
from srmi.results import load_distribution, save_distribution


def white(shape, seed=0):
    rng = np.random.default_rng(300 + seed)
    truth = (290.0 + 1.5 * rng.standard_normal(shape)).astype(np.float32)
    pred = (truth + 0.3 * rng.standard_normal(shape)).astype(np.float32)
    return pred, truth


def numpy_bins(x, lo, hi, B):
    """np.histogram's own bin of every value of x inside [lo, hi] (1 .. B), in fp64."""
    edges = np.histogram_bin_edges(x, bins=B, range=(float(lo), float(hi)))
    k = np.searchsorted(edges, x, side="right")
    k[x == edges[-1]] = B  # the last bin is closed
    assert np.array_equal(np.bincount(k, minlength=B + 1)[1:B + 1], np.histogram(x, bins=B, range=(lo, hi))[0])
    return k


@pytest.mark.parametrize("shape,B", [((2, 300, 517), 16), ((2, 300, 517), 256), ((2, 300, 517), 4096),
                                     ((1, 1024, 1024), 256)], ids=["B16", "B256", "B4096", "1024sq"])
def test_the_tables_are_numpy_histograms_but_for_the_pixels_on_an_fp32_edge(shape, B):
    pred, truth = white(shape)
    o = do.distribution(pred, truth, bins=B, joint=0, probs=())
    moved, total = 0, 0
    for c in range(shape[0]):
        lo, hi = o["lo"][c], o["hi"][c]
        assert lo == truth[c].min() and hi == truth[c].max()
        for key, field in (("hist_pred", pred[c]), ("hist_truth", truth[c])):
            x = field.reshape(-1)
            x = x[(x >= lo) & (x <= hi)].astype(np.float64)
            k32 = do.bin_index(x.astype(np.float32), lo, hi, B)
            kn = numpy_bins(x, np.float64(lo), np.float64(hi), B)
            diff = k32 != kn
            moved += int(diff.sum())
            total += x.size
            fixed = o[key][c].copy()
            fixed -= np.bincount(k32[diff], minlength=B + 2)
            fixed += np.bincount(kn[diff], minlength=B + 2)
            assert np.array_equal(fixed[1:B + 1], np.histogram(x, bins=B, range=(np.float64(lo), np.float64(hi)))[0])
            assert o[key][c][0] == (field < lo).sum() and o[key][c][B + 1] == (field > hi).sum()
    print(f"{shape} B = {B}: {moved} of {total} pixels sit in another bin in fp32 ({moved / total:.1e})")
    assert moved <= 1e-4 * total
    assert (o["hist_truth"][:, 0] == 0).all() and (o["hist_truth"][:, B + 1] == 0).all()
    assert (o["count"] == shape[1] * shape[2]).all()


def test_a_field_against_itself():
    _, truth = white((2, 60, 70))
    o = do.distribution(truth, truth, bins=64, joint=8)
    assert (o["pss"] == 1.0).all() and (o["w1"] == 0.0).all() and (o["q_bias"] == 0.0).all()
    assert (o["under"] == 0.0).all() and (o["over"] == 0.0).all()
    off = o["joint"].copy()
    off[:, np.arange(8), np.arange(8)] = 0
    assert (off == 0).all() and (o["joint"].sum((1, 2)) == o["count"]).all()


def test_a_shift_by_m_bin_widths_has_w1_m_w():
    rng = np.random.default_rng(1)
    truth = (rng.integers(10, 40, (1, 50, 60)) + 0.5).astype(np.float32)  # bin centres of a (0, 64) range, B = 64
    for m in (1, 3, 7):
        o = do.distribution(truth + np.float32(m), truth, bins=64, joint=0, value_range=(0.0, 64.0))
        assert o["w1"][0] == float(m)  # w = 1, and the integer sum is m N
        assert np.array_equal(o["hist_pred"][0][m:], o["hist_truth"][0][:66 - m])
        assert np.allclose(o["q_bias"][0], m, rtol=0, atol=1e-12)
    o = do.distribution(truth * np.float32(0.5), truth * np.float32(0.5), bins=64, joint=0, value_range=(0.0, 32.0))
    assert o["w1"][0] == 0.0


def test_shrinking_toward_the_mean_shows_in_q_bias():
    pred, truth = white((1, 200, 200))
    mean = truth.mean(dtype=np.float64)
    smooth = (mean + 0.7 * (truth - mean)).astype(np.float32)
    o = do.distribution(smooth, truth, probs=(0.01, 0.5, 0.99))
    print("q_bias of a field shrunk to 0.7:", o["q_bias"][0])
    assert o["q_bias"][0, 0] > 0.5 and o["q_bias"][0, 2] < -0.5 and abs(o["q_bias"][0, 1]) < 0.05
    assert o["pss"][0] < 0.9 and o["under"][0] == 0 and o["over"][0] == 0


def test_quantiles_agree_with_numpy_to_a_bin_width():
    pred, truth = white((2, 150, 170))
    for B in (16, 256):
        o = do.distribution(pred, truth, bins=B)
        for c in range(2):
            w = (float(o["hi"][c]) - float(o["lo"][c])) / B
            for key, field in (("q_pred", pred[c]), ("q_truth", truth[c])):
                want = np.quantile(field.astype(np.float64), do.DEFAULT_PROBS)
                assert np.abs(o[key][c] - want).max() <= w, (B, c, key)


def test_contingency_is_a_direct_count_at_a_bin_edge():
    rng = np.random.default_rng(2)
    truth = (64.0 * rng.random((2, 80, 90))).astype(np.float32)
    pred = (truth + 4.0 * rng.standard_normal(truth.shape)).astype(np.float32)  # leaves (0, 64) on both sides
    pred[0, 5, 5] = np.nan
    truth[1, 7, 7] = np.inf
    o = do.distribution(pred, truth, bins=64, joint=32, value_range=(0.0, 64.0))
    for k in (1, 10, 31):
        thr = np.float32(2.0 * k)  # the lower edge of joint bin k: the scale 0.5 is exact
        t = contingency(o["joint"], k)
        for c in range(2):
            used = np.isfinite(pred[c]) & np.isfinite(truth[c])
            ea, eb = pred[c][used] >= thr, truth[c][used] >= thr
            assert t["hits"][c] == (ea & eb).sum() and t["misses"][c] == (~ea & eb).sum()
            assert t["false_alarms"][c] == (ea & ~eb).sum() and t["correct_negatives"][c] == (~ea & ~eb).sum()
            assert t["csi"][c] == (ea & eb).sum() / float((ea | eb).sum())
            assert t["bias"][c] == ea.sum() / float(eb.sum())
    for bad in (0, 32):
        with pytest.raises(ValueError):
            contingency(o["joint"], bad)
    with pytest.raises(ValueError):
        contingency(np.zeros((2, 3, 4)), 1)


def test_the_mask_and_a_channel_without_a_used_pixel():
    pred, truth = (v.copy() for v in white((2, 40, 50)))
    base = do.distribution(pred, truth, bins=32, joint=4)
    pred[0, 3, 4] = np.nan
    truth[0, 9, 9] = -np.inf
    truth[0, 10:20, 10:30] = np.nan
    pred[1] = np.nan
    o = do.distribution(pred, truth, bins=32, joint=4)
    assert o["count"][0] == 40 * 50 - 202 and o["count"][1] == 0
    for key in ("hist_pred", "hist_truth"):
        assert o[key][0].sum() == o["count"][0] and (o[key][1] == 0).all()
    assert o["joint"][0].sum() == o["count"][0] and (o["joint"][1] == 0).all()
    assert np.isnan(o["derived"][1]).all() and np.isnan(o["lo"][1]) and np.isnan(o["hi"][1])
    assert np.isfinite(o["derived"][0]).all()
    used = np.isfinite(pred[0]) & np.isfinite(truth[0])
    assert o["lo"][0] == truth[0][used].min() and o["hi"][0] == truth[0][used].max()
    assert base["count"][0] == 2000


def test_a_constant_truth_and_a_narrow_range():
    truth = np.full((1, 20, 30), 5.0, dtype=np.float32)
    pred = truth.copy()
    pred[0, :5] = 4.0
    pred[0, 5:7] = 6.0
    o = do.distribution(pred, truth, bins=8, joint=2)
    want = np.zeros(10, dtype=np.int64)
    want[0], want[8], want[9] = 150, 390, 60
    assert np.array_equal(o["hist_pred"][0], want) and o["hist_truth"][0][8] == 600
    assert o["under"][0] == 0.25 and o["over"][0] == 0.1
    pred, truth = white((1, 50, 60))
    o = do.distribution(pred, truth, bins=16, value_range=(289.0, 291.0))
    assert o["hist_truth"][0][0] == (truth < 289).sum() > 0 and o["hist_truth"][0][17] == (truth > 291).sum() > 0
    assert o["lo"][0] == 289 and o["hi"][0] == 291


def test_bin_edges():
    e = bin_edges(np.float32([0.0, 290.0]), np.float32([64.0, 293.0]), 64)
    assert e.shape == (2, 67) and e.dtype == np.float64
    assert np.array_equal(e[0], np.arange(-1.0, 66.0))
    assert e[1, 1] == 290.0 and e[1, 65] == 293.0 and np.allclose(np.diff(e[1]), 3.0 / 64, rtol=1e-9)


def test_the_result_file_round_trip(tmp_path):
    pred, truth = (v.copy() for v in white((2, 40, 50)))
    pred[1, :3] = np.nan
    for joint, probs in ((8, do.DEFAULT_PROBS), (0, ())):
        o = do.distribution(pred, truth, bins=32, joint=joint, probs=probs)
        o["hist_pred"] = o["hist_pred"].copy()
        o["hist_pred"][0, 1] += 2 ** 40  # a count no float32 holds
        path = save_distribution(str(tmp_path / f"d{joint}.nc"), o, ["SST", "SSS"], probs)
        back, names, pr = load_distribution(path)
        assert names == ["SST", "SSS"] and np.array_equal(pr, np.asarray(probs, dtype=np.float64))
        for k in ("hist_pred", "hist_truth", "joint", "count"):
            assert back[k].dtype == np.int64 and np.array_equal(back[k], o[k]), k
        for k in ("lo", "hi", "pss", "w1", "under", "over", "q_pred", "q_truth", "q_bias"):
            assert back[k].dtype == o[k].dtype and np.array_equal(back[k], o[k], equal_nan=True), k
        assert np.array_equal(back["edges"], bin_edges(o["lo"], o["hi"], 32))
    with pytest.raises(ValueError):
        save_distribution(str(tmp_path / "bad.nc"), {"pss": o["pss"]}, ["SST", "SSS"], ())
    with pytest.raises(ValueError):
        save_distribution(str(tmp_path / "bad.nc"), o, ["SST"], ())
