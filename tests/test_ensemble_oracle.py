"""The self-ensemble oracle (tests/ensemble_oracle.py) against the reference's recorded
xyflip outputs and against the plain blend oracle, and srmi.superres.ensemble_variants
(pure host code).  No GPU."""
import os

import numpy as np
import pytest

import ensemble_oracle as eo
import overlap_oracle as oo
from srmi.superres import ensemble_variants

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "xyflip.npz")


def test_dihedral_is_the_recorded_xyflip():
    z = np.load(GOLDEN)
    for f in range(8):
        assert int(z[f"attr{f}"]) == f
        assert np.array_equal(eo.dihedral(z["input"], f), z[f"flip{f}"]), f


@pytest.mark.parametrize("shape", [(2, 3, 8, 8), (3, 5, 7), (6, 6)])
def test_undo_inverts_dihedral(shape):
    x = np.random.RandomState(61).randn(*shape)
    for f in range(8 if shape[-1] == shape[-2] else 4):
        v = eo.dihedral(x, f)
        assert v.shape == x.shape and np.array_equal(eo.undo(v, f), x), f
    if shape[-1] != shape[-2]:  # a swap of a rectangular plane changes its shape
        assert eo.dihedral(x, 4).shape[-2:] == shape[:-3:-1]


def test_variants_of_and_expand():
    assert eo.variants_of(0b10010001) == (0, 4, 7) and eo.variants_of(1) == (0,) and len(eo.variants_of(255)) == 8
    for bad in (0, 256, -1):
        with pytest.raises(ValueError):
            eo.variants_of(bad)
    x = np.random.RandomState(62).randn(3, 6, 6)
    e = eo.expand(x, 0b10010001)
    assert e.shape == (3, 3, 6, 6) and np.array_equal(e[0], x) and np.array_equal(e[2], eo.dihedral(x, 7))


@pytest.mark.parametrize("with_mask", [False, True])
def test_identical_variants_give_the_plain_blend_and_no_spread(with_mask):
    rng = np.random.RandomState(63)
    hw, T, S = (40, 56), 16, 12
    n = len(oo.origins(hw[0], T, S)) * len(oo.origins(hw[1], T, S))
    tiles = rng.randn(n, 2, T, T)
    off, div = rng.randn(n, 2), rng.rand(n, 2) + 0.5
    bad = (rng.rand(n) < 0.3).astype(np.int32)
    mask = None
    if with_mask:
        mask = rng.randn(2, 10, 14)
        mask[0, 3, 4] = mask[1, 9, 13] = np.nan
    ref, M = oo.blend(tiles, off, div, bad, S, S, *hw)
    if with_mask:
        ref = np.where(np.repeat(np.repeat(np.isnan(mask), 4, 1), 4, 2), np.nan, ref)
    for vmask in (1, 0b1111, 0b10010001, 255):
        mean, spread, Me = eo.blend_ensemble(eo.expand(tiles, vmask), vmask, off, div, bad, S, S, *hw, mask=mask,
                                             scale=4)
        nan = np.isnan(ref)
        assert nan.any() and (np.isnan(mean) == nan).all() and (np.isnan(spread) == nan).all()
        # the mean of K equal float64 values: a few roundings of the sum
        np.testing.assert_allclose(mean[~nan], ref[~nan], rtol=1e-15, atol=1e-15)
        assert np.abs(spread[~nan]).max() <= 1e-14 and np.array_equal(Me, M)


def test_independent_slabs_have_the_mean_and_std_of_their_blends():
    rng = np.random.RandomState(64)
    hw, T, S = (40, 54), 16, 12
    n = len(oo.origins(hw[0], T, S)) * len(oo.origins(hw[1], T, S))
    tiles = rng.randn(3, n, 1, T, T)
    var = (0, 3, 6)
    mean, spread, M = eo.blend_ensemble(tiles, var, None, None, None, S, S, *hw)
    each = np.stack([oo.blend(eo.undo(tiles[j], f), None, None, None, S, S, *hw)[0] for j, f in enumerate(var)])
    np.testing.assert_allclose(mean, each.mean(0), rtol=1e-14)
    np.testing.assert_allclose(spread, each.std(0), rtol=1e-12)
    assert (spread > 0).all() and (M >= np.abs(each).max(0) - 1e-12).all()


def superres_results_round_trip(tmp_path, images, names):
    """save_superres_results of ``images`` (numpy or device tensors, 'spread' among them):
    'spread' comes back as a fourth variable on the axes of 'model', NaN kept, and without
    it -- whatever else the dict holds -- the file is, byte for byte, the one the
    three-image dict gives."""
    from functools import partial
    from srmi import results as R

    def arr(x):
        return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)

    def path_for(sub):
        return partial(R.results_path, str(tmp_path / sub), "swot", "superres-48", timestep=0, structure="image")

    paths = R.save_superres_results(lambda v: path_for("spread")(varname=v), images, names, {"model": 0.25})
    for iv, p in enumerate(paths):
        back, bl = R.load_inference_results(p)
        assert bl == {"model": 0.25} and sorted(back) == ["input", "interpolated", "model", "spread"]
        for k in ("input", "interpolated", "model", "spread"):
            np.testing.assert_array_equal(back[k].values, arr(images[k])[iv].astype(np.float64))
        assert back["spread"].dims == back["model"].dims == ("y", "x")
        np.testing.assert_array_equal(back["spread"].coords["y"], back["model"].coords["y"])
    three = {k: images[k] for k in ("input", "interpolated", "model")}
    others = dict(three, nwet=np.zeros((4, len(names)), np.int32))
    pa = R.save_superres_results(lambda v: path_for("three")(varname=v), three, names, {"model": 0.25})
    pb = R.save_superres_results(lambda v: path_for("others")(varname=v), others, names, {"model": 0.25})
    for a, b, c in zip(pa, pb, paths):
        assert open(a, "rb").read() == open(b, "rb").read() != open(c, "rb").read()
        assert sorted(R.load_inference_results(a)[0]) == ["input", "interpolated", "model"]


def test_superres_results_round_trip_with_spread(tmp_path):
    rng = np.random.RandomState(65)
    C, h, w, s = 2, 20, 27, 4
    images = {"input": rng.randn(C, h, w).astype(np.float32),
              "interpolated": rng.randn(C, h * s, w * s).astype(np.float32),
              "model": rng.randn(C, h * s, w * s).astype(np.float32),
              "spread": rng.rand(C, h * s, w * s).astype(np.float32)}
    images["model"][1, 32:48, 56:72] = images["spread"][1, 32:48, 56:72] = np.nan
    superres_results_round_trip(tmp_path, images, ["SSS", "SST"])


def test_ensemble_variants():
    assert ensemble_variants(1, (48, 48)) == (0,)
    assert ensemble_variants(4, (48, 48)) == (0, 1, 2, 3) == ensemble_variants(4, (16, 32))
    assert ensemble_variants(8, (32, 32)) == tuple(range(8))
    assert ensemble_variants((3, 0), (16, 32)) == (0, 3)
    assert ensemble_variants([7, 0, 4], (32, 32)) == (0, 4, 7)
    assert ensemble_variants(np.int64(4), (32, 32)) == (0, 1, 2, 3)  # numpy integers count as integers
    assert ensemble_variants(np.array([2, 0]), (16, 32)) == (0, 2)
    for bad in (0, 2, 3, 16, -1, 1.0, "8", None, True, (), (1, 2), (0, 0), (0, 8), (0, -1), (0, 1.5)):
        with pytest.raises(ValueError):
            ensemble_variants(bad, (32, 32))
    for e in (8, (0, 4), [0, 1, 7]):
        with pytest.raises(ValueError, match=r"\(16, 32\).*ensemble=4"):
            ensemble_variants(e, (16, 32))
