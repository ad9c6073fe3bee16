"""Host-side checks of the overlapped tiling plan (srmi.superres.overlap_plan, the
library's srmi_overlap_count), the integer blend weights, and the fp64 oracle of the
cut and the blend (tests/overlap_oracle.py) that the GPU tests compare against."""
import numpy as np
import pytest

import overlap_oracle as oo
from srmi.superres import blend_weight, lib_overlap_count, overlap_count, overlap_plan

# the issue's five plus: a stride of 1, a prime length, the bench's two plans and the
# floor grid's 4096 / 192
PLANS = [(54, 16, 12), (40, 16, 12), (40, 16, 16), (16, 16, 16), (48, 16, 16), (41, 16, 5), (55, 16, 7), (17, 16, 1),
         (160, 64, 48), (216, 64, 48), (1024, 48, 40), (1024, 48, 48), (4096, 192, 192), (5, 1, 1)]


@pytest.mark.parametrize("L,t,S", PLANS)
def test_plan_covers_the_axis(L, t, S):
    o = overlap_plan(L, t, S)
    n = -((t - L) // S) + 1  # ceil((L - t) / S) + 1
    assert len(o) == n == overlap_count(L, t, S) == lib_overlap_count(L, t, S)
    assert o[0] == 0 and o[-1] == L - t
    assert all(b > a for a, b in zip(o, o[1:]))
    assert list(oo.origins(L, t, S)) == o
    cover = oo.cover_count(L, t, S)
    assert cover.min() >= 1
    # the shifted last tile may add a third cover at S > t / 2, never a fourth
    assert cover.max() <= -(-t // S) + 1


def test_plan_triple_cover_case():
    assert overlap_plan(54, 16, 12) == [0, 12, 24, 36, 38]
    cover = oo.cover_count(54, 16, 12)
    assert cover[38] == 3 and cover[39] == 3
    assert list(np.flatnonzero(cover == 3)) == [38, 39]
    assert overlap_plan(1024, 48, 40)[-2:] == [960, 976] and len(overlap_plan(1024, 48, 40)) == 26
    assert len(overlap_plan(1024, 48, 48)) == 22


@pytest.mark.parametrize("L,t,S", [(15, 16, 12), (40, 16, 0), (40, 16, -3), (40, 16, 17), (0, 0, 0), (40, 0, 0)])
def test_plan_errors(L, t, S):
    with pytest.raises(ValueError):
        overlap_plan(L, t, S)
    with pytest.raises(ValueError):
        lib_overlap_count(L, t, S)
    with pytest.raises(ValueError):
        oo.origins(L, t, S)


@pytest.mark.parametrize("t,S", [(16, 12), (16, 16), (16, 8), (16, 5), (64, 48), (7, 4), (1, 1)])
def test_weights(t, S):
    R = t - S
    w = [blend_weight(p, t, S) for p in range(t)]
    assert all(isinstance(v, int) and 1 <= v <= R + 1 for v in w)
    assert w == list(oo.weights(t, S)) and w == w[::-1]
    if R == 0:
        assert w == [1] * t
    # two regularly overlapping tiles (origins 0 and S): position S + q of the first
    # meets position q of the second, and the two weights sum to R + 1 across the ramp
    if 2 * R <= t:
        for q in range(R):
            assert (w[S + q], w[q]) == (R - q, q + 1)
    with pytest.raises(ValueError):
        blend_weight(t, t, S)


@pytest.mark.parametrize("shape,tile,stride", [((2, 40, 54), (16, 16), (12, 12)), ((1, 41, 55), (16, 16), (5, 7)),
                                               ((2, 40, 54), (16, 16), (16, 16))])
@pytest.mark.parametrize("mode", [oo.LNORM, oo.LSCALE])
def test_oracle_reconstruction(shape, tile, stride, mode):
    """cut + norm + denorm + blend of a random region returns the region (fp64): every
    covering tile de-normalises to the region's own value, and a weighted mean of equal
    values is that value."""
    rng = np.random.RandomState(5)
    region = rng.randn(*shape) * 3 + 1
    tiles, off, div, bad = oo.cut(region, *tile, *stride, mode)
    assert not bad.any()
    out, M = oo.blend(tiles, off, div, bad, *stride, *shape[1:])
    np.testing.assert_allclose(out, region, rtol=1e-12, atol=1e-12 * np.abs(region).max())
    assert (M >= np.abs(region) * (1 - 1e-12)).all()


def test_oracle_bad_tile_leaves_exactly_its_own_pixels():
    """The 8 x 8 patch at rows 16..23, columns 28..35 of the 40 x 54 plan lies in tile
    (1, 2) alone, and in the part of it no other tile covers."""
    rng = np.random.RandomState(6)
    region = rng.randn(1, 40, 54) * 3 + 1
    region[0, 16:24, 28:36] = np.nan
    tiles, off, div, bad = oo.cut(region, 16, 16, 12, 12, oo.LNORM)
    assert list(np.flatnonzero(bad)) == [1 * 5 + 2]
    out, _ = oo.blend(tiles, off, div, bad, 12, 12, 40, 54)
    assert int(np.isnan(out).sum()) == 64 and np.isnan(out[0, 16:24, 28:36]).all()
    ok = ~np.isnan(out)
    np.testing.assert_allclose(out[ok], region[ok], rtol=1e-12, atol=1e-11)


@pytest.mark.parametrize("losses", [None, {"model": 0.25, "interpolated": 0.5}])
def test_superres_results_round_trip(tmp_path, losses):
    """The three images of super_resolve through the netCDF-3 result writer: one file
    per variable, 'input' on ys / xs, no 'target', NaN pixels kept."""
    from functools import partial
    from srmi import results as R
    rng = np.random.RandomState(3)
    C, h, w, s = 2, 40, 54, 4
    images = {"input": rng.randn(C, h, w).astype(np.float32),
              "interpolated": rng.randn(C, h * s, w * s).astype(np.float32),
              "model": rng.randn(C, h * s, w * s).astype(np.float32)}
    images["model"][1, 64:96, 112:144] = np.nan  # pixels whose tiles were all bad
    names = ["SSS", "SST"]
    path_for = partial(R.results_path, str(tmp_path), "swot", "superres-48", timestep=0, structure="image")
    paths = R.save_superres_results(lambda v: path_for(varname=v), images, names, losses)
    assert [p.rsplit("/", 1)[1] for p in paths] == ["SSS-0.image.nc", "SST-0.image.nc"]
    for iv, p in enumerate(paths):
        back, bl = R.load_inference_results(p)
        assert bl == (losses or {})
        assert sorted(back) == ["input", "interpolated", "model"]
        assert back["input"].values.shape == (h, w) and back["model"].values.shape == (h * s, w * s)
        for k, v in images.items():
            np.testing.assert_array_equal(back[k].values, v[iv].astype(np.float64))
        np.testing.assert_allclose(back["model"].coords["y"], np.arange(0.0, 100.0, 100.0 / (h * s)))
    with pytest.raises(ValueError):
        R.save_superres_results(lambda v: path_for(varname=v), {"model": images["model"]}, names)


def test_new_symbols_are_bound():
    from srmi import _lib
    lib = _lib.load()
    for name in ("srmi_overlap_count", "srmi_region_to_tiles_overlap", "srmi_tiles_blend"):
        assert name in _lib.EXPORTED and hasattr(lib, name)
    # bad scalars never reach a launch: they are refused before any device call
    P = [None] * 7
    assert lib.srmi_region_to_tiles_overlap(None, 1, 40, 54, 16, 16, 17, 12, 0, *P) == _lib.SRMI_ERR_ARG
    assert lib.srmi_region_to_tiles_overlap(None, 1, 40, 54, 16, 16, 12, 12, 3, *P) == _lib.SRMI_ERR_ARG
    assert lib.srmi_region_to_tiles_overlap(None, 1, 40, 54, 16, 16, 12, 12, 0, *P) == _lib.SRMI_ERR_ARG  # NULL buffers
    assert lib.srmi_tiles_blend(None, None, None, None, 1, 16, 16, 0, 12, 40, 54, None, None) == _lib.SRMI_ERR_ARG
    assert lib.srmi_tiles_blend(None, None, None, None, 1, 16, 16, 12, 12, 40, 54, None, None) == _lib.SRMI_ERR_ARG
