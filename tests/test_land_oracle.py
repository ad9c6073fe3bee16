"""Host-side checks of the land-aware oracle (tests/land_oracle.py) the GPU tests compare
against -- the flood fill's own properties, the float32 bit model against the float64
fill, the masked cut, blend and RMSE -- and of the three new entry points' binding and
argument refusals (no launch, so no GPU is needed)."""
import os

import numpy as np
import pytest

import land_oracle as lo
import overlap_oracle as oo


# ------------------------------------------------------------------- the fill
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fill_properties(dtype):
    planes = lo.coast_planes()
    assert len(planes) > 10
    seen = 0
    for plane, wet in planes:
        f, stamp, passes = lo.fill(plane, wet, dtype)
        w = plane[wet].astype(dtype)
        # wet pixels untouched, everything filled and finite
        assert f.dtype == dtype and (f[wet] == w).all() and np.isfinite(f).all() and (stamp >= 0).all()
        # a mean of means of wet values: inside their hull, up to the roundings of 8 adds and a multiply
        slack = 16 * np.finfo(dtype).eps * np.abs(w).max()
        assert f.min() >= w.min() - slack and f.max() <= w.max() + slack
        # pass j fills exactly the pixels at Chebyshev distance j from the wet set
        dist = lo.chebyshev_to_wet(wet)
        assert (stamp == dist).all() and passes == dist.max() <= max(plane.shape) - 1
        seen = max(seen, passes if plane.shape == (16, 16) else 0)
    assert seen == 15  # the single wet corner of a 16 x 16 plane: the most a plane of that size can need


def test_fill_leaves_an_all_wet_plane_alone():
    rng = np.random.RandomState(1)
    plane = rng.randn(16, 16).astype(np.float32)
    for dtype in (np.float32, np.float64):
        f, stamp, passes = lo.fill(plane, np.ones((16, 16), bool), dtype)
        assert passes == 0 and (stamp == 0).all() and (f == plane).all()
    with pytest.raises(ValueError):
        lo.fill(plane, np.zeros((16, 16), bool))


def test_fill_is_jacobi_and_ordered():
    """A 1 x 4 row with one wet end fills one pixel per pass with the same value; a dry
    pixel between two wet ones takes fp32(fp32(a + b) * 0.5), left neighbour first."""
    f, stamp, passes = lo.fill(np.array([[3.0, 0, 0, 0]], np.float32), np.array([[True, False, False, False]]))
    assert passes == 3 and list(stamp[0]) == [0, 1, 2, 3] and (f == 3.0).all()
    a, b = np.float32(1.0000001), np.float32(3.0000002)
    f, _, _ = lo.fill(np.array([[a, 0, b]], np.float32), np.array([[True, False, True]]))
    assert f[0, 1] == np.float32(np.float32(a + b) * np.float32(0.5))
    # three neighbours: the table's fp32 1/3, not a division
    plane = np.array([[1.0, 0.1, 0.7], [0, 0, 0]], np.float32)
    f, _, _ = lo.fill(plane, np.array([[True, True, True], [False, False, False]]))
    s = np.float32(np.float32(np.float32(0) + plane[0, 0]) + plane[0, 1])
    s = np.float32(s + plane[0, 2])
    assert f[1, 1] == np.float32(s * lo.RECIP[2])


def test_fill_f32_stays_close_to_f64():
    """The bit model against the float64 fill, on the planes the GPU tests use (the
    normalised tiles of coast_region in every mode) and on larger coast planes: within
    16 * 2^-24 * max |wet value| -- a filled value is a convex combination of wet values
    reached through at most 8 adds and a multiply per pass, and the error of a pass is
    averaged, not amplified, by the next."""
    planes = list(lo.coast_planes())
    region = lo.coast_region().astype(np.float64)
    wet = lo.wet_tiles(region, 16, 16, 12, 12)
    rng = np.random.RandomState(2)
    off, div = rng.randn(15, 2) * 0.5 + 1, rng.rand(15, 2) * 2 + 2
    for mode in (lo.LNORM, lo.LSCALE, lo.AFFINE):
        norm, _, _, bad, nwet = lo.cut(region, 16, 16, 12, 12, mode, 1, off, div)
        planes += [(norm[k, c].astype(np.float32), wet[k, c]) for k in range(15) for c in range(2)
                   if not bad[k] and np.isfinite(norm[k, c][wet[k, c]]).all()]
    worst = 0.0
    for plane, w in planes:
        f32, _, p32 = lo.fill(plane, w, np.float32)
        f64, _, p64 = lo.fill(plane.astype(np.float64), w, np.float64)
        scale = np.abs(plane[w]).max()
        assert p32 == p64
        worst = max(worst, float(np.abs(f32 - f64).max() / scale))
        assert np.abs(f32 - f64).max() <= 16 * 2.0 ** -24 * scale
    print(f"fill f32 vs f64: worst error / max|wet| = {worst:.3g} over {len(planes)} planes (bar {16 * 2.0 ** -24:.3g})")


# ------------------------------------------------------------ cut, blend, rmse
def test_cut_of_the_coast_region():
    region = lo.coast_region().astype(np.float64)
    norm, o, d, bad, nwet = lo.cut(region, 16, 16, 12, 12, lo.LNORM, 1)
    assert list(np.flatnonzero(bad)) == [13, 14]  # tile (2, 3) through channel 1, the all-land tile (2, 4)
    assert list(nwet[0]) == [1, 1] and list(nwet[13]) == [32, 0] and list(nwet[14]) == [0, 0]
    assert (norm[13] == 0).all() and (norm[14] == 0).all()
    wet = lo.wet_tiles(region, 16, 16, 12, 12)
    assert (nwet == wet.sum(axis=(2, 3))).all()
    for k in range(1, 13):
        for c in range(2):
            w = norm[k, c][wet[k, c]]
            assert abs(w.mean()) < 1e-12 and abs(w.std() - 1) < 1e-12 and np.isnan(norm[k, c][~wet[k, c]]).all()
    _, passes = lo.fill_tiles(norm, wet, bad, np.float64)
    assert passes[0].tolist() == [15, 15] and passes.max() == 15
    # a larger min_wet drops the thin tiles too
    assert list(np.flatnonzero(lo.cut(region, 16, 16, 12, 12, lo.LSCALE, 40)[3])) == [0, 13, 14]
    # without land: overlap_oracle.cut
    full = np.random.RandomState(3).randn(2, 40, 54) * 3 + 1
    for mode in (lo.LNORM, lo.LSCALE):
        got, ref = lo.cut(full, 16, 16, 12, 12, mode, 256), oo.cut(full, 16, 16, 12, 12, mode)
        for g, r in zip(got[:4], ref):
            np.testing.assert_allclose(g, r, rtol=1e-13, atol=1e-13)
        assert (got[4] == 256).all()


def test_blend_masks_exactly_the_upsampled_dry_set():
    rng = np.random.RandomState(4)
    region = lo.coast_region().astype(np.float64)
    tiles = rng.randn(15, 2, 64, 64)
    off, div = rng.randn(15, 2), rng.rand(15, 2) + 0.5
    plain, _ = oo.blend(tiles, off, div, None, 48, 48, 160, 216)
    out, _ = lo.blend(tiles, off, div, None, 48, 48, 160, 216, region, 4)
    dry = lo.dry_hr(region, 4)
    assert dry.shape == out.shape and dry[0, 83, 120] and dry[0, 80:84, 120:124].all() and not dry[0, 84, 120]
    assert (np.isnan(out) == dry).all() and (out[~dry] == plain[~dry]).all()
    assert int(dry.sum()) == 16 * int(np.isnan(region).sum())


def test_rmse_masked():
    rng = np.random.RandomState(5)
    p, t = rng.randn(1000), rng.randn(1000)
    p[::7] = np.nan
    t[::5] = np.inf
    loss, count = lo.rmse(p, t)
    keep = [i for i in range(1000) if i % 7 and i % 5]
    assert count == len(keep) and abs(loss - np.sqrt(np.mean((p[keep] - t[keep]) ** 2))) < 1e-14
    loss, count = lo.rmse(np.full(4, np.nan), np.zeros(4))
    assert count == 0 and np.isnan(loss)


# -------------------------------------------------------------------- the ABI
def test_land_symbols_are_bound():
    from srmi import _lib
    lib = _lib.load()
    names = ("srmi_region_to_tiles_overlap_masked", "srmi_tiles_blend_masked", "srmi_rmse_partial_masked")
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "srmi.h")) as f:
        header = f.read()
    for name in names:
        assert name in _lib.EXPORTED and hasattr(lib, name) and f"int {name}(" in header
    # bad scalars never reach a launch: they are refused before any device call
    E = _lib.SRMI_ERR_ARG
    cut, blend = lib.srmi_region_to_tiles_overlap_masked, lib.srmi_tiles_blend_masked
    P6 = [None] * 6
    assert cut(None, 1, 40, 54, 16, 16, 12, 12, 0, *P6, 0, None, None) == E  # min_wet = 0
    assert cut(None, 1, 40, 54, 16, 16, 12, 12, 0, *P6, -3, None, None) == E
    assert cut(None, 1, 40, 54, 16, 16, 17, 12, 0, *P6, 1, None, None) == E  # the plan
    assert cut(None, 1, 40, 54, 16, 16, 12, 12, 3, *P6, 1, None, None) == E  # the mode
    assert cut(None, 1, 40, 54, 16, 16, 12, 12, 0, *P6, 1, None, None) == E  # NULL buffers
    P4 = [None] * 4
    assert blend(*P4, 1, 16, 16, 12, 12, 40, 54, None, 0, None, None) == E  # scale = 0
    assert blend(*P4, 1, 16, 16, 12, 12, 40, 54, None, 4, None, None) == E  # Wo % scale != 0 (and NULL)
    assert blend(*P4, 1, 16, 16, 12, 12, 40, 56, None, 3, None, None) == E  # Ho % scale != 0
    assert blend(*P4, 1, 16, 16, 0, 12, 40, 56, None, 4, None, None) == E  # the plan
    assert blend(*P4, 1, 16, 16, 12, 12, 40, 56, None, 4, None, None) == E  # NULL buffers
    assert lib.srmi_rmse_partial_masked(None, None, None, 16, None, None) == E


def test_land_option_is_declared():
    """RegionSuperResolver takes land / min_wet, off by default."""
    import inspect
    from srmi.superres import RegionSuperResolver
    sig = inspect.signature(RegionSuperResolver.__init__).parameters
    assert sig["land"].default is False and sig["min_wet"].default == 0.25
