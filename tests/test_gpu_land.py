"""The land-aware forms on the HIP path: the masked cut with its flood fill
(srmi_region_to_tiles_overlap_masked), the re-masking blend (srmi_tiles_blend_masked),
the masked RMSE (srmi_rmse_partial_masked) and RegionSuperResolver(land=True) end to end,
against the unmasked kernels (bit for bit where no land is involved) and the numpy oracle
(tests/land_oracle.py).

Bars, derived, not measured.  off_out / div_out: one rounding of an fp64 result, plus an
ulp for the fp64 reduction order: 2 * 2^-24 relative.  Wet pixels of a tile: the fp64
(x - off) * (1 / div) rounded once, next to the oracle's division: 4 * 2^-24 *
max(1, |value|).  Dry pixels: the float32 bit model of the fill run from the device's own
wet values -- bit for bit.  The blend: overlap's 16 * 2^-24 * M."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import land_oracle as lo  # noqa: E402
import overlap_oracle as oo  # noqa: E402
from srmi import _lib  # noqa: E402
from srmi._lib import call, ptr  # noqa: E402
from srmi.engine import Engine, upsample  # noqa: E402
from srmi.superres import RegionSuperResolver, overlap_count  # noqa: E402
from test_gpu_inference import _small_rcan  # noqa: E402
from test_gpu_overlap import TILE, _affine, _field, assert_blend_close, bits, blend_dev, cut_dev, dev, f64, st  # noqa: E402

U = 2.0 ** -24
MODES = [lo.LNORM, lo.LSCALE, lo.AFFINE]


def cut_masked_dev(region, ty, tx, sy, sx, mode, min_wet, off=None, div=None):
    """srmi_region_to_tiles_overlap_masked of a numpy region -> device (tiles, off_out,
    div_out, bad, nwet), the outputs pre-filled as test_gpu_overlap.cut_dev's."""
    d = dev()
    C, H, W = region.shape
    n = overlap_count(H, ty, sy) * overlap_count(W, tx, sx)
    rg = torch.tensor(region, device=d)
    tiles = torch.full((n, C, ty, tx), -7.0, device=d)
    o_in = torch.tensor(off, device=d) if off is not None else None
    d_in = torch.tensor(div, device=d) if div is not None else None
    o_out = o_in.clone() if o_in is not None else torch.full((n, C), -7.0, device=d)
    d_out = d_in.clone() if d_in is not None else torch.full((n, C), -7.0, device=d)
    bad = torch.full((n,), 5, dtype=torch.int32, device=d)
    nwet = torch.full((n, C), -1, dtype=torch.int32, device=d)
    call("srmi_region_to_tiles_overlap_masked", ptr(rg), C, H, W, ty, tx, sy, sx, mode, ptr(o_in), ptr(d_in), ptr(tiles),
         ptr(o_out), ptr(d_out), ptr(bad), int(min_wet), ptr(nwet), st())
    return tiles, o_out, d_out, bad, nwet


def blend_masked_dev(tiles, off, div, bad, C, Ty, Tx, Sy, Sx, Ho, Wo, mask, scale):
    out = torch.full((C, Ho, Wo), -7.0, device=tiles.device)
    call("srmi_tiles_blend_masked", ptr(tiles), ptr(off), ptr(div), ptr(bad), C, Ty, Tx, Sy, Sx, Ho, Wo, ptr(mask),
         scale, ptr(out), st())
    return out


def same_bits_or_nan(a, b):
    """float32 arrays: equal bit for bit, any NaN standing for any NaN."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    nan = np.isnan(a)
    return bool((nan == np.isnan(b)).all() and (a.view(np.int32)[~nan] == b.view(np.int32)[~nan]).all())


# ------------------------------------------------------------------ 1. cut, identity
# W = 56: the float4 forms of both cuts; W = 54 / stride 5 x 7: the scalar ones
@pytest.mark.parametrize("hw,stride", [((40, 56), (12, 12)), ((40, 54), (12, 12)), ((41, 55), (5, 7))])
@pytest.mark.parametrize("mode", [lo.LSCALE, lo.AFFINE])
@pytest.mark.parametrize("min_wet", [1, 256])
def test_cut_without_land_is_the_unmasked_cut(hw, stride, mode, min_wet):
    rng = np.random.RandomState(31)
    region = (rng.randn(2, *hw) * 3 + 1).astype(np.float32)
    n = overlap_count(hw[0], 16, stride[0]) * overlap_count(hw[1], 16, stride[1])
    off, div = _affine(rng, n, 2) if mode == lo.AFFINE else (None, None)
    got = cut_masked_dev(region, 16, 16, *stride, mode, min_wet, off, div)
    ref = cut_dev(region, 16, 16, *stride, mode, off, div)
    for g, r, what in zip(got, ref, ("tiles", "off_out", "div_out", "bad")):
        assert torch.equal(bits(g), bits(r)), what
    assert int(got[3].sum()) == 0 and (got[4] == 256).all()


# ---------------------------------------------------------------------- 2. cut, fill
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("min_wet", [1, 40])
def test_cut_fills_the_dry_pixels(mode, min_wet):
    """lo.coast_region: a coast across several tiles, an isolated dry pixel, a lake in the
    land, a tile with one wet corner pixel (15 passes, and in the tile-local modes the IEEE
    NaN of a zero spread), an all-land tile, a tile bad through its other channel."""
    region = lo.coast_region()
    rng = np.random.RandomState(32)
    off, div = _affine(rng, 15, 2) if mode == lo.AFFINE else (None, None)
    tiles, o, dv, bad, nwet = (t.cpu().numpy() for t in cut_masked_dev(region, 16, 16, 12, 12, mode, min_wet, off, div))
    as64 = (lambda a: None if a is None else a.astype(np.float64))
    ref_t, ref_o, ref_d, ref_bad, ref_nwet = lo.cut(region.astype(np.float64), 16, 16, 12, 12, mode, min_wet, as64(off),
                                                    as64(div))
    wet = lo.wet_tiles(region, 16, 16, 12, 12)
    assert (nwet == ref_nwet).all() and (bad == ref_bad).all()
    assert list(np.flatnonzero(bad)) == ([13, 14] if min_wet == 1 else [0, 13, 14])
    # statistics of every plane that has a wet pixel
    if mode == lo.AFFINE:
        assert (o.view(np.int32) == off.view(np.int32)).all() and (dv.view(np.int32) == div.view(np.int32)).all()
    else:
        has = nwet > 0
        for got, ref, what in ((o, ref_o, "off"), (dv, ref_d, "div")):
            err = np.abs(got[has] - ref[has]) / np.maximum(np.abs(ref[has]), 1e-300)
            err[ref[has] == 0] = np.abs(got[has])[ref[has] == 0]
            print(f"{what}: max relative error {float(err.max()) / U:.3f} x 2^-24 (bar 2)")
            assert (err <= 2 * U).all(), what
    worst = 0.0
    for k in range(15):
        if bad[k]:
            assert (tiles[k].view(np.int32) == 0).all(), f"bad tile {k} is not all +0.0"
            continue
        for c in range(2):
            w, got, ref = wet[k, c], tiles[k, c], ref_t[k, c]
            nan = np.isnan(ref[w])
            assert (np.isnan(got[w]) == nan).all()  # a single wet pixel in a tile-local mode: 0 * inf
            err = np.abs(got[w][~nan] - ref[w][~nan]) / np.maximum(1.0, np.abs(ref[w][~nan]))
            worst = max(worst, float(err.max()) if err.size else 0.0)
            assert (err <= 4 * U).all(), (k, c)
            fill32, _, _ = lo.fill(got, w, np.float32)  # from the device's own wet values
            assert same_bits_or_nan(got, fill32), (k, c)
            assert nan.any() or np.isfinite(got).all()
    print(f"wet pixels: max error {worst / U:.3f} x 2^-24 max(1, |v|) (bar 4)")


def test_cut_fill_on_the_float4_path_and_a_large_plane():
    """W, tx, sx multiples of 4 (float4 loads and stores), one channel, a 48 x 48 tile
    (more pixels than threads) with a coast through every tile, and the 96 x 96 plane the
    entry point must serve."""
    rng = np.random.RandomState(33)
    for side, tile, stride in ((112, 48, 32), (96, 96, 96)):
        region = (rng.randn(1, side, side) * 2 + 5).astype(np.float32)
        yy, xx = np.mgrid[0:side, 0:side]
        region[0, (xx + 2 * yy) % 37 < 9] = np.nan
        region[0, 60:90, 50:95] = np.nan
        region[0, 70, 70] = 3.0
        tiles, o, dv, bad, nwet = (t.cpu().numpy() for t in cut_masked_dev(region, tile, tile, stride, stride, lo.LNORM, 1))
        ref_t, ref_o, ref_d, ref_bad, ref_nwet = lo.cut(region.astype(np.float64), tile, tile, stride, stride, lo.LNORM, 1)
        wet = lo.wet_tiles(region, tile, tile, stride, stride)
        assert (nwet == ref_nwet).all() and not bad.any() and not ref_bad.any()
        assert (np.abs(o - ref_o) <= 2 * U * np.abs(ref_o)).all() and (np.abs(dv - ref_d) <= 2 * U * ref_d).all()
        for k in range(tiles.shape[0]):
            w = wet[k, 0]
            assert (np.abs(tiles[k, 0][w] - ref_t[k, 0][w]) <= 4 * U * np.maximum(1.0, np.abs(ref_t[k, 0][w]))).all()
            assert same_bits_or_nan(tiles[k, 0], lo.fill(tiles[k, 0], w, np.float32)[0]), k


# --------------------------------------------------------------------------- 3. blend
# the quad form (scale 4, every edge on a quad boundary) / the scalar form (scale 2, odd Tx)
@pytest.mark.parametrize("hw,T,stride,scale", [((160, 216), (64, 64), (48, 48), 4), ((40, 54), (16, 15), (12, 11), 2)])
@pytest.mark.parametrize("denorm", [True, False])
def test_blend_with_a_finite_mask_is_the_plain_blend(hw, T, stride, scale, denorm):
    d = dev()
    rng = np.random.RandomState(34)
    C = 2
    n = overlap_count(hw[0], T[0], stride[0]) * overlap_count(hw[1], T[1], stride[1])
    tiles = torch.tensor(rng.randn(n, C, *T).astype(np.float32), device=d)
    off = torch.tensor((rng.randn(n, C) * 2 + 1).astype(np.float32), device=d) if denorm else None
    div = torch.tensor((rng.rand(n, C) + 0.5).astype(np.float32), device=d) if denorm else None
    bad = torch.tensor((rng.rand(n) < 0.3).astype(np.int32), device=d)
    mask = torch.tensor(rng.randn(C, hw[0] // scale, hw[1] // scale).astype(np.float32), device=d)
    ref = blend_dev(tiles, off, div, bad, C, *T, *stride, *hw)
    out = blend_masked_dev(tiles, off, div, bad, C, *T, *stride, *hw, mask, scale)
    assert torch.equal(bits(out), bits(ref))


@pytest.mark.parametrize("scale", [4, 2])  # the quad form / the scalar one
def test_blend_puts_the_land_back(scale):
    d = dev()
    rng = np.random.RandomState(35)
    region = lo.coast_region()
    T, S, Ho, Wo = 16 * scale, 12 * scale, 40 * scale, 54 * scale
    tiles = rng.randn(15, 2, T, T).astype(np.float32)
    off = (rng.randn(15, 2) * 2 + 1).astype(np.float32)
    div = (rng.rand(15, 2) + 0.5).astype(np.float32)
    bad = np.zeros(15, np.int32)
    bad[[6, 13, 14]] = 1  # tile (1, 1) too: its own 8 x 8 LR pixels are wet, and NaN for want of a cover
    tiles[bad != 0] = np.nan  # never read
    out = blend_masked_dev(torch.tensor(tiles, device=d), torch.tensor(off, device=d), torch.tensor(div, device=d),
                           torch.tensor(bad, device=d), 2, T, T, S, S, Ho, Wo, torch.tensor(region, device=d), scale)
    out = out.cpu().numpy()
    ref, M = lo.blend(tiles.astype(np.float64), off.astype(np.float64), div.astype(np.float64), bad, S, S, Ho, Wo,
                      region, scale)
    plain, _ = oo.blend(tiles.astype(np.float64), off.astype(np.float64), div.astype(np.float64), bad, S, S, Ho, Wo)
    dry = lo.dry_hr(region, scale)
    assert (np.isnan(ref) == (dry | np.isnan(plain))).all() and (np.isnan(plain) & ~dry).any()
    assert_blend_close(out, ref, M)
    assert (out.view(np.int32)[np.isnan(out)] == 0x7fc00000).all()  # the canonical NaN


# ----------------------------------------------------------------------- 4. end to end
def land_lr(rng, variant=0):
    """[1, 52, 86] LR region for the 4 x 3 plan of tile 16 x 32 at overlap 4 (origins y 0 12
    24 36, x 0 28 54).  variant 0: land rows 38.., columns 56.. with a 3 x 3 lake, which
    leaves tile (3, 2) 101 wet pixels of 512 (bad at min_wet 0.25; the lake is covered by it
    alone), tiles (2, 2) and (3, 1) coastal, and the isolated dry pixel (5, 10) in tile (0, 0)
    alone.  variant 1: another coast -- land rows 0..13, columns 0..20 (tile (0, 0) keeps 218
    wet pixels, its fill takes 14 passes) and a dry column 60."""
    lr = _field(rng, 1, 52, 86) * 2 + 5
    if variant == 0:
        lr[0, 38:52, 56:86] = np.nan
        lr[0, 44:47, 70:73] = 4.0
        lr[0, 5, 10] = np.nan
    else:
        lr[0, 0:14, 0:21] = np.nan
        lr[0, :, 60] = np.nan
    return lr.astype(np.float32)


def test_super_resolve_with_land():
    d = dev()
    spec, model, flat = _small_rcan()
    rng = np.random.RandomState(36)
    lr = land_lr(rng)
    rs = RegionSuperResolver(spec, flat.to(d), lr.shape, tile_lr=TILE, overlap=(4, 4), land=True, device=d)
    assert (rs.ny, rs.nx, rs.sy, rs.sx, rs.min_wet) == (4, 3, 12, 28, 128)
    images = rs.super_resolve(torch.tensor(lr, device=d))
    got = images["model"].cpu().numpy()
    bad = rs.bad.cpu().numpy()
    assert list(np.flatnonzero(bad)) == [11] and images["nwet"].cpu().numpy()[:, 0].tolist()[-1] == 101
    assert torch.isfinite(rs.tiles).all() and (rs.tiles[11] == 0).all()
    # the engine's own outputs, blended and re-masked by the oracle: NaN exactly there, values within the bar
    eng = Engine(spec, rs.n, TILE, train=False, device=d)
    eng.pack(flat.to(d))
    assert torch.equal(bits(eng.forward(flat.to(d), rs.tiles)), bits(rs.sr))
    off, div = np.nan_to_num(f64(rs.off)), np.nan_to_num(f64(rs.div))
    ref, M = lo.blend(f64(rs.sr), off, div, bad, 48, 112, 208, 344, lr, 4)
    assert_blend_close(got, ref, M)
    # every wet HR pixel covered by a non-bad tile is finite; the lake under the bad tile is not
    covered = ~np.isnan(oo.blend(np.ones((12, 1, 64, 128)), None, None, bad, 48, 112, 208, 344)[0])
    wet_hr = ~lo.dry_hr(lr, 4)
    assert np.isfinite(got[wet_hr & covered]).all() and np.isnan(got[~wet_hr]).all()
    assert np.isnan(got[0, 176:188, 280:292]).all() and not covered[0, 176:188, 280:292].any()
    # the tiled baseline: the upsampled tiles through the same blend
    up = upsample(rs.tiles, 4)
    ref_i, M_i = lo.blend(f64(up), off, div, bad, 48, 112, 208, 344, lr, 4)
    assert_blend_close(images["interpolated"].cpu().numpy(), ref_i, M_i)
    # the regression this mode fixes: without it every tile touching land is dropped
    plain = RegionSuperResolver(spec, flat.to(d), lr.shape, tile_lr=TILE, overlap=(4, 4), device=d)
    got_plain = plain.super_resolve(torch.tensor(lr, device=d))["model"].cpu().numpy()
    n_land, n_plain, n_wet = int(np.isfinite(got[wet_hr]).sum()), int(np.isfinite(got_plain[wet_hr]).sum()), int(wet_hr.sum())
    print(f"finite wet HR pixels of {n_wet}: land=True {n_land}, land=False {n_plain}")
    assert list(np.flatnonzero(plain.bad.cpu().numpy())) == [0, 7, 8, 10, 11]
    assert n_plain < n_land == n_wet - 9 * 16


def test_super_resolve_land_mode_without_land_is_the_plain_path():
    d = dev()
    spec, model, flat = _small_rcan()
    rng = np.random.RandomState(37)
    lr = torch.tensor(_field(rng, 1, 52, 86) * 2 + 5, device=d)
    a = RegionSuperResolver(spec, flat.to(d), tuple(lr.shape), tile_lr=TILE, overlap=(4, 4), norm="lscale", land=True,
                            device=d)
    b = RegionSuperResolver(spec, flat.to(d), tuple(lr.shape), tile_lr=TILE, overlap=(4, 4), norm="lscale", device=d)
    ia, ib = a.super_resolve(lr), b.super_resolve(lr)
    assert torch.equal(bits(ia["model"]), bits(ib["model"])) and torch.isfinite(ia["model"]).all()
    assert torch.equal(bits(a.tiles), bits(b.tiles)) and int(a.bad.sum()) == 0 and (a.nwet == 512).all()
    assert "nwet" not in ib and not hasattr(b, "up")


# --------------------------------------------------------------------------- 5. graph
def test_land_graph_replays_another_coast():
    """One captured graph, two coasts whose fills take different numbers of passes (4 and
    14): the trip count lives on the device, nothing of it is baked in at capture."""
    d = dev()
    spec, model, flat = _small_rcan()
    rng = np.random.RandomState(38)
    lrs = [torch.tensor(land_lr(rng, v), device=d) for v in (0, 1)]
    kw = dict(tile_lr=TILE, overlap=(4, 4), land=True, device=d)
    g = RegionSuperResolver(spec, flat.to(d), (1, 52, 86), graph=True, **kw)
    e = RegionSuperResolver(spec, flat.to(d), (1, 52, 86), **kw)
    for lr in (lrs[0], lrs[0], lrs[1], lrs[0]):  # capture + replay, replay, the other coast, and back
        ig, ie = g.super_resolve(lr), e.super_resolve(lr)
        for k in ("model", "interpolated", "nwet"):
            assert torch.equal(bits(ig[k]), bits(ie[k])), k
        assert torch.equal(g.bad, e.bad) and torch.equal(bits(g.tiles), bits(e.tiles))
        assert torch.equal(torch.isnan(ig["model"]).cpu(), torch.tensor(np.isnan(lo.blend(
            np.ones((12, 1, 64, 128)), None, None, e.bad.cpu().numpy(), 48, 112, 208, 344, lr.cpu().numpy(), 4)[0])))
    assert g._graph is not None and e._graph is None
    assert list(np.flatnonzero(e.bad.cpu().numpy())) == [11]


# -------------------------------------------------------------------- 6. masked score
@pytest.mark.parametrize("n", [4 * 5000, 4 * 5000 + 3, 37])
def test_rmse_partial_masked(n):
    """Against fp64 numpy, the count exact, the loss within the 1e-5 that
    test_gpu_kernels holds the device's RMSE of N(0, 1) data to."""
    d = dev()
    spec, model, flat = _small_rcan()
    eng = Engine(spec, 1, TILE, train=False, device=d)
    rng = np.random.RandomState(39)
    p, t = rng.randn(n).astype(np.float32), rng.randn(n).astype(np.float32)
    p[rng.rand(n) < 0.2] = np.nan
    t[rng.rand(n) < 0.3] = np.nan
    t[n // 2] = np.inf
    l4 = torch.full((4,), -7.0, device=d)
    eng.rmse_partial_masked(torch.tensor(p, device=d), torch.tensor(t, device=d), l4)
    Engine.rmse_finalize(l4)
    ref, count = lo.rmse(p, t)
    got = l4.cpu().numpy()
    print(f"n {n}: count {got[1]:.0f} ({count}), loss {got[3]:.8f} numpy {ref:.8f}")
    assert got[1] == count and 0 < count < n and abs(float(got[3]) - ref) < 1e-5
    # nothing in common: the IEEE result
    eng.rmse_partial_masked(torch.full((n,), float("nan"), device=d), torch.tensor(t, device=d), l4)
    Engine.rmse_finalize(l4)
    assert float(l4[1]) == 0 and float(l4[0]) == 0 and np.isnan(float(l4[3]))


def test_score_with_a_coastal_truth():
    d = dev()
    spec, model, flat = _small_rcan()
    rng = np.random.RandomState(40)
    hr = _field(rng, 1, 208, 344) * 2 + 5
    hr[lo.dry_hr(land_lr(rng), 4)] = np.nan  # land on whole LR pixels: the downsample is NaN exactly there
    rs = RegionSuperResolver(spec, flat.to(d), (1, 52, 86), tile_lr=TILE, overlap=(4, 4), land=True, device=d)
    images, losses = rs.score(torch.tensor(hr, device=d))
    assert sorted(losses) == ["count", "interpolated", "model"]
    assert (np.isnan(images["input"].cpu().numpy()) == np.isnan(land_lr(np.random.RandomState(0)))).all()
    for k in ("interpolated", "model"):
        ref, count = lo.rmse(f64(images[k]), hr)
        got = float(losses[k])
        print(f"score {k}: {got:.7f} numpy {ref:.7f} over {count} pixels")
        assert np.isfinite(got) and abs(got - ref) <= 1e-5 * ref
        assert count == int(np.isfinite(hr).sum()) - 9 * 16  # the wet pixels, less the lake under the bad tile
    assert float(losses["count"]) == count


# ------------------------------------------------------------------------ 7. refusals
def test_land_refusals():
    d = dev()
    spec, model, flat = _small_rcan()
    p = flat.to(d)
    for mw in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="min_wet"):
            RegionSuperResolver(spec, p, (1, 40, 54), tile_lr=TILE, land=True, min_wet=mw, device=d)
    with pytest.raises(ValueError, match="floor-grid"):
        RegionSuperResolver(spec, p, (1, 40, 54), tile_lr=TILE, norm="tnorm", land=True, device=d)
    assert RegionSuperResolver(spec, p, (1, 40, 54), tile_lr=TILE, land=True, min_wet=1e-9, device=d).min_wet == 1
    # bad scalars at the ABI: refused with valid buffers in hand, nothing launched
    lib = _lib.load()
    rg = torch.zeros(1, 40, 54, device=d)
    tiles = torch.full((15, 1, 16, 16), 3.0, device=d)
    o, dv = torch.zeros(15, 1, device=d), torch.ones(15, 1, device=d)
    out = torch.full((1, 40, 54), 3.0, device=d)
    nw = torch.full((15, 1), 3, dtype=torch.int32, device=d)
    big = torch.zeros(1, 161, 161, device=d)

    def cut(C=1, H=40, W=54, ty=16, tx=16, sy=12, sx=12, mode=0, min_wet=1, region=rg):
        return lib.srmi_region_to_tiles_overlap_masked(ptr(region), C, H, W, ty, tx, sy, sx, mode, None, None, ptr(tiles),
                                                       ptr(o), ptr(dv), None, min_wet, ptr(nw), st())

    def blend(C=1, Ty=16, Tx=16, Sy=12, Sx=12, Ho=40, Wo=54, scale=2, mask=rg):
        return lib.srmi_tiles_blend_masked(ptr(tiles), ptr(o), ptr(dv), None, C, Ty, Tx, Sy, Sx, Ho, Wo, ptr(mask), scale,
                                           ptr(out), st())

    for kw in (dict(min_wet=0), dict(min_wet=-1), dict(sy=0), dict(sx=17), dict(H=15), dict(C=0), dict(mode=3),
               dict(mode=2)):  # mode 2: AFFINE without off / div
        assert cut(**kw) == _lib.SRMI_ERR_ARG, kw
    assert _lib.ERRORS[cut(H=161, W=161, ty=161, tx=161, sy=161, sx=161, region=big)] == "SRMI_ERR_SHAPE"  # past LDS
    for kw in (dict(scale=0), dict(scale=-2), dict(scale=3), dict(scale=4), dict(Sy=0), dict(Wo=15), dict(C=0),
               dict(mask=None)):  # 40 % 3, 54 % 4
        assert blend(**kw) == _lib.SRMI_ERR_ARG, kw
    torch.cuda.synchronize()
    assert float(tiles.min()) == 3.0 and float(out.min()) == 3.0 and int(nw.min()) == 3  # nothing was written
    assert cut() == 0 and blend() == 0
    torch.cuda.synchronize()
    assert int(nw.min()) == 256
