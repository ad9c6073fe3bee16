"""Overlapped tiles and their blended mosaic on the HIP path: the cut
(srmi_region_to_tiles_overlap) and the blend (srmi_tiles_blend) against the existing
floor-grid kernels (bit for bit where the plans coincide) and against the fp64 oracle
(tests/overlap_oracle.py), and srmi.superres.RegionSuperResolver end to end.

The blend's bar, per pixel: |out - oracle| <= 16 * 2^-24 * M with M the largest
|x * div| + |off| among the covering tiles -- derived, not measured: at most two
roundings per de-normalisation, the products and sums of exactly representable integer
weights, one division, about 13 roundings of 2^-24 relative to M, rounded up."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import overlap_oracle as oo  # noqa: E402
from oracle import rcan_oracle as ro  # noqa: E402
from srmi import _lib  # noqa: E402
from srmi._lib import call, ptr  # noqa: E402
from srmi.engine import Engine, upsample  # noqa: E402
from srmi.superres import RegionSuperResolver, overlap_count  # noqa: E402
from test_gpu_inference import _small_rcan, rel_l2  # noqa: E402

EPS16 = 16.0 * 2.0 ** -24
MODES = [oo.LNORM, oo.LSCALE, oo.AFFINE]


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def st():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.contiguous().view(torch.int32)


def _affine(rng, n, C):
    return (rng.randn(n, C) * 0.5 + 1).astype(np.float32), (rng.rand(n, C) * 2 + 2).astype(np.float32)


def cut_dev(region, ty, tx, sy, sx, mode, off=None, div=None, overlap=True):
    """The overlapped cut (or srmi_region_to_tiles_norm on the floor grid) of a numpy
    region -> device (tiles, off_out, div_out, bad); off_out / div_out are pre-filled
    with the inputs (AFFINE leaves them alone)."""
    d = dev()
    C, H, W = region.shape
    n = overlap_count(H, ty, sy) * overlap_count(W, tx, sx) if overlap else (H // ty) * (W // tx)
    rg = torch.tensor(region, device=d)
    tiles = torch.full((n, C, ty, tx), -7.0, device=d)
    o_in = torch.tensor(off, device=d) if off is not None else None
    d_in = torch.tensor(div, device=d) if div is not None else None
    o_out = o_in.clone() if o_in is not None else torch.full((n, C), -7.0, device=d)
    d_out = d_in.clone() if d_in is not None else torch.full((n, C), -7.0, device=d)
    bad = torch.full((n,), 5, dtype=torch.int32, device=d)
    if overlap:
        call("srmi_region_to_tiles_overlap", ptr(rg), C, H, W, ty, tx, sy, sx, mode, ptr(o_in), ptr(d_in), ptr(tiles),
             ptr(o_out), ptr(d_out), ptr(bad), st())
    else:
        call("srmi_region_to_tiles_norm", ptr(rg), C, H, W, ty, tx, mode, ptr(o_in), ptr(d_in), ptr(tiles), ptr(o_out),
             ptr(d_out), ptr(bad), st())
    return tiles, o_out, d_out, bad


def blend_dev(tiles, off, div, bad, C, Ty, Tx, Sy, Sx, Ho, Wo):
    out = torch.full((C, Ho, Wo), -7.0, device=tiles.device)
    call("srmi_tiles_blend", ptr(tiles), ptr(off), ptr(div), ptr(bad), C, Ty, Tx, Sy, Sx, Ho, Wo, ptr(out), st())
    return out


def f64(t):
    return t.cpu().numpy().astype(np.float64)


def assert_blend_close(out, ref, M):
    """NaN exactly where the oracle is NaN; every other pixel within 16 * 2^-24 * M."""
    out = np.asarray(out, np.float64)
    nan = np.isnan(ref)
    assert (np.isnan(out) == nan).all()
    err, bar = np.abs(out - ref)[~nan], EPS16 * M[~nan]
    print(f"blend: max err / (2^-24 M) = {float((err / (2.0 ** -24 * np.maximum(M[~nan], 1e-300))).max()):.3f}"
          f" over {err.size} pixels (bar 16)")
    assert (err <= bar).all()


# ---------------------------------------------------------------- 1. cut, bit-identity
@pytest.mark.parametrize("tx", [56, 55])  # the register-resident float4 form / the scalar one
@pytest.mark.parametrize("mode", MODES)
def test_cut_at_stride_tile_is_region_to_tiles_norm(tx, mode):
    rng = np.random.RandomState(21)
    region = (rng.randn(2, 3 * 40, 2 * tx) * 3 + 1).astype(np.float32)
    region[1, 45, tx + 3] = np.nan  # tile (1, 1) of the grid is bad
    off, div = _affine(rng, 6, 2) if mode == oo.AFFINE else (None, None)
    got = cut_dev(region, 40, tx, 40, tx, mode, off, div)
    ref = cut_dev(region, 40, tx, 40, tx, mode, off, div, overlap=False)
    for g, r, what in zip(got, ref, ("tiles", "off_out", "div_out", "bad")):
        assert torch.equal(bits(g), bits(r)), what
    assert got[3].cpu().tolist() == [0, 0, 0, 1, 0, 0]


# ------------------------------------------------------- 2. cut, general plan vs oracle
# 40 x 54 / 12: odd origins, a shifted last tile, a triple cover; 41 x 55 / (5, 7): W % 4 != 0
# and misaligned origins; 40 x 56 / 12: the float4 form with a shifted last tile
@pytest.mark.parametrize("hw,stride", [((40, 54), (12, 12)), ((41, 55), (5, 7)), ((40, 56), (12, 12))])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("mode", MODES)
def test_cut_general_plan_matches_oracle(hw, stride, C, mode):
    rng = np.random.RandomState(22)
    region = (rng.randn(C, *hw) * 3 + 1).astype(np.float32)
    n = overlap_count(hw[0], 16, stride[0]) * overlap_count(hw[1], 16, stride[1])
    off, div = _affine(rng, n, C) if mode == oo.AFFINE else (None, None)
    tiles, o, dv, bad = cut_dev(region, 16, 16, *stride, mode, off, div)
    ref_t, ref_o, ref_d, ref_bad = oo.cut(region.astype(np.float64), 16, 16, *stride, mode,
                                          None if off is None else off.astype(np.float64),
                                          None if div is None else div.astype(np.float64))
    assert tiles.shape[0] == ref_t.shape[0] == n and int(bad.sum()) == 0 and not ref_bad.any()
    # the bars of test_region_tiles_kernels (data 3 randn + 1)
    np.testing.assert_allclose(o.cpu().numpy(), ref_o, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(dv.cpu().numpy(), ref_d, rtol=1e-5)
    np.testing.assert_allclose(tiles.cpu().numpy(), ref_t, atol=2e-5)


# -------------------------------------------------------------- 3. blend, bit-identity
@pytest.mark.parametrize("tx", [56, 55])  # the float4 form / the scalar one
@pytest.mark.parametrize("denorm", [True, False])
def test_blend_at_stride_tile_is_tiles_to_region(tx, denorm):
    d = dev()
    rng = np.random.RandomState(23)
    C, ty, gy, gx = 2, 40, 3, 2
    tiles = torch.tensor(rng.randn(gy * gx, C, ty, tx).astype(np.float32), device=d)
    mean = torch.tensor((rng.randn(gy * gx, C) * 2 + 1).astype(np.float32), device=d) if denorm else None
    std = torch.tensor((rng.rand(gy * gx, C) + 0.5).astype(np.float32), device=d) if denorm else None
    ref = torch.full((C, gy * ty, gx * tx), -7.0, device=d)
    call("srmi_tiles_to_region", ptr(tiles), ptr(mean), ptr(std), None, C, ty, tx, gy, gx, ptr(ref), st())
    out = blend_dev(tiles, mean, std, None, C, ty, tx, ty, tx, gy * ty, gx * tx)
    assert torch.equal(bits(out), bits(ref))


# ------------------------------------------------------------- 4. blend vs the oracle
# the plans of the cut test scaled by 4 (every edge on a quad boundary: the float4 form)
# and unscaled (the scalar form)
BLEND_PLANS = [((160, 216), 64, (48, 48)), ((164, 220), 64, (20, 28)), ((40, 54), 16, (12, 12)),
               ((41, 55), 16, (5, 7))]


@pytest.mark.parametrize("hw,T,stride", BLEND_PLANS)
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("with_bad", [False, True])
def test_blend_matches_oracle(hw, T, stride, C, with_bad):
    d = dev()
    rng = np.random.RandomState(24)
    ny, nx = overlap_count(hw[0], T, stride[0]), overlap_count(hw[1], T, stride[1])
    n = ny * nx
    tiles = rng.randn(n, C, T, T).astype(np.float32)
    off = (rng.randn(n, C) * 2 + 1).astype(np.float32)
    div = (rng.rand(n, C) + 0.5).astype(np.float32)
    bad = (rng.rand(n) < 0.3).astype(np.int32) if with_bad else None
    if with_bad:
        tiles[bad != 0] = np.nan  # what a bad tile holds; it must never be read into a sum
    out = blend_dev(torch.tensor(tiles, device=d), torch.tensor(off, device=d), torch.tensor(div, device=d),
                    torch.tensor(bad, device=d) if with_bad else None, C, T, T, *stride, *hw)
    ref, M = oo.blend(tiles.astype(np.float64), off.astype(np.float64), div.astype(np.float64), bad, *stride, *hw)
    assert_blend_close(out.cpu().numpy(), ref, M)
    # no denorm: the stored values
    out = blend_dev(torch.tensor(tiles, device=d), None, None, torch.tensor(bad, device=d) if with_bad else None, C, T,
                    T, *stride, *hw)
    ref, M = oo.blend(tiles.astype(np.float64), None, None, bad, *stride, *hw)
    assert_blend_close(out.cpu().numpy(), ref, M)


# --------------------------------------------------------- 5. round trip on the device
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("patch", [False, True])
def test_cut_then_blend_returns_the_region(C, patch):
    """40 x 54, tile 16, stride 12, lnorm.  With the 8 x 8 NaN patch at rows 16..23,
    columns 28..35 exactly tile (1, 2) is bad and exactly those 64 pixels (3 % of the
    region) are NaN; every other pixel is compared."""
    rng = np.random.RandomState(25)
    region = (rng.randn(C, 40, 54) * 3 + 1).astype(np.float32)
    if patch:
        region[:, 16:24, 28:36] = np.nan
    tiles, off, div, bad = cut_dev(region, 16, 16, 12, 12, oo.LNORM)
    out = blend_dev(tiles, off, div, bad, C, 16, 16, 12, 12, 40, 54).cpu().numpy()
    ref_t, ref_o, ref_d, ref_bad = oo.cut(region.astype(np.float64), 16, 16, 12, 12, oo.LNORM)
    ref, _ = oo.blend(ref_t, ref_o, ref_d, ref_bad, 12, 12, 40, 54)
    assert bad.cpu().tolist() == list(ref_bad) == [int(patch and k == 1 * 5 + 2) for k in range(15)]
    nan = np.isnan(ref)
    assert int(nan.sum()) == (64 * C if patch else 0) and (nan == np.isnan(region)).all()
    # M from the device's own tiles: the scale its roundings are relative to
    keep = np.where(bad.cpu().numpy()[:, None, None, None] != 0, 0.0, f64(tiles))
    _, M = oo.blend(keep, np.nan_to_num(f64(off)), np.nan_to_num(f64(div)), bad.cpu().numpy(), 12, 12, 40, 54)
    assert_blend_close(out, np.where(nan, np.nan, region.astype(np.float64)), M)


# ------------------------------------------------------------------- 6. end to end
def _field(rng, C, h, w):
    base = rng.randn(C, h, w)
    return (base + np.roll(base, 1, 1) + np.roll(base, 1, 2)).astype(np.float32)


TILE = (16, 32)  # the inference engine refuses a 16-wide tile (width % 32 or % 48): the smallest 16-row tile it takes


def test_super_resolve_end_to_end():
    """The small RCAN (1 group, 2 RCABs, C = 1), LR region 40 x 54, LR tile 16 x 32 --
    not 16 x 16: the engine takes widths that are multiples of 32 or 48 -- overlap 4:
    strides (12, 28), a 3 x 2 plan whose last column is shifted to x = 22."""
    d = dev()
    spec, model, flat = _small_rcan()
    rng = np.random.RandomState(26)
    lr = _field(rng, 1, 40, 54)
    rs = RegionSuperResolver(spec, flat.to(d), lr.shape, tile_lr=TILE, overlap=(4, 4), device=d)
    assert (rs.ny, rs.nx, rs.sy, rs.sx) == (3, 2, 12, 28)
    images = rs.super_resolve(torch.tensor(lr, device=d))
    got = images["model"].cpu().numpy()
    assert got.shape == (1, 160, 216) and np.isfinite(got).all()
    assert torch.equal(images["input"], torch.tensor(lr, device=d))
    # (e) the baseline is srmi_upsample of the whole region
    assert torch.equal(bits(images["interpolated"]), bits(upsample(torch.tensor(lr, device=d)[None], 4)[0]))
    # (a) the blend of the engine's own per-tile outputs (the forward is batch-invariant)
    eng = Engine(spec, rs.n, TILE, train=False, device=d)
    eng.pack(flat.to(d))
    sr = eng.forward(flat.to(d), rs.tiles)
    assert torch.equal(bits(sr), bits(rs.sr))
    ref, M = oo.blend(f64(sr), f64(rs.off), f64(rs.div), rs.bad.cpu().numpy(), 48, 112, 160, 216)
    assert_blend_close(got, ref, M)
    # (b) the fp64 torch oracle per tile, blended by the oracle: the bf16 mosaic bar
    t64, o64, d64, b64 = oo.cut(lr.astype(np.float64), *TILE, 12, 28, oo.LNORM)
    with torch.no_grad():
        sr64 = model(torch.tensor(t64)).numpy()
    ref64, _ = oo.blend(sr64, o64, d64, b64, 48, 112, 160, 216)
    assert rel_l2(got, ref64) < 2e-2
    # (d) micro-batch engines, chunks and the captured graph change no bit
    for kw in (dict(micro=2), dict(micro=1, max_batch=4), dict(micro=2, max_batch=2), dict(graph=True)):
        rs2 = RegionSuperResolver(spec, flat.to(d), lr.shape, tile_lr=TILE, overlap=(4, 4), device=d, **kw)
        for _ in range(2):  # graph: the capture's warm-up, then a replay
            im2 = rs2.super_resolve(torch.tensor(lr, device=d))
            assert torch.equal(bits(im2["model"]), bits(images["model"])), kw
            assert torch.equal(bits(im2["interpolated"]), bits(images["interpolated"])), kw


def test_super_resolve_overlap_zero_is_the_plain_mosaic():
    """(c) overlap 0 on a region the tile divides (32 x 64 LR, tile 16 x 32): the manual
    composition of srmi_region_to_tiles, Engine.forward and srmi_tiles_to_region."""
    d = dev()
    spec, model, flat = _small_rcan()
    rng = np.random.RandomState(27)
    lr = torch.tensor(_field(rng, 1, 32, 64), device=d)
    rs = RegionSuperResolver(spec, flat.to(d), tuple(lr.shape), tile_lr=TILE, overlap=(0, 0), device=d)
    got = rs.super_resolve(lr)["model"]
    n = 4
    tiles = torch.empty(n, 1, *TILE, device=d)
    mean, std = torch.empty(n, 1, device=d), torch.empty(n, 1, device=d)
    call("srmi_region_to_tiles", ptr(lr), 1, 32, 64, *TILE, ptr(tiles), ptr(mean), ptr(std), None, st())
    eng = Engine(spec, n, TILE, train=False, device=d)
    eng.pack(flat.to(d))
    sr = eng.forward(flat.to(d), tiles)
    ref = torch.empty(1, 128, 256, device=d)
    call("srmi_tiles_to_region", ptr(sr), ptr(mean), ptr(std), None, 1, 64, 128, 2, 2, ptr(ref), st())
    assert torch.equal(bits(got), bits(ref))


def test_score_is_the_rmse_of_the_returned_images():
    d = dev()
    spec, model, flat = _small_rcan()
    rng = np.random.RandomState(28)
    hr = _field(rng, 1, 160, 216)
    rs = RegionSuperResolver(spec, flat.to(d), (1, 40, 54), tile_lr=TILE, overlap=(4, 4), device=d)
    images, losses = rs.score(torch.tensor(hr, device=d))
    for k, tol in (("interpolated", 1e-5), ("model", 2e-3)):
        ref = float(np.sqrt(np.mean((f64(images[k]) - hr.astype(np.float64)) ** 2)))
        got = float(losses[k])
        print(f"score {k}: {got:.7f} numpy {ref:.7f}")
        assert np.isfinite(got) and abs(got - ref) <= tol * ref


@pytest.mark.parametrize("norm", ["lscale", "gnorm", "gscale"])
def test_super_resolve_other_norms(norm):
    """lscale from the LR tile, gnorm / gscale from the dataset's global constants (one
    AFFINE row per tile): the tiles the engine sees are the oracle's, and the output is
    de-normalised -- the blend of the engine's outputs with those offsets and divisors."""
    from srmi.norm import NormStats
    d = dev()
    spec, model, flat = _small_rcan()
    rng = np.random.RandomState(29)
    lr = _field(rng, 1, 40, 54) * 2 + 5
    stats = NormStats()
    stats.tiles = torch.tensor([[[5.0, 9.0, 14.0, -3.0]]], device=d)  # mean, var, max, min
    stats.globals = stats.tiles[0].clone()
    rs = RegionSuperResolver(spec, flat.to(d), lr.shape, tile_lr=TILE, overlap=(4, 4), norm=norm, stats=stats, device=d)
    got = rs.super_resolve(torch.tensor(lr, device=d))["model"].cpu().numpy()
    mode = oo.LSCALE if norm == "lscale" else oo.AFFINE
    off, div = {"lscale": (None, None), "gnorm": (5.0, 3.0), "gscale": (-3.0, 17.0)}[norm]
    aff = (None, None) if off is None else (np.full((rs.n, 1), off), np.full((rs.n, 1), div))
    ref_t, ref_o, ref_d, _ = oo.cut(lr.astype(np.float64), *TILE, 12, 28, mode, *aff)
    np.testing.assert_allclose(rs.tiles.cpu().numpy(), ref_t, atol=2e-5)
    np.testing.assert_allclose(rs.off.cpu().numpy(), ref_o, rtol=1e-6)
    np.testing.assert_allclose(rs.div.cpu().numpy(), ref_d, rtol=1e-5)
    ref, M = oo.blend(f64(rs.sr), f64(rs.off), f64(rs.div), rs.bad.cpu().numpy(), 48, 112, 160, 216)
    assert_blend_close(got, ref, M)


# --------------------------------------------------------------------- 7. refusals
def test_refusals():
    d = dev()
    spec, model, flat = _small_rcan()
    p = flat.to(d)
    with pytest.raises(ValueError, match="floor-grid"):
        RegionSuperResolver(spec, p, (1, 40, 54), tile_lr=TILE, norm="tnorm", device=d)
    with pytest.raises(ValueError, match="floor-grid"):
        RegionSuperResolver(spec, p, (1, 40, 54), tile_lr=TILE, task={"norm": "tscale"}, device=d)
    with pytest.raises(ValueError, match="overlap"):
        RegionSuperResolver(spec, p, (1, 40, 54), tile_lr=TILE, overlap=(9, 4), device=d)
    with pytest.raises(ValueError, match="smaller"):
        RegionSuperResolver(spec, p, (1, 40, 31), tile_lr=TILE, device=d)
    with pytest.raises(ValueError, match="statistics"):
        RegionSuperResolver(spec, p, (1, 40, 54), tile_lr=TILE, norm="gnorm", device=d)
    # bad scalars at the ABI: refused with valid buffers in hand, nothing launched
    lib = _lib.load()
    rg = torch.zeros(1, 40, 54, device=d)
    tiles = torch.full((15, 1, 16, 16), 3.0, device=d)
    o, dv = torch.zeros(15, 1, device=d), torch.ones(15, 1, device=d)
    out = torch.full((1, 40, 54), 3.0, device=d)

    def cut(C=1, H=40, W=54, ty=16, tx=16, sy=12, sx=12, mode=0):
        return lib.srmi_region_to_tiles_overlap(ptr(rg), C, H, W, ty, tx, sy, sx, mode, None, None, ptr(tiles), ptr(o),
                                                ptr(dv), None, st())

    def blend(C=1, Ty=16, Tx=16, Sy=12, Sx=12, Ho=40, Wo=54):
        return lib.srmi_tiles_blend(ptr(tiles), ptr(o), ptr(dv), None, C, Ty, Tx, Sy, Sx, Ho, Wo, ptr(out), st())

    for kw in (dict(sy=0), dict(sx=17), dict(H=15), dict(W=15), dict(ty=0), dict(C=0), dict(mode=3), dict(mode=-1),
               dict(sx=-4), dict(mode=2)):  # mode 2: AFFINE without off / div
        assert cut(**kw) == _lib.SRMI_ERR_ARG, kw
    for kw in (dict(Sy=0), dict(Sx=17), dict(Ho=15), dict(Wo=15), dict(Tx=0), dict(C=0), dict(Sy=-1)):
        assert blend(**kw) == _lib.SRMI_ERR_ARG, kw
    torch.cuda.synchronize()
    assert float(tiles.min()) == 3.0 and float(out.min()) == 3.0  # nothing was written
    assert cut() == 0 and blend() == 0
    torch.cuda.synchronize()
