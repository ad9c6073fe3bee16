"""Training on tiles with land on the HIP path: the keep flags with a threshold
(srmi_tiles_dry), the fill in place (srmi_tiles_fill), the masked batch preparation
(srmi_batch_prep_masked), the masked loss and its gradient (srmi_tile_loss_parts_masked,
srmi_loss_from_parts_masked, srmi_loss_dy_masked), FusedTrainer(land=True), the land feed
and data parallelism -- against the unmasked kernels (bit for bit where no land is
involved) and the fp64 oracle (tests/land_train_oracle.py).

Bars, derived, not measured (U = 2^-24).  Statistics: one rounding of an fp64 result plus
an ulp for the reduction order, 2 U relative; wet pixels: the fp64 (x - off) * (1 / div)
rounded once next to the oracle's division, 4 U max(1, |v|) -- both as tests/test_gpu_land.py.
The LR tile: the compiler contracts and pairs the 20 multiply-adds of downsample_kernel's
arithmetic as it sees fit, so its fp32 order cannot be restated exactly; its wet pixels are
held to 4 U max(1, |v|) of the fp64 resampling of the device's own hr, and its filled
pixels, bit for bit, to land_oracle.fill run from the device's wet LR values.  The masked
loss against fp64: 1e-5 relative, the bar tests/test_gpu_model.py
(test_small_model_step_vs_golden, the interp loss) and tests/test_gpu_fp32.py put on a loss
that went through srmi_tile_loss_parts / srmi_loss_from_parts on exact inputs -- no test
compares those two kernels with an oracle directly.  Charbonnier dy: sqrt, divide and the
product, one rounding each and one for eps: 4 U relative."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import land_oracle as lo  # noqa: E402
import land_train_oracle as lt  # noqa: E402
import test_gpu_model  # noqa: E402
from oracle import rcan_oracle as ro  # noqa: E402
from srmi import _lib  # noqa: E402
from srmi._lib import SRMI_LOSS_MEAN, SRMI_LOSS_RMSE, TILE_LOSS_SUB, call, ptr, stream_handle  # noqa: E402
from srmi.engine import NetSpec, param_table  # noqa: E402
from srmi.trainer import CHARBONNIER_EPS, FusedTrainer, default_init_  # noqa: E402
from test_gpu_model import flat_from_model, rel_l2  # noqa: E402

U = 2.0 ** -24
KINDS = {"l2": SRMI_LOSS_RMSE, "charbonnier": SRMI_LOSS_MEAN}
ERR_SHAPE = -10002


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def st():
    return stream_handle()


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool((a.view(np.int32) == b.view(np.int32)).all())


def rcan_spec(nl, nb, scale=4, dtype="bf16"):
    return NetSpec(arch="rcan", nchannels_in=2, nchannels_out=2, nfeatures=64, nlayers=nl, nblocks=nb, cbottleneck=2,
                   scale=scale, dtype=dtype)


def init_flat(spec, seed):
    table = param_table(spec)
    flat = torch.empty(sum(t[2] for t in table), device=dev())
    default_init_(flat, table, seed=seed)
    return flat


# ------------------------------------------------------------------ 1. srmi_tiles_dry
@pytest.mark.parametrize("min_wet", [1, 64, 256])
def test_tiles_dry_matches_numpy(min_wet):
    region = lo.coast_region()
    C, H, W = region.shape
    ncells = (H // 16) * (W // 16)
    rg = torch.tensor(region, device=dev())
    bad = torch.full((C * ncells,), 5, dtype=torch.int32, device=dev())
    nwet = torch.full((C * ncells,), -1, dtype=torch.int32, device=dev())
    call("srmi_tiles_dry", ptr(rg), C, H, W, 16, 16, min_wet, ptr(bad), ptr(nwet), st())
    ref_bad, ref_nwet = lt.keep_flags(region, 16, 16, min_wet)
    assert (nwet.cpu().numpy() == ref_nwet.ravel()).all()
    assert (bad.cpu().numpy() == ref_bad.ravel()).all()
    # nwet is optional
    bad2 = torch.full_like(bad, 5)
    call("srmi_tiles_dry", ptr(rg), C, H, W, 16, 16, min_wet, ptr(bad2), None, st())
    assert torch.equal(bad, bad2)
    if min_wet == 256:  # the whole plane, channels that share a mask: srmi_tiles_nonfinite
        both = torch.stack([rg[0], rg[0]]).contiguous()
        both[:, 16:32, 32:48] = 1.0  # every tile of the floor grid touches land: one that does not
        got = torch.full_like(bad, 5)
        want = torch.full_like(bad, 5)
        call("srmi_tiles_dry", ptr(both), C, H, W, 16, 16, 256, ptr(got), None, st())
        call("srmi_tiles_nonfinite", ptr(both), C, H, W, 16, 16, ptr(want), st())
        assert torch.equal(got, want) and 0 < int(want.sum()) < want.numel()
    with pytest.raises(_lib.SrmiError, match="SRMI_ERR_ARG"):
        call("srmi_tiles_dry", ptr(rg), C, H, W, 16, 16, 0, ptr(bad), None, st())


# ----------------------------------------------------------------- 2. srmi_tiles_fill
def fill_dev(planes):
    """planes [n, h, w] numpy -> (filled numpy, passes numpy), passes pre-filled with junk."""
    t = torch.tensor(planes, device=dev())
    passes = torch.full((t.shape[0],), 77, dtype=torch.int32, device=dev())
    call("srmi_tiles_fill", ptr(t), t.shape[0], t.shape[1], t.shape[2], ptr(passes), st())
    return t.cpu().numpy(), passes.cpu().numpy()


def test_tiles_fill_is_the_bit_model():
    by_shape = {}
    for plane, wet in lo.coast_planes():
        by_shape.setdefault(plane.shape, []).append((np.where(wet, plane, np.nan).astype(np.float32), wet))
    assert set(by_shape) == {(16, 16), (48, 48), (32, 40), (17, 23)}
    rng = np.random.RandomState(3)
    for shape, items in by_shape.items():
        finite = rng.randn(*shape).astype(np.float32)
        finite[0, 0] = -0.0  # kept as it is: an all-finite plane is not rewritten
        stack = np.stack([p for p, _ in items] + [finite, np.full(shape, np.nan, np.float32)])
        got, passes = fill_dev(stack)
        for k, (p, wet) in enumerate(items):
            ref, _, j = lo.fill(p, wet, np.float32)
            assert same_bits(got[k], ref) and passes[k] == j, (shape, k, passes[k], j)
        assert same_bits(got[-2], finite) and passes[-2] == 0
        assert (got[-1].view(np.int32) == 0).all() and passes[-1] == -1
    assert max(lo.fill(p, w, np.float32)[2] for p, w in lo.coast_planes()) >= 15


def test_tiles_fill_plane_limit_and_plane_stride():
    rng = np.random.RandomState(4)
    big = rng.randn(1, 160, 160).astype(np.float32)  # 25600 pixels: the largest plane
    yy, xx = np.mgrid[0:160, 0:160]
    big[0, xx > 100 + 20 * np.sin(yy / 9.0)] = np.nan
    got, passes = fill_dev(big)
    ref, _, j = lo.fill(big[0], np.isfinite(big[0]), np.float32)
    assert same_bits(got[0], ref) and passes[0] == j
    lib = _lib.load()
    t = torch.zeros(161 * 160, device=dev())
    assert lib.srmi_tiles_fill(ptr(t), 1, 161, 160, None, st()) == ERR_SHAPE
    # 70 000 planes of 4 x 4: more than the grid holds, plane p carries pattern p % 97
    pats = rng.randn(97, 4, 4).astype(np.float32)
    pats[rng.rand(97, 4, 4) < 0.35] = np.nan
    pats[5], pats[6] = np.nan, rng.randn(4, 4)
    refs, rpass = [], []
    for p in pats:
        wet = np.isfinite(p)
        if not wet.any():
            refs.append(np.zeros((4, 4), np.float32)), rpass.append(-1)
        elif wet.all():
            refs.append(p), rpass.append(0)
        else:
            r, _, j = lo.fill(p, wet, np.float32)
            refs.append(r), rpass.append(j)
    idx = np.arange(70000) % 97
    got, passes = fill_dev(pats[idx])
    assert same_bits(got, np.stack(refs)[idx]) and (passes == np.array(rpass)[idx]).all()


# ---------------------------------------------------------- 3. srmi_batch_prep_masked
def prep_masked_dev(raw, mode, flip, scale, off=None, div=None, with_lr=True):
    d = dev()
    B, C, T, _ = raw.shape
    r = torch.tensor(raw, device=d)
    hr = torch.full((B, C, T, T), -7.0, device=d)
    lr = torch.full((B, C, T // scale, T // scale), -7.0, device=d) if with_lr else None
    o_in = torch.tensor(off, device=d) if off is not None else None
    d_in = torch.tensor(div, device=d) if div is not None else None
    o = torch.full((B, C), -7.0, device=d)
    dv = torch.full((B, C), -7.0, device=d)
    nwet = torch.full((B, C), -1, dtype=torch.int32, device=d)
    call("srmi_batch_prep_masked", ptr(r), B, C, T, flip, scale, mode, ptr(o_in), ptr(d_in), ptr(hr), ptr(lr), ptr(o),
         ptr(dv), ptr(nwet), st())
    return hr, lr, o, dv, nwet


def _affine(rng, B, C):
    return (rng.randn(B, C) + 5).astype(np.float32), (1 + rng.rand(B, C)).astype(np.float32)


def check_prep(raw, mode, flip, scale, off=None, div=None):
    hr, lr, o, dv, nwet = (t.cpu().numpy() for t in prep_masked_dev(raw, mode, flip, scale, off, div))
    as64 = (lambda a: None if a is None else a.astype(np.float64))
    ref_hr, ref_o, ref_d, ref_nwet = lt.prep(raw.astype(np.float64), mode, flip, as64(off), as64(div))
    # the conditions of the comparison
    lt.check_conditions(ref_hr, scale)
    assert (nwet == ref_nwet).all()
    if mode == lt.AFFINE:
        assert (o == -7.0).all() and (dv == -7.0).all()  # not written
    else:
        for got, ref, what in ((o, ref_o, "off"), (dv, ref_d, "div")):
            err = np.abs(got - ref) / np.abs(ref)
            print(f"{what}: max relative error {float(err.max()) / U:.3f} U (bar 2)")
            assert (err <= 2 * U).all(), what
    dry = np.isnan(ref_hr)
    assert (np.isnan(hr) == dry).all() and np.isfinite(hr[~dry]).all()
    assert (hr.view(np.int32)[dry] == 0x7fc00000).all()  # the canonical NaN
    err = np.abs(hr[~dry] - ref_hr[~dry]) / np.maximum(1.0, np.abs(ref_hr[~dry]))
    print(f"hr wet pixels: max error {float(err.max()) / U:.3f} U max(1, |v|) (bar 4)")
    assert (err <= 4 * U).all()
    # lr from the device's own hr: the wet pixels against the fp64 resampling, the filled
    # ones against the bit model of the fill run from the device's wet LR values
    lr64 = ro.downsample_explicit(hr.astype(np.float64), scale)
    ldry = lt.lr_dry(dry, scale)
    assert (np.isnan(lr64) == ldry).all() and np.isfinite(lr).all()
    err = np.abs(lr[~ldry] - lr64[~ldry]) / np.maximum(1.0, np.abs(lr64[~ldry]))
    print(f"lr wet pixels: max error {float(err.max()) / U:.3f} U max(1, |v|) (bar 4)")
    assert (err <= 4 * U).all()
    for b in range(lr.shape[0]):
        for c in range(lr.shape[1]):
            assert same_bits(lr[b, c], lo.fill(lr[b, c], ~ldry[b, c], np.float32)[0]), (b, c)


@pytest.mark.parametrize("mode,flip", [(lt.LSCALE, f) for f in range(8)] + [(lt.LNORM, 0), (lt.LNORM, 5),
                                                                            (lt.AFFINE, 0), (lt.AFFINE, 5)])
def test_batch_prep_masked_vs_oracle(mode, flip):
    raw = lt.land_batch(3, 2, 32, 11) * np.float32(3) + np.float32(5)
    off, div = _affine(np.random.RandomState(12), 3, 2) if mode == lt.AFFINE else (None, None)
    check_prep(raw, mode, flip, 4, off, div)


@pytest.mark.parametrize("T", [192, 196])
def test_batch_prep_masked_real_size_and_the_unstaged_form(T):
    """192: the real tile, the plane in LDS; 196: the first even size past the 150 KiB the
    staged plane may take (194 x 195 floats still fit), read through L2 instead."""
    raw = lt.land_batch(2, 1, T, 13) * np.float32(2) + np.float32(290)
    check_prep(raw, lt.LNORM, 5, 4)


@pytest.mark.parametrize("T", [32, 196])
@pytest.mark.parametrize("mode", [lt.LSCALE, lt.AFFINE])
def test_batch_prep_masked_without_land_is_batch_prep_norm(mode, T):
    rng = np.random.RandomState(14)
    raw = (rng.randn(3, 2, T, T) * 3 + 1).astype(np.float32)
    off, div = _affine(rng, 3, 2) if mode == lt.AFFINE else (None, None)
    d = dev()
    for flip in (0, 6):
        got = prep_masked_dev(raw, mode, flip, 4, off, div)
        r = torch.tensor(raw, device=d)
        hr, lr = torch.full_like(got[0], -7.0), torch.full_like(got[1], -7.0)
        o, dv = torch.full((3, 2), -7.0, device=d), torch.full((3, 2), -7.0, device=d)
        o_in = torch.tensor(off, device=d) if off is not None else None
        d_in = torch.tensor(div, device=d) if div is not None else None
        call("srmi_batch_prep_norm", ptr(r), 3, 2, T, flip, 4, mode, ptr(o_in), ptr(d_in), ptr(hr), ptr(lr), ptr(o),
             ptr(dv), st())
        for g, w, what in zip(got[:4], (hr, lr, o, dv), ("hr", "lr", "off_out", "div_out")):
            assert torch.equal(bits(g), bits(w)), (what, flip)
        assert (got[4] == T * T).all()


def test_batch_prep_masked_plane_without_a_wet_pixel_and_errors():
    raw = lt.land_batch(2, 2, 32, 15)
    raw[1, 1] = np.nan
    hr, lr, o, dv, nwet = (t.cpu().numpy() for t in prep_masked_dev(raw, lt.LNORM, 0, 4))
    assert np.isnan(hr[1, 1]).all() and (lr[1, 1].view(np.int32) == 0).all() and nwet[1, 1] == 0
    assert np.isnan(o[1, 1]) and np.isfinite(hr[1, 0]).any() and np.isfinite(lr).all()
    lib = _lib.load()
    r, h = torch.zeros(2 * 8 * 8 + 4, device=dev()), torch.zeros(2 * 8 * 8 + 4, device=dev())
    E = _lib.SRMI_ERR_ARG
    f = lib.srmi_batch_prep_masked
    assert f(ptr(r), 1, 1, 7, 0, 2, 0, None, None, ptr(h), None, None, None, None, st()) == ERR_SHAPE  # T odd
    assert f(ptr(r), 1, 1, 8, 8, 2, 0, None, None, ptr(h), None, None, None, None, st()) == ERR_SHAPE  # flip
    assert f(ptr(r), 1, 1, 8, 0, 3, 0, None, None, ptr(h), ptr(h), None, None, None, st()) == ERR_SHAPE  # T % scale
    assert f(ptr(r), 1, 1, 8, 0, 2, 3, None, None, ptr(h), None, None, None, None, st()) == E  # mode
    assert f(ptr(r), 1, 1, 8, 0, 2, 2, None, None, ptr(h), None, None, None, None, st()) == E  # AFFINE without off
    assert f(ptr(r) + 4, 1, 1, 8, 0, 2, 1, None, None, ptr(h), None, None, None, None, st()) == E  # alignment
    assert f(ptr(r), 1, 1, 8, 0, 2, 1, None, None, None, None, None, None, None, st()) == E


def test_prep_batch_land_python():
    from srmi.batch import prep_batch
    raw = torch.tensor(lt.land_batch(3, 2, 32, 16) * np.float32(3) + np.float32(5), device=dev())
    out = prep_batch(raw, 5, 4, land=True)
    want = prep_masked_dev(raw.cpu().numpy(), lt.LNORM, 5, 4)
    assert torch.equal(bits(out["hr"]), bits(want[0])) and torch.equal(bits(out["lr"]), bits(want[1]))
    assert torch.equal(out["nwet"], want[4]) and torch.equal(bits(out["mean"].view(3, 2)), bits(want[2]))
    ls = prep_batch(raw, 0, 4, norm="lscale", land=True, with_lr=False)
    wet = raw.cpu().numpy()
    assert "lr" not in ls and np.array_equal(ls["max"].cpu().numpy()[..., 0, 0], np.nanmax(wet, axis=(2, 3)))
    assert np.array_equal(ls["min"].cpu().numpy()[..., 0, 0], np.nanmin(wet, axis=(2, 3)))
    with pytest.raises(ValueError, match="land=True"):
        prep_batch(raw, norm="tscale", land=True)


@pytest.mark.parametrize("norm", ["gnorm", "gscale"])
def test_prep_batch_land_dataset_constants(norm):
    """gnorm / gscale with land: the constants come from the statistics of all-wet tiles
    (what a land=False feed over the same files gives) and go through the AFFINE mode."""
    from srmi.batch import prep_batch
    from srmi.norm import NormStats
    d = dev()
    stats = NormStats.compute([torch.tensor(ro.synthetic_hr(5, 2, 32, 26) * np.float32(3) + np.float32(5), device=d)])
    raw_np = lt.land_batch(3, 2, 32, 16) * np.float32(3) + np.float32(5)
    raw = torch.tensor(raw_np, device=d)
    off, div = (v.cpu().numpy() for v in stats.offsets(norm, (0, 3)))
    assert off.shape == (3, 2) and (div > 0).all()
    out = prep_batch(raw, 5, 4, norm=norm, stats=stats, land=True)
    want = prep_masked_dev(raw_np, lt.AFFINE, 5, 4, off, div)
    assert torch.equal(bits(out["hr"]), bits(want[0])) and torch.equal(bits(out["lr"]), bits(want[1]))
    assert torch.equal(out["nwet"], want[4]) and set(out) == {"hr", "lr", "nwet", "xyflip"}
    check_prep(raw_np, lt.AFFINE, 5, 4, off, div)
    with pytest.raises(ValueError, match="needs the dataset statistics"):
        prep_batch(raw, norm=norm, land=True)
    with pytest.raises(ValueError, match="statistics rows"):  # statistics of another channel count
        prep_batch(raw[:, :1].contiguous(), norm=norm, stats=stats, land=True)


# -------------------------------------------------------------------- 4. loss kernels
def loss_dev(p, t, kind, masked, count=None):
    """-> (parts, cparts or None, loss4 finalised, loss4 not finalised)."""
    d = dev()
    nt, te = p.shape[0], p[0].numel()
    parts = torch.full((nt * TILE_LOSS_SUB,), -7.0, device=d)
    cparts = torch.full((nt * TILE_LOSS_SUB,), -7.0, device=d) if masked else None
    l4, l4n = torch.full((4,), -7.0, device=d), torch.full((4,), -7.0, device=d)
    if masked:
        call("srmi_tile_loss_parts_masked", ptr(p), ptr(t), nt, te, kind, CHARBONNIER_EPS, ptr(parts), ptr(cparts), st())
        call("srmi_loss_from_parts_masked", ptr(parts), ptr(cparts), nt, kind, ptr(l4), st())
        call("srmi_loss_from_parts_masked", ptr(parts), ptr(cparts), nt, -1, ptr(l4n), st())
    else:
        call("srmi_tile_loss_parts", ptr(p), ptr(t), nt, te, kind, CHARBONNIER_EPS, ptr(parts), st())
        call("srmi_loss_from_parts", ptr(parts), nt, float(count), kind, ptr(l4), st())
        call("srmi_loss_from_parts", ptr(parts), nt, float(count), -1, ptr(l4n), st())
    return parts, cparts, l4, l4n


@pytest.mark.parametrize("loss_fn", ["l2", "charbonnier"])
def test_masked_loss_kernels(loss_fn):
    kind = KINDS[loss_fn]
    rng = np.random.RandomState(17)
    d = dev()
    pn = rng.randn(3, 2, 32, 32).astype(np.float32)
    p = torch.tensor(pn, device=d)
    # all finite: the unmasked kernels, bit for bit
    tf = torch.tensor(ro.synthetic_hr(3, 2, 32, 18), device=d)
    parts, cparts, l4, l4n = loss_dev(p, tf, kind, True)
    rparts, _, r4, r4n = loss_dev(p, tf, kind, False, count=p.numel())
    assert torch.equal(bits(parts), bits(rparts)) and torch.equal(bits(l4), bits(r4))
    assert torch.equal(bits(l4n[:2]), bits(r4n[:2])) and (l4n[2:] == -7.0).all()  # kind -1: not finalised
    assert float(cparts.double().sum()) == p.numel() and (cparts == 2 * 32 * 32 // TILE_LOSS_SUB).all()
    # with land
    tn = lt.land_batch(3, 2, 32, 18)
    pn2 = pn.copy()
    pn2[0, 0, 3, 4] = np.inf  # a non-finite prediction is masked too
    p2, t = torch.tensor(pn2, device=d), torch.tensor(tn, device=d)
    parts, cparts, l4, _ = loss_dev(p2, t, kind, True)
    ref, count = lt.masked_loss(torch.tensor(pn2, dtype=torch.float64), torch.tensor(tn, dtype=torch.float64), loss_fn)
    l4 = l4.cpu().numpy()
    assert l4[1] == count == int((np.isfinite(pn2) & np.isfinite(tn)).sum())
    rel = abs(float(l4[3]) - float(ref)) / float(ref)
    print(f"{loss_fn}: masked loss {l4[3]:.8f} oracle {float(ref):.8f} rel {rel:.2e} (bar 1e-5)")
    assert rel < 1e-5
    # dy
    l4d = torch.tensor(l4, device=d)
    dy = torch.full_like(p2, -7.0)
    call("srmi_loss_dy_masked", ptr(p2), ptr(t), p2.numel(), kind, CHARBONNIER_EPS, ptr(l4d), ptr(dy), st())
    dy = dy.cpu().numpy()
    both = np.isfinite(pn2) & np.isfinite(tn)
    assert (dy.view(np.int32)[~both] == 0).all()  # +0.0 on land
    with np.errstate(invalid="ignore"):
        dd = (pn2 - tn).astype(np.float32)
    if loss_fn == "l2":
        assert same_bits(dy[both], (dd * np.float32(l4[2]))[both])
        assert l4[2] == np.float32(1) / (np.float32(l4[1]) * np.float32(l4[3]))
    else:
        d64 = dd[both].astype(np.float64)
        want = d64 / np.sqrt(d64 ** 2 + CHARBONNIER_EPS) / count
        err = np.abs(dy[both] - want) / np.abs(want)
        print(f"charbonnier dy: max relative error {float(err.max()) / U:.3f} U (bar 4)")
        assert (err <= 4 * U).all()
    np.testing.assert_allclose(dy, lt.masked_dy(pn2, tn, loss_fn), rtol=1e-5, atol=1e-12)
    # nothing finite in common: the IEEE result
    nan = torch.full_like(p, float("nan"))
    _, cparts, l4, _ = loss_dev(p, nan, kind, True)
    assert float(cparts.sum()) == 0 and float(l4[1]) == 0 and np.isnan(float(l4[3]))


# ------------------------------------------------------------- 5. trainer, no land
@pytest.mark.parametrize("loss_fn", ["l2", "charbonnier"])
@pytest.mark.parametrize("B,micro", [(2, 1), (4, 2)])
def test_land_trainer_on_an_all_wet_batch_is_the_plain_trainer(B, micro, loss_fn):
    """The fill finds nothing to fill, the masked parts are the plain parts, the count is
    the element count, and the tail kernels use dy = (sr - hr) * loss4[2] as it is instead
    of forming it: every bit of two steps is the plain trainer's."""
    spec = rcan_spec(1, 2)
    flat = init_flat(spec, 5)
    hr = torch.tensor(ro.synthetic_hr(B, 2, 192, 19), device=dev())
    res = []
    for land in (False, True):
        tr = FusedTrainer(spec, B, (48, 48), device=dev(), params=flat, micro=micro, loss_fn=loss_fn, land=land)
        assert tr.micro == micro
        rows = []
        for _ in range(2):
            out = tr.step(hr)
            torch.cuda.synchronize()
            rows.append((out["loss"].clone(), out["interp_loss"].clone(), tr.sr.clone(), tr.grads.clone(),
                         tr.params.clone()))
        res.append(rows)
        del tr
    for k, (a, b) in enumerate(zip(*res)):
        for x, y, what in zip(a, b, ("loss", "interp_loss", "sr", "grads", "params")):
            assert torch.equal(bits(x), bits(y)), (k, what, float((x - y).abs().max()))
    assert np.isfinite(float(res[0][1][0]))


# -------------------------------------------------- 6. trainer with a coast, vs fp64
def masked_drift_bounds(monkeypatch, model, hr, scale, loss_fn, g_ref):
    """test_gpu_model.drift_bounds itself -- the engine may sit at most 3 x the drift of the
    same fp64 step with bf16-rounded conv operands (tests/gpu_oracle.py), + 1e-3, from the
    exact gradient -- with the oracle step it runs the emulation through replaced by the
    masked one (same signature, same return)."""
    monkeypatch.setattr(test_gpu_model, "oracle_grads", lambda m, h, s: lt.train_step(m, h, s, loss_fn))
    return test_gpu_model.drift_bounds(model, hr, scale, g_ref)


@pytest.fixture(scope="module")
def coast3():
    hr = lt.land_batch(3, 2, 192, 21)
    lt.check_conditions(hr, 4)
    assert np.isfinite(hr[0]).all() and 0.4 < np.isfinite(hr[1:]).mean() < 0.9
    return hr


@pytest.mark.parametrize("loss_fn", ["l2", "charbonnier"])
def test_land_trainer_step_vs_masked_oracle(coast3, loss_fn, monkeypatch):
    d = dev()
    model = ro.RCANOracle(nchannels_in=2, nchannels_out=2, nlayers=2, nblocks=2, nfeatures=64, cbottleneck=2)
    ro.init_params_numpy(model, 22)
    spec = rcan_spec(2, 2)
    table = param_table(spec)
    flat = flat_from_model(model, table).to(d)
    model = model.double()
    l_ref, _, g_ref = lt.train_step(model, coast3, 4, loss_fn)
    il_ref = lt.interp_loss(coast3, 4, loss_fn)
    bound = masked_drift_bounds(monkeypatch, model, coast3, 4, loss_fn, g_ref)
    tr = FusedTrainer(spec, 3, (48, 48), device=d, params=flat, loss_fn=loss_fn, land=True)
    hr_d = torch.tensor(coast3, device=d)
    out = tr.step(hr_d)
    torch.cuda.synchronize()
    loss, iloss = float(out["loss"]), float(out["interp_loss"])
    print(f"{loss_fn}: loss {loss:.6f} oracle {l_ref:.6f}; interp {iloss:.6f} oracle {il_ref:.6f}")
    assert abs(loss - l_ref) / l_ref < 2e-3
    assert abs(iloss - il_ref) / il_ref < 1e-5
    assert float(tr.loss4[1]) == float(np.isfinite(coast3).sum())  # the sr is finite everywhere
    assert torch.isfinite(tr.sr).all() and torch.isfinite(tr.lrbuf).all()
    assert (tr.dy.cpu().numpy()[~np.isfinite(coast3)].view(np.int32) == 0).all()
    grads = tr.grads.clone()
    g = grads.cpu()
    for name, off, n, shape in table:
        r = rel_l2(g[off:off + n].view(shape), g_ref[name])
        assert r <= bound[name], (name, r, bound[name])
    # another NaN on land: the same bits
    other = bits(hr_d).clone()
    other[torch.isnan(hr_d)] = -4194304 + 0x12345  # 0xffc12345: the sign bit and a payload
    other = other.view(torch.float32)
    assert torch.isnan(other).sum() == torch.isnan(hr_d).sum() and not torch.equal(bits(other), bits(hr_d))
    tr2 = FusedTrainer(spec, 3, (48, 48), device=d, params=flat, loss_fn=loss_fn, land=True)
    out2 = tr2.step(other)
    torch.cuda.synchronize()
    assert torch.equal(bits(out2["loss"]), bits(out["loss"])) and torch.equal(bits(tr2.grads), bits(grads))
    # one more step: the weights stay finite
    out = tr.step(hr_d)
    torch.cuda.synchronize()
    assert torch.isfinite(tr.params).all() and np.isfinite(float(out["loss"]))


@pytest.mark.parametrize("arch", ["edsr", "rcan"])
def test_land_trainer_fp32_step_vs_masked_oracle(coast3, arch):
    """The exact-fp32 engine -- EDSR, 2 ResBlocks, x4 (48 -> 192), the only case that takes
    land through the EDSR plan, and RCAN 2 x 2 beside it -- at the bars tests/test_gpu_fp32.py
    holds it to against plain fp64 (test_fp32_small_model_step_vs_golden): the loss and the
    output 1e-5 relative, every gradient tensor 1e-3 rel-L2."""
    d = dev()
    if arch == "edsr":
        model = ro.EDSROracle(nchannels_in=2, nchannels_out=2, nlayers=2, nfeatures=64, downscale_factors=[2, 2])
        spec = NetSpec(arch="edsr", nchannels_in=2, nchannels_out=2, nfeatures=64, nlayers=2, nblocks=0, cbottleneck=2,
                       scale=4, dtype="fp32")
    else:
        model = ro.RCANOracle(nchannels_in=2, nchannels_out=2, nlayers=2, nblocks=2, nfeatures=64, cbottleneck=2)
        spec = rcan_spec(2, 2, dtype="fp32")
    ro.init_params_numpy(model, 23)
    table = param_table(spec)
    tr = FusedTrainer(spec, 3, (48, 48), device=d, params=flat_from_model(model, table).to(d), land=True)
    l_ref, out_ref, g_ref = lt.train_step(model.double(), coast3, 4, "l2")
    out = tr.step(torch.tensor(coast3, device=d))
    torch.cuda.synchronize()
    assert abs(float(out["loss"]) - l_ref) / l_ref < 1e-5
    assert rel_l2(tr.sr, out_ref) < 1e-5
    g = tr.grads.cpu()
    worst = max(rel_l2(g[off:off + n].view(shape), g_ref[name]) for name, off, n, shape in table)
    print(f"fp32 {arch} engine with land: worst per-tensor grad rel-L2 {worst:.2e} (bar 1e-3)")
    assert worst < 1e-3


def test_land_trainer_without_the_interp_metric(coast3):
    """interp_loss=False: gparts is [loss | loss counts] instead of [loss | interp | loss
    counts | interp counts]; the loss and the gradient are those of the step with the metric."""
    spec = rcan_spec(1, 2)
    flat = init_flat(spec, 5)
    hr = torch.tensor(coast3, device=dev())
    res = []
    for interp in (True, False):
        tr = FusedTrainer(spec, 3, (48, 48), device=dev(), params=flat, land=True, interp_loss=interp)
        out = tr.step(hr)
        torch.cuda.synchronize()
        res.append((out["loss"].clone(), tr.grads.clone(), tr.loss4.clone()))
        del tr
    for a, b, what in zip(*res, ("loss", "grads", "loss4")):
        assert torch.equal(bits(a), bits(b)), what
    assert np.isfinite(float(res[0][0])) and float(res[0][2][1]) == float(np.isfinite(coast3).sum())


# ------------------------------------------------------ 7. micro-batch split with land
def test_land_micro_batch_split():
    """test_gpu_model.test_micro_batch_step_matches_single_engine's bars on a coast batch:
    the loss bit-identical (parts and counts in tile order), the gradients to 1e-5."""
    spec = rcan_spec(1, 2)
    flat = init_flat(spec, 5)
    hr_np = lt.land_batch(4, 2, 192, 24)
    lt.check_conditions(hr_np, 4)
    hr = torch.tensor(hr_np, device=dev())
    res = []
    for micro in (1, 2):
        tr = FusedTrainer(spec, 4, (48, 48), device=dev(), params=flat, micro=micro, land=True)
        out = tr.step(hr)
        torch.cuda.synchronize()
        res.append((float(out["loss"]), float(out["interp_loss"]), tr.grads.clone(), tr.params.clone()))
        del tr
    (l1, i1, g1, p1), (l2, i2, g2, p2) = res
    assert l1 == l2 and i1 == i2 and np.isfinite(l1)
    assert rel_l2(g2, g1) < 1e-5
    assert rel_l2(p2 - flat, p1 - flat) < 1e-4


# -------------------------------------------------------------------------- 8. feed
from test_gpu_feed import data, source  # noqa: E402,F401  (fixtures: the synthetic LLC files, land blocks and a NaN)


def test_land_feed_keeps_the_coastal_tiles(data, source):
    from srmi.feed import TimesliceFeed
    from srmi.llc import get_tiles, min_wet_pixels
    paths = data["paths"][:2]
    mw = min_wet_pixels(0.25, 64, 64)
    assert mw == 1024
    with TimesliceFeed(source, paths, 64, block_words=256, land=True, min_wet=0.25) as feed, \
            TimesliceFeed(source, paths, 64, block_words=256) as plain:
        for i, p in enumerate(paths):
            region = source.load_region_data(p)
            tiles, ids, grid = feed.timeslice(i)
            ref_t, ref_ids = lt.get_tiles(region.cpu().numpy(), 64, 64, mw)
            assert same_bits(tiles.cpu().numpy(), ref_t) and np.array_equal(ids, ref_ids)
            gt, gids, ggrid = get_tiles(region, 64, 64, min_wet=0.25)
            assert torch.equal(bits(gt), bits(tiles)) and np.array_equal(gids, ids) and ggrid == grid
            pt, pids, _ = plain.timeslice(i)
            et, eids, _ = get_tiles(region, 64, 64)  # land=False: what it gives today
            assert torch.equal(bits(pt), bits(et)) and np.array_equal(pids, eids)
            assert tiles.shape[0] > pt.shape[0] and torch.isnan(tiles).any() and not torch.isnan(pt).any()
        with pytest.raises(ValueError, match="land=False"):
            feed.norm_stats()


def test_training_over_the_land_feed(data, source, tmp_path):
    from srmi.batch import prep_batch
    from srmi.feed import TimesliceFeed
    from srmi.harness import LossRecords, train_timeslices
    spec = rcan_spec(1, 2, scale=2)
    flat = init_flat(spec, 7)
    paths = data["paths"][:2]
    rec = []
    with TimesliceFeed(source, paths, 64, block_words=256, land=True, min_wet=0.25) as feed:
        tr = FusedTrainer(spec, 4, (32, 32), device=dev(), params=flat, land=True)
        prep = feed.prepare("lnorm", scale=2)
        step = tr.step

        def prepare(raw, start, gb, flip):
            rec.append([raw.clone(), flip, tr.params.clone(), None])
            return prep(raw, start, gb, flip)

        def recording_step(hr, shard=None):
            out = step(hr)
            rec[-1][3] = out["loss"].clone()
            return out
        tr.step = recording_step
        root = str(tmp_path / "land")
        out = train_timeslices(tr, feed.timeslices(), 2, 4, records=LossRecords(root, "ds", "t", "m"),
                               refresh_state=True, rng=random.Random(9), prepare=prepare, xyflip=True)
        torch.cuda.synchronize()
    assert np.isfinite(out["prediction"]) and np.isfinite(out["interpolated"])
    assert len(LossRecords(root, "ds", "t", "m").load_results()) == 2
    assert len(rec) == 14 and any(torch.isnan(r[0]).any() for r in rec) and len({r[1] for r in rec}) > 1
    one = FusedTrainer(spec, 4, (32, 32), device=dev(), params=flat, land=True)
    for k, (raw, flip, params, loss) in enumerate(rec):
        one.params.copy_(params)
        for e in one.engines:
            e.pack(one.params)
        got = one.step(prep_batch(raw, flip, 2, with_lr=False, land=True)["hr"])["loss"]
        torch.cuda.synchronize()
        assert np.isfinite(float(loss)) and torch.equal(bits(got), bits(loss)), k


# ----------------------------------------------------------------- 9. data parallel
def _dp_worker(rank, port, q, reducer_stream):
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(root, "super-resolution-climate_amd"), root, os.path.join(root, "tests")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK="0")
    import torch.distributed as dist
    from srmi.dist import init_from_env, shard_range
    info = init_from_env("gloo")
    d = torch.device("cuda", 0)
    torch.cuda.set_device(d)
    spec = rcan_spec(1, 2)
    flat = init_flat(spec, 5)
    hr_all = torch.tensor(lt.land_batch(4, 2, 192, 25), device=d)
    a, b = shard_range(4, info)
    tr = FusedTrainer(spec, b - a, (48, 48), device=d, params=flat, micro=2, info=info, land=True,
                      dp_reducer_stream=reducer_stream)
    out = tr.step(hr_all[a:b].contiguous())
    torch.cuda.synchronize()
    q.put((rank, float(out["loss"]), float(out["interp_loss"]), tr.grads.cpu().numpy(), tr.params.cpu().numpy()))
    dist.destroy_process_group()


@pytest.mark.parametrize("reducer_stream", [False, True])
def test_land_dp_world2_matches_single_process(reducer_stream):
    """tests/test_gpu_dp.py's conventions (gloo, both ranks on cuda:0) on the coast batch:
    rank 0 holds the all-wet tile, so the ranks' counts differ; the loss parts and the
    counts go through the one all-reduce, and the loss is the one-process loss bit for bit,
    the gradient within that file's world-2 bar (2e-4 rel-L2: fp32 summation order)."""
    import multiprocessing as mp
    hr_np = lt.land_batch(4, 2, 192, 25)
    lt.check_conditions(hr_np, 4)
    wet = np.isfinite(hr_np).sum(axis=(1, 2, 3))
    assert wet[0] == hr_np[0].size and wet[:2].sum() != wet[2:].sum()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 45000 + random.randint(0, 2000)
    ps = [ctx.Process(target=_dp_worker, args=(r, port, q, reducer_stream)) for r in range(2)]
    for p in ps:
        p.start()
    res = sorted([q.get(timeout=100) for _ in ps], key=lambda t: t[0])
    for p in ps:
        p.join(timeout=30)
        assert p.exitcode == 0
    d = dev()
    spec = rcan_spec(1, 2)
    tr = FusedTrainer(spec, 4, (48, 48), device=d, params=init_flat(spec, 5), micro=1, land=True)
    out = tr.step(torch.tensor(hr_np, device=d))
    torch.cuda.synchronize()
    loss, iloss, g = float(out["loss"]), float(out["interp_loss"]), tr.grads.cpu().numpy()
    for rank, l_r, il_r, g_r, p_r in res:
        assert l_r == loss and il_r == iloss, (rank, l_r, loss, il_r, iloss)
        assert np.linalg.norm(g_r - g) / np.linalg.norm(g) < 2e-4
    np.testing.assert_array_equal(res[0][4], res[1][4])  # replicas stay identical after Adam
