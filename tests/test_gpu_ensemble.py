"""Geometric self-ensemble on the HIP path: the dihedral variants of tile planes
(srmi_tiles_dihedral), the blend of their back-transformed outputs into a mean and a
spread (srmi_tiles_blend_ensemble), and RegionSuperResolver(ensemble=...) end to end,
against the existing blends (bit for bit where the variants are transforms of one tile)
and the fp64 oracle (tests/ensemble_oracle.py).

Bars, derived, not measured.  srmi_tiles_dihedral is a permutation: bit for bit.  Every
B_j is a value of srmi_tiles_blend and carries its 16 * 2^-24 * M (test_gpu_overlap.py; M
here is that bound's scale maximised over the K slabs).  The mean adds K - 1 additions and
one division, at most K roundings of values no larger than M:
    |mean - oracle| <= (16 + K) * 2^-24 * M.
The RMS over j is 1-Lipschitz in the vector (B_j - mean), every component of which is off
by at most the sum of the two bars above, 2 * (16 + K) * 2^-24 * M rounded up; the division
by K and the square root add two roundings:
    |spread - oracle| <= 2 * (17 + K) * 2^-24 * M."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ensemble_oracle as eo  # noqa: E402
import overlap_oracle as oo  # noqa: E402
from srmi import _lib  # noqa: E402
from srmi._lib import call, ptr  # noqa: E402
from srmi.engine import Engine  # noqa: E402
from srmi.superres import RegionSuperResolver, ensemble_variants, overlap_count  # noqa: E402
from test_ensemble_oracle import superres_results_round_trip  # noqa: E402
from test_gpu_inference import _small_rcan  # noqa: E402
from test_gpu_land import blend_masked_dev  # noqa: E402
from test_gpu_overlap import _field, bits, blend_dev, dev, f64, st  # noqa: E402

U = 2.0 ** -24
NAN_BITS = 0x7fc00000


def popcount(m):
    return bin(m).count("1")


def dihedral_dev(x, mask):
    """srmi_tiles_dihedral of a device tensor [..., h, w] -> [K, ..., h, w]."""
    x = x.contiguous()
    out = torch.full((popcount(mask),) + tuple(x.shape), -7.0, device=x.device)
    call("srmi_tiles_dihedral", ptr(x), x.numel() // (x.shape[-1] * x.shape[-2]), x.shape[-2], x.shape[-1], mask,
         ptr(out), st())
    return out


def ensemble_dev(tiles, mask, off, div, bad, C, Ty, Tx, Sy, Sx, Ho, Wo, mask_src=None, scale=1):
    mean = torch.full((C, Ho, Wo), -7.0, device=tiles.device)
    spread = torch.full((C, Ho, Wo), -7.0, device=tiles.device)
    call("srmi_tiles_blend_ensemble", ptr(tiles), mask, ptr(off), ptr(div), ptr(bad), C, Ty, Tx, Sy, Sx, Ho, Wo,
         ptr(mask_src), scale, ptr(mean), ptr(spread), st())
    return mean, spread


def assert_ensemble_close(mean, spread, ref_mean, ref_spread, M, K, what=""):
    """NaN exactly where the oracle has it; elsewhere within the bars of the module docstring."""
    nan = np.isnan(ref_mean)
    assert (np.isnan(ref_spread) == nan).all()
    for name, got, ref, bar in (("mean", mean, ref_mean, 16 + K), ("spread", spread, ref_spread, 2 * (17 + K))):
        got = np.asarray(got, np.float64)
        assert (np.isnan(got) == nan).all(), name
        err = np.abs(got - ref)[~nan]
        print(f"{what}{name}: max err / (2^-24 M) = {float((err / (U * np.maximum(M[~nan], 1e-300))).max()):.3f} over "
              f"{err.size} pixels (bar {bar})")
        assert (err <= bar * U * M[~nan]).all(), name


# --------------------------------------------------------------- 1. the variants, bit for bit
def _planes(rng, nplanes, h, w):
    x = rng.randn(nplanes, h, w).astype(np.float32)
    x[0, 1, 2] = -0.0
    x[-1, h - 1, 0] = np.nan
    b = x.view(np.int32)
    b[1, h // 2, w - 1] = 0x7fc12345  # a NaN with a payload
    b[0, 0, w // 2] = np.int32(-0x3fedcb)  # 0xffc01235: a negative one
    return x


# 16^2, 48^2: the float4 form; 50^2: the scalar one; 80^2, 68 x 132, 70 x 130: more than one
# 64 x 64 block, with partial ones, in both forms
@pytest.mark.parametrize("h,w,mask", [(16, 16, 0xff), (16, 16, 0b10010001), (16, 16, 1), (48, 48, 0xff),
                                      (48, 48, 0b10010001), (48, 48, 1), (50, 50, 0xff), (50, 50, 0b10010001),
                                      (50, 50, 1), (16, 24, 0b1111), (80, 80, 0xff), (68, 132, 0b1111),
                                      (70, 130, 0b1110)])
def test_dihedral_is_bit_exact(h, w, mask):
    x = _planes(np.random.RandomState(71), 3, h, w)
    out = dihedral_dev(torch.tensor(x, device=dev()), mask)
    ref = eo.expand(x.view(np.int32), mask)
    assert np.array_equal(bits(out).cpu().numpy(), ref)


def test_dihedral_misaligned_buffers_take_the_scalar_form():
    x = _planes(np.random.RandomState(72), 3, 16, 16)
    buf_in = torch.zeros(3 * 256 + 1, device=dev())
    buf_out = torch.zeros(8 * 3 * 256 + 1, device=dev())
    buf_in[1:].copy_(torch.tensor(x, device=dev()).reshape(-1))
    call("srmi_tiles_dihedral", buf_in.data_ptr() + 4, 3, 16, 16, 0xff, buf_out.data_ptr() + 4, st())
    assert np.array_equal(bits(buf_out[1:]).cpu().numpy().reshape(8, 3, 16, 16), eo.expand(x.view(np.int32), 0xff))


def test_dihedral_of_the_recorded_xyflip_input():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "xyflip.npz"))
    out = dihedral_dev(torch.tensor(z["input"].astype(np.float32), device=dev()), 0xff).cpu().numpy()
    assert out.shape == (8, 2, 2, 8, 8)
    for f in range(8):
        assert np.array_equal(out[f], z[f"flip{f}"].astype(np.float32)), f


def test_dihedral_refusals():
    lib = _lib.load()
    d = dev()
    sq, rect = torch.full((3, 16, 16), 3.0, device=d), torch.full((3, 16, 24), 3.0, device=d)
    out = torch.full((8, 3, 16, 24), 3.0, device=d)

    def run(x, mask, o=out, n=3):
        return lib.srmi_tiles_dihedral(ptr(x), n, x.shape[1], x.shape[2], mask, ptr(o), st())

    for m in (0b10000, 0b11111, 0xff):
        assert run(rect, m) == -10002, m  # SRMI_ERR_SHAPE: a swap of a rectangular plane
    assert run(sq, 1, n=0) == -10002
    for m in (0, 256, -1):
        assert run(sq, m) == _lib.SRMI_ERR_ARG, m
    assert run(sq, 1, o=sq) == _lib.SRMI_ERR_ARG
    assert lib.srmi_tiles_dihedral(None, 3, 16, 16, 1, ptr(out), st()) == _lib.SRMI_ERR_ARG
    assert lib.srmi_tiles_dihedral(ptr(sq), 3, 16, 16, 1, None, st()) == _lib.SRMI_ERR_ARG
    torch.cuda.synchronize()
    assert float(out.min()) == float(out.max()) == 3.0  # nothing was written
    assert run(rect, 0b1111) == 0 and run(sq, 0xff) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------- 2. the round trip closes the maps
def _plan_inputs(rng, hw, T, stride, C, with_bad=True):
    Ty, Tx = T
    n = overlap_count(hw[0], Ty, stride[0]) * overlap_count(hw[1], Tx, stride[1])
    tiles = rng.randn(n, C, Ty, Tx).astype(np.float32)
    off = (rng.randn(n, C) * 2 + 1).astype(np.float32)
    div = (rng.rand(n, C) + 0.5).astype(np.float32)
    bad = (rng.rand(n) < 0.3).astype(np.int32) if with_bad else None
    if with_bad:
        bad[0], bad[n // 2] = 1, 0  # the corner pixel has tile 0 alone: it is left without a cover
        tiles[bad != 0] = np.nan  # what a bad tile may hold: it must never be read into a sum
    return n, tiles, off, div, bad


def _lr_mask(rng, C, hw, scale):
    m = rng.randn(C, hw[0] // scale, hw[1] // scale).astype(np.float32)
    m[rng.rand(*m.shape) < 0.1] = np.nan
    m[0, 0, 0] = np.inf
    return m


# (40 x 54, T 16, S 12): the scalar form; (40 x 56, T 16, S 12): the quad form -- both with a
# triple cover; (40 x 88, T 16 x 32, S (12, 28)): rectangular tiles, the flips alone
@pytest.mark.parametrize("hw,T,stride,masks,scale", [
    ((40, 54), (16, 16), (12, 12), (1, 0b100001, 0b11000011, 0xff), 2),
    ((40, 56), (16, 16), (12, 12), (1, 0b100001, 0b11000011, 0xff), 4),
    ((40, 88), (16, 32), (12, 28), (0b1111,), 4)])
@pytest.mark.parametrize("masked", [False, True])
def test_round_trip_is_the_plain_blend_and_no_spread(hw, T, stride, masks, scale, masked):
    d = dev()
    rng = np.random.RandomState(73)
    C = 2
    n, tiles, off, div, bad = _plan_inputs(rng, hw, T, stride, C)
    t, o, dv, b = (torch.tensor(a, device=d) for a in (tiles, off, div, bad))
    msk = torch.tensor(_lr_mask(rng, C, hw, scale), device=d) if masked else None
    if masked:
        ref = blend_masked_dev(t, o, dv, b, C, *T, *stride, *hw, msk, scale)
    else:
        ref = blend_dev(t, o, dv, b, C, *T, *stride, *hw)
    finite = torch.isfinite(ref)
    assert bool(finite.any()) and not bool(finite.all())
    for m in masks:
        vt = dihedral_dev(t, m)  # scale 1: the "model" is the identity
        mean, spread = ensemble_dev(vt, m, o, dv, b, C, *T, *stride, *hw, msk, scale)
        assert torch.equal(bits(mean), bits(ref)), (m, "mean")
        sb = bits(spread)
        assert bool((sb[finite] == 0).all()) and bool(torch.isnan(spread[~finite]).all()), (m, "spread")
        # no denorm: the stored values
        if not masked:
            mean, spread = ensemble_dev(vt, m, None, None, b, C, *T, *stride, *hw)
            assert torch.equal(bits(mean), bits(blend_dev(t, None, None, b, C, *T, *stride, *hw))), (m, "no denorm")
            assert bool((bits(spread)[finite] == 0).all())


# ----------------------------------------------------------- 3. independent slabs vs the oracle
# the plans of test_gpu_overlap's blend test (scalar; quad; misaligned strides), and for the
# mask at scale 4 -- Ho, Wo multiples of 4 -- the quad plan, its x4 form and a scalar one
PLANS = [((40, 54), 16, (12, 12), False), ((40, 56), 16, (12, 12), False), ((41, 55), 16, (5, 7), False),
         ((40, 56), 16, (12, 12), True), ((160, 216), 64, (48, 48), True), ((44, 60), 16, (5, 7), True)]


@pytest.mark.parametrize("hw,T,stride,masked", PLANS)
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("vmask", [0xff, 0b00100101])
@pytest.mark.parametrize("with_bad", [False, True])
def test_independent_slabs_match_the_oracle(hw, T, stride, masked, C, vmask, with_bad):
    d = dev()
    rng = np.random.RandomState(74)
    K = popcount(vmask)
    n, _, off, div, bad = _plan_inputs(rng, hw, (T, T), stride, C, with_bad)
    tiles = rng.randn(K, n, C, T, T).astype(np.float32)
    if with_bad:
        tiles[:, bad != 0] = np.nan
    msk = _lr_mask(rng, C, hw, 4) if masked else None
    mean, spread = ensemble_dev(torch.tensor(tiles, device=d), vmask, torch.tensor(off, device=d),
                                torch.tensor(div, device=d), torch.tensor(bad, device=d) if with_bad else None, C, T, T,
                                *stride, *hw, torch.tensor(msk, device=d) if masked else None, 4)
    ref_m, ref_s, M = eo.blend_ensemble(tiles.astype(np.float64), vmask, off.astype(np.float64),
                                        div.astype(np.float64), bad, *stride, *hw, mask=msk, scale=4)
    assert np.isnan(ref_m).any() == (with_bad or masked)
    assert_ensemble_close(mean.cpu().numpy(), spread.cpu().numpy(), ref_m, ref_s, M, K)
    nan = np.isnan(ref_m)
    assert (bits(mean).cpu().numpy()[nan] == NAN_BITS).all() and (bits(spread).cpu().numpy()[nan] == NAN_BITS).all()


def test_spread_is_optional_and_refusals():
    d = dev()
    lib = _lib.load()
    rng = np.random.RandomState(75)
    n, tiles, off, div, _ = _plan_inputs(rng, (40, 56), (16, 16), (12, 12), 1, False)
    vt = dihedral_dev(torch.tensor(tiles, device=d), 0xff)
    o, dv = torch.tensor(off, device=d), torch.tensor(div, device=d)
    mean, _ = ensemble_dev(vt, 0xff, o, dv, None, 1, 16, 16, 12, 12, 40, 56)
    out = torch.full((1, 40, 56), 3.0, device=d)
    msk = torch.zeros((1, 10, 14), device=d)

    def run(variants=0xff, C=1, Ty=16, Tx=16, Sy=12, Sx=12, Ho=40, Wo=56, mask_src=None, scale=4, mean=out, tl=vt):
        return lib.srmi_tiles_blend_ensemble(ptr(tl), variants, ptr(o), ptr(dv), None, C, Ty, Tx, Sy, Sx, Ho, Wo,
                                             ptr(mask_src), scale, ptr(mean), None, st())

    for kw in (dict(variants=0), dict(variants=256), dict(variants=-1), dict(Sy=0), dict(Sx=17), dict(Ho=15),
               dict(C=0), dict(mean=None), dict(tl=None), dict(mask_src=msk, scale=0), dict(mask_src=msk, scale=3)):
        assert run(**kw) == _lib.SRMI_ERR_ARG, kw
    for kw in (dict(Ty=12, Sy=12), dict(variants=0b10000, Ty=12, Sy=12)):  # a swap of a rectangular tile
        assert run(**kw) == -10002, kw
    torch.cuda.synchronize()
    assert float(out.min()) == float(out.max()) == 3.0  # nothing was written
    assert run(scale=-5) == 0  # no spread, no mask: scale is ignored
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(mean))


# ------------------------------------------------------------------------- 4. end to end
LR_SHAPE, TILE32, OVERLAP = (1, 72, 88), (32, 32), (8, 8)  # 32^2: the smallest square tile the engine takes


def _transformed(tiles, variants):
    """torch's own flips and transposes of [n, C, t, t] -> [K, n, C, t, t]."""
    out = []
    for f in variants:
        x = tiles
        if f & 1:
            x = torch.flip(x, dims=[-1])
        if f & 2:
            x = torch.flip(x, dims=[-2])
        if f & 4:
            x = x.transpose(-1, -2)
        out.append(x.contiguous())
    return torch.stack(out)


_E2E = {}


def e2e():
    """The ensemble=8 run every end-to-end check shares (made once, never changed)."""
    if not _E2E:
        d = dev()
        spec, model, flat = _small_rcan()
        lr = torch.tensor(_field(np.random.RandomState(76), *LR_SHAPE), device=d)
        rs = RegionSuperResolver(spec, flat.to(d), LR_SHAPE, tile_lr=TILE32, overlap=OVERLAP, device=d, ensemble=8)
        images = {k: v.clone() for k, v in rs.super_resolve(lr).items()}
        _E2E.update(spec=spec, flat=flat.to(d), lr=lr, rs=rs, images=images)
    return _E2E


def make(e, lr_shape=LR_SHAPE, tile=TILE32, **kw):
    return RegionSuperResolver(e["spec"], e["flat"], lr_shape, tile_lr=tile, overlap=OVERLAP, device=dev(), **kw)


def test_super_resolve_ensemble_end_to_end():
    e = e2e()
    rs, images, d = e["rs"], e["images"], dev()
    assert (rs.ny, rs.nx, rs.sy, rs.sx, rs.K, rs.vmask, rs.nfwd) == (3, 4, 24, 24, 8, 0xff, 96)
    assert tuple(rs.sr.shape) == (8, 12, 1, 128, 128) and tuple(images["spread"].shape) == (1, 288, 352)
    # (a) the engine's own outputs of torch's transforms of the cut tiles, blended by the oracle
    vt = _transformed(rs.tiles, rs.variants)
    assert torch.equal(bits(vt), bits(rs.vtiles))
    eng = Engine(e["spec"], 96, TILE32, train=False, device=d)
    eng.pack(e["flat"])
    sr = eng.forward(e["flat"], vt.view(96, 1, 32, 32))
    assert torch.equal(bits(sr), bits(rs.sr.view(96, 1, 128, 128)))
    ref_m, ref_s, M = eo.blend_ensemble(f64(rs.sr), rs.variants, f64(rs.off), f64(rs.div), rs.bad.cpu().numpy(), 96, 96,
                                        288, 352)
    model, spread = images["model"].cpu().numpy(), images["spread"].cpu().numpy()
    assert_ensemble_close(model, spread, ref_m, ref_s, M, 8)
    # (b) the network is not equivariant: the variants disagree
    assert np.isfinite(model).all() and np.isfinite(spread).all() and (spread >= 0).all() and spread.max() > 0
    print(f"spread: median {np.median(spread):.3e} max {spread.max():.3e}; |model| median {np.median(np.abs(model)):.3e}")


@pytest.mark.parametrize("kw", [dict(micro=2), dict(max_batch=5), dict(graph=True)])
def test_ensemble_engines_chunks_and_graph_change_no_bit(kw):
    e = e2e()
    rs2 = make(e, ensemble=8, **kw)
    for _ in range(2):  # graph: the capture's warm-up, then a replay
        im = rs2.super_resolve(e["lr"])
        for k in ("model", "spread", "interpolated"):
            assert torch.equal(bits(im[k]), bits(e["images"][k])), (kw, k)


def test_ensemble_one_is_the_object_as_it_was():
    e = e2e()
    a, b = make(e).super_resolve(e["lr"]), make(e, ensemble=1).super_resolve(e["lr"])
    assert sorted(a) == sorted(b) == ["input", "interpolated", "model"]
    for k in ("model", "interpolated"):
        assert torch.equal(bits(a[k]), bits(b[k])), k
    assert torch.equal(bits(a["interpolated"]), bits(e["images"]["interpolated"]))


def test_ensemble_of_chosen_variants_is_the_abi_with_their_mask():
    e = e2e()
    d = dev()
    rs = make(e, ensemble=(3, 0))
    assert rs.variants == ensemble_variants((0, 3), TILE32) == (0, 3) and rs.vmask == 0b1001
    im = rs.super_resolve(e["lr"])
    vt = dihedral_dev(rs.tiles, 0b1001)
    assert torch.equal(bits(vt), bits(_transformed(rs.tiles, (0, 3))))
    eng = Engine(e["spec"], 24, TILE32, train=False, device=d)
    eng.pack(e["flat"])
    sr = eng.forward(e["flat"], vt.view(24, 1, 32, 32))
    mean, spread = ensemble_dev(sr, 0b1001, rs.off, rs.div, rs.bad, 1, 128, 128, 96, 96, 288, 352)
    assert torch.equal(bits(mean), bits(im["model"])) and torch.equal(bits(spread), bits(im["spread"]))


def test_ensemble_on_a_rectangular_tile():
    e = e2e()
    rs = make(e, tile=(16, 32), ensemble=4)
    assert rs.variants == (0, 1, 2, 3)
    im = rs.super_resolve(e["lr"])
    s = rs.s
    ref_m, ref_s, M = eo.blend_ensemble(f64(rs.sr), rs.variants, f64(rs.off), f64(rs.div), rs.bad.cpu().numpy(),
                                        rs.sy * s, rs.sx * s, 288, 352)
    assert_ensemble_close(im["model"].cpu().numpy(), im["spread"].cpu().numpy(), ref_m, ref_s, M, 4)
    with pytest.raises(ValueError, match="ensemble=4"):
        make(e, tile=(16, 32), ensemble=8)
    with pytest.raises(ValueError):
        make(e, ensemble=3)


# --------------------------------------------------------------------------------- 5. land
def test_ensemble_with_land():
    e = e2e()
    lr = e["lr"].clone()
    lr[0, 30:38, 40:48] = float("nan")  # an 8 x 8 patch
    lr[0, :, 80] = float("nan")  # a coastline column
    rs = make(e, land=True, min_wet=0.25, ensemble=8)
    im = rs.super_resolve(lr)
    one = make(e, land=True, min_wet=0.25).super_resolve(lr)["model"]
    nan = torch.isnan(one)
    assert bool(nan.any()) and torch.equal(torch.isnan(im["model"]), nan) and torch.equal(torch.isnan(im["spread"]), nan)
    assert torch.equal(bits(rs.vtiles), bits(_transformed(rs.tiles, rs.variants)))  # transforms of the FILLED tile
    off, div = np.nan_to_num(f64(rs.off)), np.nan_to_num(f64(rs.div))
    ref_m, ref_s, M = eo.blend_ensemble(f64(rs.sr), rs.variants, off, div, rs.bad.cpu().numpy(), 96, 96, 288, 352,
                                        mask=lr.cpu().numpy(), scale=4)
    assert_ensemble_close(im["model"].cpu().numpy(), im["spread"].cpu().numpy(), ref_m, ref_s, M, 8, "land ")
    assert torch.equal(bits(im["interpolated"]), bits(make(e, land=True).super_resolve(lr)["interpolated"]))


# ------------------------------------------------------------------------------ 6. results
def test_results_round_trip_spread(tmp_path):
    superres_results_round_trip(tmp_path, e2e()["images"], ["SST"])
