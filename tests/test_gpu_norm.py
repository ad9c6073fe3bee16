"""The six task.norm modes and the dataset tile statistics on the device
(srmi_tile_stats, srmi_tile_stats_finalize, srmi_batch_prep_norm,
srmi_region_to_tiles_norm through the C ABI; srmi.norm, srmi.batch.prep_batch and
srmi.inference.TiledInference above them) against the fp64 restatement of the
reference in tests/norm_oracle.py.

Inputs are mu + sd * N(0, 1) with (mu, sd) = (290, 0.7) (a temperature in K),
(35, 0.05) (a salinity) and (-3, 2), where whole tiles are negative (a max that
starts at 0 instead of -inf fails there).

Bars (ulp = the spacing of fp32 at the value named):
* statistics: the kernel accumulates in fp64 and rounds once, so the mean is
  within 4 ulps of max(|mean|, sd), the variance within 4 ulps of itself, and max
  and min are exact;
* AFFINE / LSCALE closure: hr is fp32(((double)x - off) / div) of the very off /
  div arrays, within 2 ulps of that value on every element (the kernel multiplies
  by the fp64 reciprocal: one more fp32 ulp at the most after rounding; LSCALE
  divides by the exact fp64 max - min, whose fp32 rounding is the div it reports:
  a relative 2^-24, one ulp);
* the fused LR tile against srmi_downsample of the produced HR tile: 1e-6
  absolute, the bar tests/test_gpu_batch.py holds 'lnorm' to.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import norm_oracle as no  # noqa: E402
from oracle import rcan_oracle as ro  # noqa: E402
from srmi import _lib  # noqa: E402
from srmi._lib import call, ptr  # noqa: E402
from srmi.batch import prep_batch  # noqa: E402
from srmi.engine import NetSpec, downsample, param_table  # noqa: E402
from srmi.norm import ATTR_KEYS, NORM_TYPES, NormStats, normalize_tiles  # noqa: E402

MUSD = [(290.0, 0.7), (35.0, 0.05), (-3.0, 2.0)]
LNORM, LSCALE, AFFINE = _lib.SRMI_NORM_LNORM, _lib.SRMI_NORM_LSCALE, _lib.SRMI_NORM_AFFINE


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def S():
    return torch.cuda.current_stream().cuda_stream


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def field(shape, mu, sd, seed):
    return (mu + sd * np.random.RandomState(seed).standard_normal(shape)).astype(np.float32)


def assert_ulps(got, ref, nulp, at=None, what=""):
    """|got - ref| <= nulp fp32 ulps at |ref| (or at `at`), elementwise; ref fp64."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - ref)
    bar = nulp * ulp32(ref if at is None else at)
    worst = float(np.max(err / bar)) if err.size else 0.0
    print(f"{what}: worst {worst * nulp:.3f} ulps (bar {nulp})")
    assert np.all(err <= bar), f"{what}: {worst * nulp:.3f} ulps > {nulp}"


# ------------------------------------------------------------------ statistics
def stats_oracle(slices):
    """norm_oracle.compute_normalization in fp64."""
    return no.compute_normalization([s.astype(np.float64) for s in slices])


def check_stats(tstats, gstats, slices, sd):
    ref = stats_oracle(slices)
    t = tstats.cpu().numpy()
    assert_ulps(t[..., 0], ref[..., 0], 4, at=np.maximum(np.abs(ref[..., 0]), sd), what="tile mean")
    assert_ulps(t[..., 1], ref[..., 1], 4, what="tile var")
    assert np.array_equal(t[..., 2], ref[..., 2].astype(np.float32)), "tile max is not exact"
    assert np.array_equal(t[..., 3], ref[..., 3].astype(np.float32)), "tile min is not exact"
    gref = no.globalize_norm(ref)
    g = gstats.cpu().numpy()
    assert_ulps(g[..., 0], gref[..., 0], 4, at=np.maximum(np.abs(gref[..., 0]), sd), what="global mean")
    assert_ulps(g[..., 1], gref[..., 1], 4, what="global var")
    assert np.array_equal(g[..., 2:], gref[..., 2:].astype(np.float32)), "global max / min are not exact"


# (n, C, ty, tx): one wave per plane with a 16-byte load straddling rows; 256 threads;
# 1024 threads; a plane count past 65 535; an odd plane and a 256^2 plane (scalar kernel)
STAT_SHAPES = [(5, 2, 6, 6), (7, 1, 48, 48), (3, 3, 192, 192), (66000, 1, 4, 4), (3, 2, 5, 5), (2, 1, 256, 256)]


@pytest.mark.parametrize("musd", MUSD, ids=lambda m: f"mu{m[0]:g}")
@pytest.mark.parametrize("shape", STAT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tile_stats(shape, musd):
    d = dev()
    mu, sd = musd
    n, C, ty, tx = shape
    slices = [field(shape, mu, sd, 100 + i) for i in range(3)]
    for s in slices:
        s[0, 0] = np.float32(mu + 0.25)  # one constant plane
    dsl = [torch.tensor(s, device=d) for s in slices]
    acc = torch.full((n, C, 4), float("nan"), dtype=torch.float64, device=d)  # dirty
    acc[::2] = 1e30
    tst = torch.empty(n, C, 4, device=d)
    gst = torch.empty(C, 4, device=d)
    runs = []
    for rep in range(2):  # the second pass starts from the first pass's acc with first = 1
        got = {}
        for i, t in enumerate(dsl):
            call("srmi_tile_stats", ptr(t), n, C, ty, tx, ptr(acc), int(i == 0), S())
            if i in (0, 2):
                call("srmi_tile_stats_finalize", ptr(acc), n, C, i + 1, ptr(tst), ptr(gst), S())
                got[i + 1] = (tst.clone(), gst.clone())
        runs.append(got)
    torch.cuda.synchronize()
    for nt in (1, 3):
        t, g = runs[0][nt]
        check_stats(t, g, slices[:nt], sd)
        assert float(t[0, 0, 1]) == 0.0 and float(t[0, 0, 2]) == float(t[0, 0, 3]) == float(np.float32(mu + 0.25))
        assert float(t[0, 0, 0]) == float(np.float32(mu + 0.25))
        assert torch.equal(t, runs[1][nt][0]) and torch.equal(g, runs[1][nt][1]), "two runs differ"


def test_tile_stats_rejects_bad_args():
    d = dev()
    t = torch.zeros(2, 1, 4, 4, device=d)
    acc = torch.zeros(2, 1, 4, dtype=torch.float64, device=d)
    with pytest.raises(_lib.SrmiError):
        call("srmi_tile_stats", ptr(t), 0, 1, 4, 4, ptr(acc), 1, S())
    with pytest.raises(_lib.SrmiError):
        call("srmi_tile_stats", ptr(t), 2, 1, 4, 4, None, 1, S())
    with pytest.raises(_lib.SrmiError):
        call("srmi_tile_stats_finalize", ptr(acc), 2, 1, 0, None, None, S())


# ------------------------------------------------------------ batch preparation
def prep_norm_abi(raw, flip, scale, mode, off=None, div=None, with_lr=True):
    d = raw.device
    B, C, T, _ = raw.shape
    hr = torch.empty_like(raw)
    lr = torch.empty(B, C, T // scale, T // scale, device=d) if with_lr else None
    oo, do = torch.full((B, C), -7.0, device=d), torch.full((B, C), -7.0, device=d)
    call("srmi_batch_prep_norm", ptr(raw), B, C, T, flip, scale, mode, ptr(off), ptr(div), ptr(hr), ptr(lr),
         ptr(oo), ptr(do), S())
    return hr, lr, oo, do


def closure(raw, off, div, flip):
    """fp32(((double)x - off) / div), flipped: the value the kernel is held to."""
    x = raw.astype(np.float64)
    z = (x - off.astype(np.float64)[:, :, None, None]) / div.astype(np.float64)[:, :, None, None]
    return ro.xyflip(z, flip).astype(np.float32).astype(np.float64)


def check_lr(hr, lr, scale):
    lr2 = downsample(hr, scale)
    torch.cuda.synchronize()
    assert float((lr - lr2).abs().max()) < 1e-6


def affine_stats(B, C, mu, sd, seed):
    rng = np.random.RandomState(seed)
    off = (mu + sd * 0.3 * rng.standard_normal((B, C))).astype(np.float32)
    div = (sd * rng.uniform(0.8, 1.25, (B, C))).astype(np.float32)
    return off, div


# T = 6: a 16-byte load straddles rows; 192: the largest LDS tile; 256: the no-LDS path
@pytest.mark.parametrize("musd", MUSD, ids=lambda m: f"mu{m[0]:g}")
@pytest.mark.parametrize("T,scale,B,C", [(6, 2, 3, 2), (48, 2, 3, 2), (48, 4, 3, 2), (192, 2, 2, 2), (192, 4, 2, 2),
                                         (256, 2, 2, 1), (256, 4, 2, 1)])
def test_affine_closure_all_flips(T, scale, B, C, musd):
    d = dev()
    mu, sd = musd
    raw = field((B, C, T, T), mu, sd, 7 * T + scale)
    off, div = affine_stats(B, C, mu, sd, T)
    rd, od, dd = (torch.tensor(a, device=d) for a in (raw, off, div))
    for f in range(8):
        hr, lr, oo, do = prep_norm_abi(rd, f, scale, AFFINE, od, dd)
        assert_ulps(hr.cpu().numpy(), closure(raw, off, div, f), 2, what=f"hr T={T} flip={f}")
        check_lr(hr, lr, scale)
        assert float(oo.min()) == -7.0 == float(do.max())  # AFFINE writes no statistics


@pytest.mark.parametrize("mode", [AFFINE, LSCALE])
def test_whole_time_slice_past_65535_tiles(mode):
    d = dev()
    mu, sd = MUSD[0]
    B = 66000
    raw = field((B, 1, 4, 4), mu, sd, 5)
    off, div = affine_stats(B, 1, mu, sd, 6)
    rd = torch.tensor(raw, device=d)
    if mode == AFFINE:
        hr, _, _, _ = prep_norm_abi(rd, 3, 2, AFFINE, torch.tensor(off, device=d), torch.tensor(div, device=d),
                                    with_lr=False)
    else:
        hr, _, oo, do = prep_norm_abi(rd, 3, 2, LSCALE, with_lr=False)
        off, div = oo.cpu().numpy(), do.cpu().numpy()
        assert np.array_equal(off[:, 0], raw.min(axis=(1, 2, 3)))
    assert_ulps(hr.cpu().numpy(), closure(raw, off, div, 3), 2, what=f"hr B={B} mode={mode}")


@pytest.mark.parametrize("musd", MUSD, ids=lambda m: f"mu{m[0]:g}")
@pytest.mark.parametrize("T,scale,B,C", [(6, 2, 3, 2), (48, 4, 3, 2), (192, 4, 2, 2), (256, 4, 2, 1)])
def test_lscale(T, scale, B, C, musd):
    d = dev()
    mu, sd = musd
    raw = field((B, C, T, T), mu, sd, 11 * T)
    rd = torch.tensor(raw, device=d)
    mn, mx = raw.min(axis=(2, 3)), raw.max(axis=(2, 3))
    for f in (0, 5):
        hr, lr, oo, do = prep_norm_abi(rd, f, scale, LSCALE)
        off, div = oo.cpu().numpy(), do.cpu().numpy()
        assert np.array_equal(off, mn) and np.array_equal(div, mx - mn)  # fp32 max - min
        h = hr.cpu().numpy()
        assert_ulps(h, closure(raw, off, div, f), 2, what=f"lscale hr T={T} flip={f}")
        assert np.all(h.min(axis=(2, 3)) == 0.0) and np.all(h.max(axis=(2, 3)) == 1.0)
        check_lr(hr, lr, scale)


def test_lnorm_forwards_to_batch_prep():
    d = dev()
    for T, scale, f in ((48, 4, 6), (10, 2, 3), (256, 8, 1)):
        raw = torch.tensor(field((3, 2, T, T), 290.0, 0.7, T), device=d)
        hr, lr, mean, std = prep_norm_abi(raw, f, scale, LNORM)
        ref = prep_batch(raw, f, scale)
        torch.cuda.synchronize()
        assert torch.equal(hr, ref["hr"]) and torch.equal(lr, ref["lr"])
        assert torch.equal(mean, ref["mean"][:, :, 0, 0]) and torch.equal(std, ref["std"][:, :, 0, 0])


def test_batch_prep_norm_rejects_bad_args():
    d = dev()
    raw = torch.zeros(1, 1, 8, 8, device=d)
    hr = torch.empty_like(raw)
    st = torch.ones(1, 1, device=d)
    bad = [(1, 1, 8, 0, 2, 3, ptr(st), ptr(st)),        # unknown mode
           (1, 1, 8, 0, 2, AFFINE, None, ptr(st)),      # AFFINE without off
           (1, 1, 8, 8, 2, LSCALE, None, None),         # flip index
           (1, 1, 7, 0, 2, LSCALE, None, None),         # odd T
           (65536, 1, 8, 0, 2, LNORM, None, None)]      # LNORM keeps batch_prep's limit
    for B, C, T, f, s, mode, off, div in bad:
        with pytest.raises(_lib.SrmiError):
            call("srmi_batch_prep_norm", ptr(raw), B, C, T, f, s, mode, off, div, ptr(hr), None, None, None, S())
    # raw / hr off a 16-byte boundary are refused before the launch (float4 accesses)
    big = torch.zeros(2, 1, 8, 8, device=d)
    for r, h in ((ptr(big) + 4, ptr(hr)), (ptr(raw), ptr(big) + 8)):
        with pytest.raises(_lib.SrmiError):
            call("srmi_batch_prep_norm", r, 1, 1, 8, 0, 2, LSCALE, None, None, h, None, None, None, S())


# --------------------------------------------------------------- region tiling
# (C, H, W, tile): the register-resident float4 form; W % 4 != 0 -> the scalar form
@pytest.mark.parametrize("C,H,W,T", [(2, 96 + 5, 144 + 4, 48), (2, 23, 31, 10)])
def test_region_to_tiles_norm(C, H, W, T):
    d = dev()
    mu, sd = MUSD[2]
    region = field((C, H, W), mu, sd, H)
    gy, gx = H // T, W // T
    n = gy * gx
    rg = torch.tensor(region, device=d)
    # the raw tiles, tile t = grid cell t, channel c = region channel c
    raw = region[:, :gy * T, :gx * T].reshape(C, gy, T, gx, T).transpose(1, 3, 0, 2, 4).reshape(n, C, T, T)
    rawd = torch.tensor(np.ascontiguousarray(raw), device=d)

    def r2t(mode, off=None, div=None):
        tiles = torch.empty(n, C, T, T, device=d)
        oo, do = torch.full((n, C), -7.0, device=d), torch.full((n, C), -7.0, device=d)
        bad = torch.full((n,), 9, dtype=torch.int32, device=d)
        call("srmi_region_to_tiles_norm", ptr(rg), C, H, W, T, T, mode, ptr(off), ptr(div), ptr(tiles), ptr(oo),
             ptr(do), ptr(bad), S())
        return tiles, oo, do, bad
    # LNORM is srmi_region_to_tiles
    tiles, mean, std, bad = r2t(LNORM)
    t0, m0, s0 = torch.empty_like(tiles), torch.empty_like(mean), torch.empty_like(std)
    b0 = torch.empty_like(bad)
    call("srmi_region_to_tiles", ptr(rg), C, H, W, T, T, ptr(t0), ptr(m0), ptr(s0), ptr(b0), S())
    torch.cuda.synchronize()
    assert torch.equal(tiles, t0) and torch.equal(mean, m0) and torch.equal(std, s0) and torch.equal(bad, b0)
    assert int(bad.sum()) == 0
    # LSCALE and AFFINE are batch_prep_norm (flip 0) of the same tiles, bit for bit
    tiles, oo, do, bad = r2t(LSCALE)
    hr, _, po, pd = prep_norm_abi(rawd, 0, 2, LSCALE, with_lr=False)
    assert torch.equal(tiles, hr) and torch.equal(oo, po) and torch.equal(do, pd) and int(bad.sum()) == 0
    assert np.array_equal(oo.cpu().numpy(), raw.min(axis=(2, 3)))
    off, div = affine_stats(n, C, mu, sd, 3)
    od, dd = torch.tensor(off, device=d), torch.tensor(div, device=d)
    tiles, oo, do, bad = r2t(AFFINE, od, dd)
    hr, _, _, _ = prep_norm_abi(rawd, 0, 2, AFFINE, od, dd, with_lr=False)
    assert torch.equal(tiles, hr) and int(bad.sum()) == 0 and float(oo.max()) == -7.0
    assert_ulps(tiles.cpu().numpy(), closure(raw, off, div, 0), 2, what="region AFFINE tiles")
    # srmi_tiles_to_region undoes both
    out = torch.empty(C, gy * T, gx * T, device=d)
    call("srmi_tiles_to_region", ptr(tiles), ptr(od), ptr(dd), None, C, T, T, gy, gx, ptr(out), S())
    crop = region[:, :gy * T, :gx * T].astype(np.float64)
    scale_at = np.maximum(np.abs(crop), 8 * sd + abs(mu))
    assert_ulps(out.cpu().numpy(), crop, 2, at=scale_at, what="AFFINE round trip")
    # a NaN marks its tile
    region2 = region.copy()
    region2[1, T + 1, 2] = np.nan
    rg.copy_(torch.tensor(region2))
    _, _, _, bad = r2t(LSCALE)
    assert bad.cpu().tolist() == [int(t == gx) for t in range(n)]


# ------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def dataset():
    """3 time slices of a (2, 96, 144) region tiled at 48 (srmi.llc.get_tiles) and
    their statistics."""
    from srmi.llc import get_tiles
    d = dev()
    mu, sd = MUSD[0]
    regions = [field((2, 96, 144), mu, sd, 300 + i) + np.float32(0.5 * i) for i in range(3)]
    slices = [get_tiles(torch.tensor(r, device=d), 48, 48)[0] for r in regions]
    stats = NormStats.compute([slices[0], (lambda: slices[1]), slices[2]])
    torch.cuda.synchronize()
    return slices, stats, sd


def test_normstats_compute(dataset):
    slices, stats, sd = dataset
    assert stats.ntimes == 3 and tuple(stats.tiles.shape) == (6, 2, 4) and tuple(stats.globals.shape) == (2, 4)
    check_stats(stats.tiles, stats.globals, [s.cpu().numpy() for s in slices], sd)


@pytest.mark.parametrize("norm", NORM_TYPES)
def test_prep_batch_every_norm(dataset, norm):
    """prep_batch on batches of 4 tiles (tile ranges (0, 4) and (4, 6)) against the
    oracle's norm().  The dataset modes are held to the oracle fed the device's own
    fp32 statistics (those are held to the fp64 oracle in test_normstats_compute):
    off is then the same number on both sides, div = sqrt(var) differs by fp32
    rounding of the sqrt (relative 2^-24), so every element is within 4 fp32 ulps of
    itself (2 of the closure + 1 of div + 1 of the final rounding).  lnorm: the
    1e-6 absolute of tests/test_gpu_batch.py; lscale: 2 ulps as in test_lscale."""
    slices, stats, _ = dataset
    raw = slices[1]
    x = raw.cpu().numpy().astype(np.float64)
    t = stats.tiles.cpu().numpy().astype(np.float64)
    if norm[0] == "g":  # globalize_norm of equal rows is that row: the device's globals
        t = np.broadcast_to(stats.globals.cpu().numpy().astype(np.float64)[None], t.shape)
    whole = normalize_tiles(raw, norm, stats)
    for tr in ((0, 4), (4, 6)):
        out = prep_batch(raw[tr[0]:tr[1]].contiguous(), 5, 4, norm=norm, stats=stats, tile_range=tr)
        torch.cuda.synchronize()
        ref, attrs = no.norm(x[tr[0]:tr[1]], norm, tr, t)
        ref = ro.xyflip(ref, 5)
        assert set(out) - {"hr", "lr", "xyflip"} == set(ATTR_KEYS[norm]) == set(attrs)
        hr = out["hr"].cpu().numpy()
        if norm == "lnorm":
            np.testing.assert_allclose(hr, ref, atol=1e-6, rtol=0)
        else:
            assert_ulps(hr, ref, 2 if norm == "lscale" else 4, what=f"{norm} hr {tr}")
        check_lr(out["hr"], out["lr"], 4)
        for k, v in attrs.items():
            got = out[k].cpu().numpy()
            assert got.shape == v.shape
            if norm == "lnorm":
                np.testing.assert_allclose(got, v, rtol=1e-6)
            elif k == "std":  # the fp32 sqrt of the fp32 variance: one ulp of the fp64 sqrt
                np.testing.assert_allclose(got, v, rtol=2.0 ** -23, atol=0)
            else:  # stored statistics and the tile's own max / min: exact
                assert np.array_equal(got, v.astype(np.float32)), k
        # slice-wise normalisation is the batch-wise one, bit for bit
        plain = prep_batch(raw[tr[0]:tr[1]].contiguous(), 0, 4, with_lr=False, norm=norm, stats=stats, tile_range=tr)
        assert torch.equal(plain["hr"], whole[tr[0]:tr[1]])


@pytest.mark.parametrize("on_device", [False, True], ids=["load_host", "load_device"])
def test_prep_batch_with_loaded_stats(dataset, tmp_path, on_device):
    """save -> load -> prep_batch / normalize_tiles.  NormStats.load without device=
    leaves the statistics on the host; the kernel must still be handed device
    pointers.  The file holds the fp32 tile rows themselves, so tnorm and tscale are
    bit for bit what the computed statistics give, attrs included, and the attrs are
    on the batch's device.  The global rows of a loaded file are globalize_norm of the
    stored fp32 rows (as the reference derives them from the file), so gnorm and
    gscale are compared between the two ways of loading, and gnorm against the
    closure on the loaded globals."""
    slices, stats, _ = dataset
    raw = slices[1]
    path = stats.save(str(tmp_path / "norms.nc"), ["a", "b"])
    loaded = NormStats.load(path, device=dev() if on_device else None)
    assert loaded.tiles.is_cuda == on_device
    assert torch.equal(loaded.tiles.cpu(), stats.tiles.cpu())
    tr = (2, 6)
    batch = raw[tr[0]:tr[1]].contiguous()
    for norm in ("tnorm", "tscale"):
        want = prep_batch(batch, 3, 4, norm=norm, stats=stats, tile_range=tr)
        got = prep_batch(batch, 3, 4, norm=norm, stats=loaded, tile_range=tr)
        torch.cuda.synchronize()
        assert set(got) == set(want)
        for k in ("hr", "lr") + ATTR_KEYS[norm]:
            assert got[k].device == raw.device, k
            assert torch.equal(got[k], want[k]), f"{norm} {k}"
        assert torch.equal(normalize_tiles(raw, norm, loaded), normalize_tiles(raw, norm, stats))
    other = NormStats.load(path, device=None if on_device else dev())
    for norm in ("gnorm", "gscale"):
        got = prep_batch(batch, 0, 4, norm=norm, stats=loaded, tile_range=tr)
        ref = prep_batch(batch, 0, 4, norm=norm, stats=other, tile_range=tr)
        torch.cuda.synchronize()
        assert torch.equal(got["hr"], ref["hr"]) and torch.equal(got["lr"], ref["lr"]), norm
    g = loaded.globals.cpu().numpy().astype(np.float64)  # [C, 4]
    x = batch.cpu().numpy().astype(np.float64)
    gd = torch.sqrt(loaded.globals.cpu()[:, 1]).numpy().astype(np.float64)  # the fp32 sqrt prep_batch takes
    want = ((x - g[None, :, 0, None, None]) / gd[None, :, None, None]).astype(np.float32).astype(np.float64)
    got = prep_batch(batch, 0, 4, norm="gnorm", stats=loaded, tile_range=tr)["hr"]
    assert_ulps(got.cpu().numpy(), want, 2, what="gnorm from a loaded file")


# ------------------------------------------------------------------- inference
def _rcan_1x1_x2():
    spec = NetSpec(arch="rcan", nchannels_in=1, nchannels_out=1, nfeatures=64, nlayers=1, nblocks=1, cbottleneck=2,
                   scale=2)
    table = param_table(spec)
    flat = torch.empty(sum(t[2] for t in table))
    from srmi.trainer import default_init_
    default_init_(flat, table, seed=5)
    return spec, flat


@pytest.mark.parametrize("musd", MUSD, ids=lambda m: f"mu{m[0]:g}")
@pytest.mark.parametrize("norm", ["tnorm", "lscale", "gnorm"])
def test_tiled_inference_norms(norm, musd):
    """A (1, 96, 96) region as a 6 x 1 grid of 16 x 96 tiles (x2 model: 8 x 48 LR
    tiles, the smallest the engine takes).  The mosaics go through
    srmi_tiles_to_region's fp32 z * div + off, z the normalised tile: its error is
    2 * 2^-24 |x - off| (the roundings of z and of div) plus half an ulp of x, so the
    target mosaic is held to 2 ulps at max(|x|, |x - off|); for these fields
    |x - off| < |x| except for (-3, 2), whose values pass through 0."""
    from srmi.inference import TiledInference
    from srmi.llc import get_tiles
    d = dev()
    mu, sd = musd
    spec, flat = _rcan_1x1_x2()
    regions = [field((1, 96, 96), mu, sd, 500 + i) for i in range(3)]
    rd = [torch.tensor(r, device=d) for r in regions]
    tiled = [get_tiles(r, 16, 96) for r in rd]
    stats = NormStats.compute([t[0] for t in tiled])
    ids = tiled[0][1]
    inv = np.full(6, -1)
    inv[ids] = np.arange(len(ids))
    gstats = stats.for_grid(inv)
    task = {"norm": norm}
    out = {}
    for graph in (True, False):
        ti = TiledInference(spec, flat.to(d), (1, 96, 96), (16, 96), device=d, graph=graph, batch_size=4, task=task,
                            stats=gstats if norm != "lscale" else None)
        assert ti.norm == norm
        res = []
        for r in rd[:2]:  # the second region replays the captured graph
            images, losses = ti.process_region(r)
            torch.cuda.synchronize()
            res.append(({k: v.clone() for k, v in images.items()}, {k: v.clone() for k, v in losses.items()}))
        out[graph] = res
    for (ig, lg), (ie, le) in zip(out[True], out[False]):
        for k in ig:
            assert torch.equal(ig[k], ie[k]), f"graph replay != eager: {k}"
        for k in lg:
            assert torch.equal(lg[k], le[k])
    for r, (images, _) in zip(regions[:2], out[True]):
        x = r.astype(np.float64)
        target = images["target"].cpu().numpy()
        if norm == "gnorm":  # left normalised, as the reference leaves it: the AFFINE closure
            go, gd = (float(v[0, 0]) for v in stats.offsets("gnorm", (0, 1)))
            assert go == float(stats.globals[0, 0]) and abs(gd - np.sqrt(float(stats.globals[0, 1]))) <= 2.0 ** -23 * gd
            assert_ulps(target, ((x - go) / gd).astype(np.float32).astype(np.float64), 2, what="gnorm field")
        else:
            if norm == "tnorm":
                off = stats.tiles.cpu().numpy()[:, 0, 0].astype(np.float64)
            else:
                off = r.reshape(6, -1).min(axis=1).astype(np.float64)
            xo = np.abs(x.reshape(6, 16, 96) - off[:, None, None]).reshape(1, 96, 96)
            assert_ulps(target, x, 2, at=np.maximum(np.abs(x), xo), what=f"{norm} target mosaic")


def test_tiled_inference_dataset_norm_needs_stats():
    from srmi.inference import TiledInference
    d = dev()
    spec, flat = _rcan_1x1_x2()
    with pytest.raises(ValueError, match="stats"):
        TiledInference(spec, flat.to(d), (1, 96, 96), (16, 96), device=d, norm="tscale")
    with pytest.raises(Exception, match="Unknown norm"):
        TiledInference(spec, flat.to(d), (1, 96, 96), (16, 96), device=d, task={"norm": "znorm"})
