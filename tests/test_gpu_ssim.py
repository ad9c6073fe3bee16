"""The SSIM / PSNR score on the HIP path: srmi_ssim / srmi.ssim.SSIMScore against the numpy
oracle (tests/ssim_oracle.py), and RegionSuperResolver.score_ssim end to end.

Bars.  The device works in fp32, so it is held to the error of the SAME arithmetic done in
numpy: e32 is the largest per-pixel difference between the oracle in fp32 and the oracle in
fp64 on the very case under test.  The device's map, and each of its means, may be 10 x e32
off the fp64 oracle: a different summation order and FMA contraction, no floor.  mse is held
to 1e-6 relative (its differences and squares are fp64 on the device).  Counts, the range
and the map's NaN pattern are exact.  Every test prints e32, the device's error and their
ratio before it asserts.

Measured on an MI355X: on the six white shapes e32 is 8.8e-8 (the single window of 11 x 11)
and 3.5e-7 .. 5.4e-7, the device's map 0.86 .. 1.15 e32 off (3.07 e32 on the single window)
and its means 0.05 .. 0.31 e32 (3.07); the low-contrast field e32 4.0e-7, map 0.86 e32, means
0.05; the coast e32 4.5e-7, map 1.07, means 0.09; data_range 20: e32 3.4e-7, map 1.00, means
0.31.  mse is 1.4e-8 .. 3.9e-8 off in relative terms (its rounding to fp32), and ssim(a, a)
is 6.0e-8 from 1.

The shapes are the smallest at which the kernel can go wrong; TILE_H x TILE_W is the
rectangle of output pixels one workgroup owns (DESIGN.md "SSIM score"), and the last shape
exceeds it by one pixel on each axis."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ssim_oracle as so  # noqa: E402
from srmi import _lib  # noqa: E402
from srmi._lib import ptr  # noqa: E402
from srmi.ssim import SSIMScore, ssim_workspace  # noqa: E402
from srmi.superres import RegionSuperResolver  # noqa: E402
from test_gpu_inference import _small_rcan  # noqa: E402

TILE_H, TILE_W = 24, 64  # kTileH, kTileW of csrc/ssim.hip
SHAPES = [(1, 11, 11), (2, 12, 27), (1, 37, 70), (2, 96, 80), (1, 75, 150), (1, TILE_H + 1, TILE_W + 1)]
TILE = (16, 32)  # the smallest 16-row tile the inference engine takes
SCALARS = ("ssim", "cs", "mse", "data_range", "psnr")


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


@functools.lru_cache(maxsize=None)
def white(shape, seed=0, std=1.5, noise=0.3):
    """truth = 290 + std N(0, 1) (the offset is what the pivot is for), pred = truth + noise N(0, 1)."""
    rng = np.random.default_rng(200 + seed)
    truth = (290.0 + std * rng.standard_normal(shape)).astype(np.float32)
    pred = (truth + noise * rng.standard_normal(shape)).astype(np.float32)
    truth.setflags(write=False)
    pred.setflags(write=False)
    return pred, truth


def oracles(pred, truth, data_range=None):
    """(the fp64 oracle, e32 of the map, e32 of each mean) on this very case."""
    o64 = so.ssim(pred, truth, data_range)
    o32 = so.ssim(pred, truth, data_range, dtype=np.float32)
    assert np.array_equal(np.isnan(o32["map"]), np.isnan(o64["map"]))
    d = np.abs(o32["map"].astype(np.float64) - o64["map"])
    e32 = float(np.nanmax(d)) if np.isfinite(d).any() else 0.0
    return o64, e32


@functools.lru_cache(maxsize=None)
def white_oracles(shape):
    return oracles(*white(shape))


def measure(pred, truth, data_range=None, want_map=True):
    """numpy fields -> (the measure dict as numpy arrays, the SSIMScore)."""
    d = dev()
    sc = SSIMScore(pred.shape, data_range, want_map, device=d)
    m = sc.measure(torch.tensor(pred, device=d), torch.tensor(truth, device=d))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in m.items()}, sc


def check_against(tag, m, o64, e32):
    """The bar of the module docstring; prints before it asserts."""
    fin = np.isfinite(o64["map"])
    emap = float(np.abs(m["map"].astype(np.float64) - o64["map"])[fin].max()) if fin.any() else 0.0
    used = o64["nwin"] > 0
    emean = max(float(np.abs(m[k].astype(np.float64) - o64[k])[used].max()) if used.any() else 0.0
                for k in ("ssim", "cs"))
    wet = o64["npix"] > 0
    emse = float((np.abs(m["mse"].astype(np.float64) - o64["mse"]) / o64["mse"])[wet].max()) if wet.any() else 0.0
    print(f"{tag}: e32 {e32:.3e}, device map {emap:.3e} (ratio {emap / e32 if e32 else 0:.2f}), means {emean:.3e} "
          f"(ratio {emean / e32 if e32 else 0:.2f}), mse rel {emse:.2e}")
    assert np.array_equal(m["nwin"], o64["nwin"]) and np.array_equal(m["npix"], o64["npix"])
    assert np.array_equal(np.isnan(m["map"]), ~fin)
    assert emap <= 10.0 * e32 and emean <= 10.0 * e32
    assert emse <= 1e-6
    assert np.array_equal(np.isnan(m["ssim"]), ~used) and np.array_equal(np.isnan(m["mse"]), ~wet)


# ---------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_white_fields_match_the_oracle(shape):
    pred, truth = white(shape)
    o64, e32 = white_oracles(shape)
    m, sc = measure(pred, truth)
    Cn, H, W = shape
    check_against(f"white {shape}", m, o64, e32)
    assert (m["nwin"] == (H - 10) * (W - 10)).all() and (m["npix"] == H * W).all()
    # the range: max - min of the truth, one fp32 subtraction, bit for bit
    want = truth.reshape(Cn, -1).max(1) - truth.reshape(Cn, -1).min(1)
    assert want.dtype == np.float32 and np.array_equal(m["data_range"].view(np.int32), want.view(np.int32))
    # the dict: views of out / count, psnr the device's own fp32 operations
    out, count = sc.out.cpu().numpy(), sc.count.cpu().numpy()
    for i, k in enumerate(("ssim", "cs", "mse", "data_range")):
        assert np.array_equal(m[k], out[:, i])
    assert np.array_equal(m["nwin"], count[:, 0]) and np.array_equal(m["npix"], count[:, 1])
    assert np.allclose(m["psnr"], 10 * np.log10(out[:, 3].astype(np.float64) ** 2 / out[:, 2]), rtol=1e-5, atol=0)
    assert np.allclose(m["psnr"], o64["psnr"], rtol=1e-5, atol=0)
    # the border of the map is the canonical NaN
    assert (m["map"][:, :5].view(np.uint32) == 0x7fc00000).all()
    assert (m["map"][:, :, -5:].view(np.uint32) == 0x7fc00000).all()


def test_low_contrast_field_needs_the_pivot():
    """290 + 0.01 N: without the pivot E[x^2] - mu^2 in fp32 (eps 290^2 = 5e-3) loses a
    variance of 1e-4 altogether."""
    shape = SHAPES[2]
    pred, truth = white(shape, seed=1, std=0.01, noise=0.003)
    o64, e32 = oracles(pred, truth)
    m, _ = measure(pred, truth)
    assert e32 < 1e-4 and 0.5 < o64["ssim"][0] < 0.999
    check_against("low contrast", m, o64, e32)


# --------------------------------------------------------------------------- 2. mask
def test_one_nan_removes_exactly_its_121_positions():
    shape = SHAPES[3]
    pred, truth = white(shape)
    base, _ = measure(pred, truth)
    p2 = pred.copy()
    p2[1, 40, 61] = np.nan  # at least 10 from every edge; its windows straddle two rectangles in x
    o64, e32 = oracles(p2, truth)
    m, _ = measure(p2, truth)
    check_against("one NaN in a", m, o64, e32)
    assert m["nwin"][1] == base["nwin"][1] - 121 and m["npix"][1] == base["npix"][1] - 1
    assert m["nwin"][0] == base["nwin"][0] and m["npix"][0] == base["npix"][0]
    gone = np.isnan(m["map"][1]) & ~np.isnan(base["map"][1])
    want = np.zeros_like(gone)
    want[35:46, 56:67] = True
    assert np.array_equal(gone, want)
    # the truth is untouched, so r and L are: every other position keeps its bits
    keep = ~np.isnan(m["map"])
    assert np.array_equal(m["map"][keep].view(np.int32), base["map"][keep].view(np.int32))
    t2 = truth.copy()
    t2[1, 40, 61] = np.inf  # in the truth only: the same counts, the oracle's
    o64b, e32b = oracles(pred, t2)
    mb, _ = measure(pred, t2)
    check_against("one Inf in b", mb, o64b, e32b)
    assert np.array_equal(mb["nwin"], m["nwin"]) and np.array_equal(mb["npix"], m["npix"])


def test_coast_in_both_fields():
    shape = SHAPES[4]
    pred, truth = (v.copy() for v in white(shape))
    yy, xx = np.mgrid[:shape[1], :shape[2]]
    land = (yy - 80.0) ** 2 + (xx - 160.0) ** 2 < 70.0 ** 2  # the lower right corner, a round coast
    pred[0][land] = np.nan
    truth[0][land] = np.nan
    o64, e32 = oracles(pred, truth)
    share = o64["nwin"][0] / ((shape[1] - 10) * (shape[2] - 10))
    print(f"coast: {land.mean():.2f} of the pixels dry, {share:.2f} of the positions used")
    assert 0.25 <= share < 0.9
    m, _ = measure(pred, truth)
    check_against("coast", m, o64, e32)


def test_a_channel_without_a_finite_pixel():
    shape = SHAPES[1]
    pred, truth = white(shape)
    base, _ = measure(pred, truth)
    for where in ("a", "b", "both"):
        p2, t2 = pred.copy(), truth.copy()
        if where in ("a", "both"):
            p2[0] = np.nan
        if where in ("b", "both"):
            t2[0] = np.nan
        m, _ = measure(p2, t2)
        assert m["nwin"][0] == 0 and m["npix"][0] == 0
        assert np.isnan(m["ssim"][0]) and np.isnan(m["cs"][0]) and np.isnan(m["mse"][0]) and np.isnan(m["psnr"][0])
        assert np.isnan(m["map"][0]).all()
        for k in SCALARS + ("nwin", "npix", "map"):
            assert np.array_equal(m[k][1], base[k][1], equal_nan=True), (where, k)


# ---------------------------------------------------------------- 3. map against means
def test_the_means_are_the_maps_and_do_not_need_it():
    shape = SHAPES[4]
    pred, truth = white(shape)
    m, sc = measure(pred, truth)
    fin = np.isfinite(m["map"][0])
    assert int(fin.sum()) == int(m["nwin"][0])
    assert abs(m["map"][0][fin].astype(np.float64).mean() - float(m["ssim"][0])) <= 1e-6
    m0, sc0 = measure(pred, truth, want_map=False)
    assert "map" not in m0 and sc0.map is None
    assert torch.equal(bits(sc0.out), bits(sc.out)) and torch.equal(sc0.count, sc.count)


# --------------------------------------------------------------- 4. other properties
def test_a_field_against_itself():
    shape = SHAPES[3]
    _, truth = white(shape)
    m, _ = measure(truth, truth)
    print(f"ssim(a, a) - 1: {np.abs(m['ssim'].astype(np.float64) - 1).max():.2e}")
    assert np.abs(m["ssim"].astype(np.float64) - 1.0).max() <= 1e-6
    assert np.abs(m["cs"].astype(np.float64) - 1.0).max() <= 1e-6
    assert (m["mse"] == 0).all() and np.isposinf(m["psnr"]).all()


def test_data_range_override():
    shape = SHAPES[1]
    pred, truth = white(shape)
    o64, e32 = oracles(pred, truth, 20.0)
    m, _ = measure(pred, truth, 20.0)
    assert (m["data_range"] == np.float32(20.0)).all() and (o64["data_range"] == 20.0).all()
    check_against("data_range 20", m, o64, e32)
    own, _ = measure(pred, truth)
    assert (m["ssim"] > own["ssim"]).all()  # larger C1, C2: closer to 1
    neg, _ = measure(pred, truth, -1.0)  # <= 0: from the truth
    for k in SCALARS + ("map",):
        assert np.array_equal(neg[k], own[k], equal_nan=True)


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[4]], ids=["small", "several-rectangles"])
def test_bit_identical_runs_and_no_dependence_on_the_workspace(shape):
    d = dev()
    pred, truth = (torch.tensor(v, device=d) for v in white(shape))
    sc = SSIMScore(shape, want_map=True, device=d)
    sc.measure(pred, truth)
    first = (sc.out.clone(), sc.count.clone(), sc.map.clone())
    sc.measure(pred, truth)
    assert torch.equal(bits(sc.out), bits(first[0])) and torch.equal(bits(sc.map), bits(first[2]))
    sc.workspace.fill_(0xFF)
    sc.out.fill_(-7.0)
    sc.count.fill_(-3)
    sc.map.fill_(-7.0)
    sc.measure(pred, truth)
    assert torch.equal(bits(sc.out), bits(first[0])) and torch.equal(sc.count, first[1])
    assert torch.equal(bits(sc.map), bits(first[2]))


def test_measure_is_capturable_on_one_stream():
    d = dev()
    shape = SHAPES[3]
    pred, truth = (torch.tensor(v, device=d) for v in white(shape))
    eager = SSIMScore(shape, want_map=True, device=d)
    me = {k: v.clone() for k, v in eager.measure(pred, truth).items()}
    sc = SSIMScore(shape, want_map=True, device=d)
    sc.measure(pred, truth)  # warm-up outside capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(device=d)
    s.wait_stream(torch.cuda.current_stream(d))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            m = sc.measure(pred, truth)
    torch.cuda.current_stream(d).wait_stream(s)
    for _ in range(2):
        sc.out.fill_(-7.0)
        sc.count.fill_(-3)
        sc.map.fill_(-7.0)
        sc.psnr.fill_(-7.0)
        g.replay()
        torch.cuda.synchronize()
        for k in me:
            assert torch.equal(bits(m[k]), bits(me[k])), k


# --------------------------------------------------------------------- 5. refusals
@pytest.mark.parametrize("case", ["H10", "nan-range", "inf-range", "short-workspace", "null-out", "null-count", "C0"])
def test_refusals_leave_the_outputs_untouched(case):
    d = dev()
    lib = _lib.load()
    Cn, H, W = (0 if case == "C0" else 1), (10 if case == "H10" else 16), 16
    a = torch.zeros((1, 16, 16), device=d)
    nbytes = ssim_workspace(1, 16, 16)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=d)
    out = torch.full((1, 4), -7.0, device=d)
    count = torch.full((1, 2), -3, dtype=torch.int64, device=d)
    smap = torch.full((1, 16, 16), -7.0, device=d)
    dr = {"nan-range": float("nan"), "inf-range": float("inf")}.get(case, 0.0)
    rc = lib.srmi_ssim(ptr(a), ptr(a), Cn, H, W, dr, ptr(ws), nbytes - (case == "short-workspace"),
                       None if case == "null-out" else ptr(out), None if case == "null-count" else ptr(count),
                       ptr(smap), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == _lib.SRMI_ERR_ARG
    assert (out == -7.0).all() and (count == -3).all() and (smap == -7.0).all() and (ws == 0).all()
    if case in ("H10", "C0"):
        n = C.c_size_t(5)
        assert lib.srmi_ssim_workspace(Cn, H, W, C.byref(n)) == _lib.SRMI_ERR_ARG and n.value == 5
        with pytest.raises(ValueError):
            SSIMScore((Cn, H, W), device=d)
    if case in ("nan-range", "inf-range"):
        with pytest.raises(ValueError):
            SSIMScore((1, 16, 16), dr, device=d)


def test_measure_refuses_wrong_inputs():
    d = dev()
    sc = SSIMScore((1, 16, 20), device=d)
    ok = torch.zeros((1, 16, 20), device=d)
    for bad in (torch.zeros((1, 20, 16), device=d), ok.double(), ok.cpu(), torch.zeros((1, 20, 16), device=d).mT):
        with pytest.raises(ValueError):
            sc.measure(bad, ok)
        with pytest.raises(ValueError):
            sc.measure(ok, bad)


# -------------------------------------------------------------------- 6. end to end
def _field(rng, C_, h, w):
    base = rng.randn(C_, h, w)
    return (base + np.roll(base, 1, 1) + np.roll(base, 1, 2)).astype(np.float32)


def test_score_ssim_is_score_plus_the_measure_of_its_images():
    d = dev()
    spec, model, flat = _small_rcan()
    rng = np.random.RandomState(61)
    hr = torch.tensor(_field(rng, 1, 160, 224) * 2 + 5, device=d)
    kw = dict(tile_lr=TILE, overlap=(4, 4), device=d)
    rs = RegionSuperResolver(spec, flat.to(d), (1, 40, 56), **kw)
    plain = RegionSuperResolver(spec, flat.to(d), (1, 40, 56), **kw)
    images, losses, ssim = rs.score_ssim(hr, maps=True)
    images0, losses0 = plain.score(hr)
    assert set(ssim) == {"model", "interpolated"}
    for k in ("input", "interpolated", "model"):
        assert torch.equal(bits(images[k]), bits(images0[k]))
    for k in ("model", "interpolated"):
        assert torch.equal(bits(losses[k]), bits(losses0[k]))
    for k in ("model", "interpolated"):
        m = SSIMScore((1, 160, 224), want_map=True, device=d).measure(images[k], hr)
        assert set(m) == set(ssim[k]) and "map" in m
        for q in m:
            assert torch.equal(bits(m[q]), bits(ssim[k][q])), (k, q)
        assert int(ssim[k]["nwin"].item()) == 150 * 214 and torch.isfinite(ssim[k]["ssim"]).all()
        # mse is score's RMSE squared (score sums in fp32, in another order: 1e-4)
        assert abs(float(ssim[k]["mse"]) - float(losses[k]) ** 2) <= 1e-4 * float(ssim[k]["mse"])
    # a second call reuses the buffers and gives the same bits; another key gets its own
    keep = {k: ssim[k]["map"].clone() for k in ssim}
    _, _, again = rs.score_ssim(hr, maps=True)
    for k in keep:
        assert again[k]["map"].data_ptr() == ssim[k]["map"].data_ptr()
        assert torch.equal(bits(again[k]["map"]), bits(keep[k]))
    _, _, fixed = rs.score_ssim(hr, data_range=50.0)
    assert "map" not in fixed["model"] and float(fixed["model"]["data_range"]) == 50.0


def test_score_ssim_with_land_masks_the_coast():
    d = dev()
    spec, model, flat = _small_rcan()
    rng = np.random.RandomState(62)
    hr = _field(rng, 1, 160, 224) * 2 + 5
    hr[0, 40:72, 100:140] = np.nan  # land on whole LR pixels
    rs = RegionSuperResolver(spec, flat.to(d), (1, 40, 56), tile_lr=TILE, overlap=(4, 4), land=True, device=d)
    plain = RegionSuperResolver(spec, flat.to(d), (1, 40, 56), tile_lr=TILE, overlap=(4, 4), land=True, device=d)
    hrd = torch.tensor(hr, device=d)
    images, losses, ssim = rs.score_ssim(hrd, maps=True)
    images0, losses0 = plain.score(hrd)
    for k in ("interpolated", "model"):
        assert torch.equal(bits(images[k]), bits(images0[k])) and torch.equal(bits(losses[k]), bits(losses0[k]))
        m = SSIMScore((1, 160, 224), want_map=True, device=d).measure(images[k], hrd)
        for q in m:
            assert torch.equal(bits(m[q]), bits(ssim[k][q])), (k, q)
        o64 = so.ssim(images[k].cpu().numpy(), hr)
        n = int(o64["nwin"][0])
        print(f"{k}: {n} of {150 * 214} positions used")
        assert 0 < n < 150 * 214 and int(ssim[k]["nwin"].item()) == n
        assert int(ssim[k]["npix"].item()) == int(o64["npix"][0])
        assert np.array_equal(np.isnan(ssim[k]["map"].cpu().numpy()), np.isnan(o64["map"]))
        assert torch.isfinite(ssim[k]["ssim"]).all()
