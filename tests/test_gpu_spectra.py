"""The spectral score on the HIP path: srmi_spectra / srmi.spectra.SpectralScore against the
numpy oracle (tests/spectra_oracle.py), and RegionSuperResolver.score_spectra end to end.

Bars.  The device transforms in fp32, so it is held to the error of the SAME arithmetic
done by a library: e32 is the largest error of the oracle run with complex64 transforms
(scipy.fft) against the fp64 oracle on the very case under test, relative to
(Eaa + Ebb) of the shell (white fields) or to the total over shells (the red field, whose
weakest shells lie below what fp32 resolves next to its peak).  The device may be 10 x e32
off: a different butterfly order and a different summation order, no floor.  Measured:
e32 4.6e-8 .. 1.7e-7 per shell on the six plans with the device at 0.5 .. 1.4 e32, and e32
2.0e-8 of the total for the red field with the device at 2.4 e32 (every test prints its
figures before it asserts)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import spectra_oracle as so  # noqa: E402
from srmi import _lib  # noqa: E402
from srmi._lib import ptr  # noqa: E402
from srmi.spectra import QUANTITIES, SpectralScore, spectra_workspace  # noqa: E402
from srmi.superres import RegionSuperResolver  # noqa: E402
from test_gpu_inference import _small_rcan  # noqa: E402

CASES = [(1, 16, 16, 16, 16), (2, 40, 56, 16, 12), (1, 48, 40, 32, 32), (2, 96, 80, 64, 32), (1, 160, 128, 128, 64),
         (1, 300, 272, 256, 128)]
NWIN = {CASES[0]: 1, CASES[1]: 15, CASES[2]: 4, CASES[3]: 4, CASES[4]: 2, CASES[5]: 4}
TILE = (16, 32)  # the smallest 16-row tile the inference engine takes


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def white(case, seed=0):
    """truth = 290 + 1.5 N(0, 1) (the offset exercises the fp64 mean), pred = truth + 0.3 N(0, 1)."""
    Cn, H, W, _, _ = case
    rng = np.random.default_rng(100 + seed)
    truth = (290.0 + 1.5 * rng.standard_normal((Cn, H, W))).astype(np.float32)
    pred = (truth + 0.3 * rng.standard_normal((Cn, H, W))).astype(np.float32)
    return pred, truth


@functools.lru_cache(maxsize=None)
def white_oracle(case):
    pred, truth = white(case)
    o64, n = so.spectra(pred, truth, case[3], case[4])
    o32, _ = so.spectra(pred, truth, case[3], case[4], dtype="complex64")
    return o64, o32, n


def measure(pred, truth, P, Q):
    """numpy fields -> (out [C, 4, K] fp32 numpy, nused, the measure dict, the SpectralScore)."""
    d = dev()
    sc = SpectralScore(pred.shape, P, Q, device=d)
    m = sc.measure(torch.tensor(pred, device=d), torch.tensor(truth, device=d))
    torch.cuda.synchronize()
    return sc.out.cpu().numpy(), int(sc.nused.item()), m, sc


# ---------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_white_fields_match_the_oracle(case):
    pred, truth = white(case)
    o64, o32, n64 = white_oracle(case)
    scale = (o64[:, 0] + o64[:, 1])[:, None, :]
    e32 = (np.abs(o32 - o64) / scale).max()
    out, nused, m, sc = measure(pred, truth, case[3], case[4])
    err = (np.abs(out.astype(np.float64) - o64) / scale).max()
    print(f"case {case}: e32 {e32:.3e}, device {err:.3e}, ratio {err / e32:.2f}")
    assert nused == n64 == NWIN[case]
    assert np.isfinite(out).all()
    assert (np.abs(out.astype(np.float64) - o64) <= 10.0 * e32 * scale).all()
    # the dict: views of out, the derived ratios as the device's own fp32 divisions
    for i, q in enumerate(QUANTITIES):
        assert np.array_equal(m[q].cpu().numpy(), out[:, i])
    assert np.array_equal(m["wavenumber"].cpu().numpy(), (np.arange(sc.K) / np.float32(case[3])).astype(np.float32))
    # three fp32 operations at most, none of them required to be correctly rounded: 1e-6
    assert np.allclose(m["error_ratio"].cpu().numpy(), out[:, 2] / out[:, 1], rtol=1e-6, atol=0)
    assert np.allclose(m["power_ratio"].cpu().numpy(), out[:, 0] / out[:, 1], rtol=1e-6, atol=0)
    assert np.allclose(m["coherence"].cpu().numpy(), out[:, 3] * out[:, 3] / out[:, 0] / out[:, 1], rtol=1e-6, atol=0)


# --------------------------------------------------------------------- 2. a red field
def test_red_field_matches_the_oracle_relative_to_the_total():
    """96 x 96, P 64, Q 32: amplitude slope k^-2.5, unit std, pred = truth + 0.01 noise.
    The per-shell relative error is recorded, not barred: fp32 cannot resolve a shell 1e-6
    below the peak."""
    rng = np.random.default_rng(9)
    truth = so.red_field(96, 2.5, 8).astype(np.float32)[None]
    pred = (truth + 0.01 * rng.standard_normal(truth.shape)).astype(np.float32)
    o64, _ = so.spectra(pred, truth, 64, 32)
    o32, _ = so.spectra(pred, truth, 64, 32, dtype="complex64")
    total = (o64[:, 0] + o64[:, 1]).sum()
    e32 = np.abs(o32 - o64).max() / total
    out, nused, _, _ = measure(pred, truth, 64, 32)
    err = np.abs(out.astype(np.float64) - o64).max() / total
    shell = (np.abs(out[:, :2].astype(np.float64) - o64[:, :2]) / o64[:, :2]).max()
    print(f"red field: dynamic range {o64[0, 1].max() / o64[0, 1].min():.3g}, e32 {e32:.3e} of the total, device "
          f"{err:.3e} (ratio {err / e32:.2f}); largest per-shell relative error of the two power spectra {shell:.3e}")
    assert nused == 4
    assert err <= 10.0 * e32


# --------------------------------------------------------------------- 3. skipping
def test_one_nan_skips_its_windows_for_all_channels():
    case = CASES[1]
    pred, truth = white(case)
    p2 = pred.copy()
    p2[1, 13, 38] = np.nan  # windows 2, 3, 7, 8 of the 3 x 5 plan
    o64, n64 = so.spectra(p2, truth, 16, 12)
    o32, _ = so.spectra(p2, truth, 16, 12, dtype="complex64")
    scale = (o64[:, 0] + o64[:, 1])[:, None, :]
    e32 = (np.abs(o32 - o64) / scale).max()
    out, nused, _, sc = measure(p2, truth, 16, 12)
    assert nused == n64 == 11
    skip = sc.workspace[:15 * 4].view(torch.int32).cpu().numpy()
    assert list(np.flatnonzero(skip)) == [2, 3, 7, 8] and set(skip) == {0, 1}
    assert (np.abs(out.astype(np.float64) - o64) <= 10.0 * e32 * scale).all()
    t2 = truth.copy()
    t2[0, 13, 38] = np.inf  # in the truth only, the other channel: the same windows, the same result
    out_t, nused_t, _, _ = measure(pred, t2, 16, 12)
    assert nused_t == 11 and np.array_equal(out_t, out)


def test_every_window_dry_gives_nan_and_no_fault():
    case = CASES[1]
    pred, truth = white(case)
    p3 = pred.copy()
    p3[0, ::8, ::8] = np.nan
    out, nused, m, _ = measure(p3, truth, 16, 12)
    assert nused == 0 and np.isnan(out).all()
    assert all(torch.isnan(m[q]).all() for q in ("error_ratio", "power_ratio", "coherence"))


# ------------------------------------------------------------------- 4. determinism
@pytest.mark.parametrize("case", [CASES[1], CASES[5]], ids=["P16", "P256"])
def test_bit_identical_runs_and_no_dependence_on_the_workspace(case):
    d = dev()
    pred, truth = (torch.tensor(v, device=d) for v in white(case))
    sc = SpectralScore(pred.shape, case[3], case[4], device=d)
    sc.measure(pred, truth)
    first = sc.out.clone()
    sc.measure(pred, truth)
    assert torch.equal(bits(sc.out), bits(first))
    sc.workspace.fill_(0xFF)
    sc.out.fill_(-7.0)
    sc.measure(pred, truth)
    assert torch.equal(bits(sc.out), bits(first)) and int(sc.nused.item()) == NWIN[case]


# ----------------------------------------------------------------------- 5. capture
def test_measure_is_capturable_and_replays_on_new_inputs():
    d = dev()
    case = CASES[3]
    pred, truth = (torch.tensor(v, device=d) for v in white(case))
    pred2, truth2 = (torch.tensor(v, device=d) for v in white(case, seed=1))
    sc = SpectralScore(pred.shape, case[3], case[4], device=d)
    pa, tb = pred.clone(), truth.clone()
    sc.measure(pa, tb)  # warm-up outside capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(device=d)
    s.wait_stream(torch.cuda.current_stream(d))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            m = sc.measure(pa, tb)
    torch.cuda.current_stream(d).wait_stream(s)
    pa.copy_(pred2)
    tb.copy_(truth2)
    sc.out.fill_(-7.0)
    g.replay()
    torch.cuda.synchronize()
    eager = SpectralScore(pred.shape, case[3], case[4], device=d)
    me = eager.measure(pred2, truth2)
    assert torch.equal(bits(sc.out), bits(eager.out)) and int(sc.nused.item()) == 4
    for q in ("error_ratio", "power_ratio", "coherence"):
        assert torch.equal(bits(m[q]), bits(me[q]))
    sc.measure(pred, truth)
    assert not torch.equal(bits(sc.out), bits(eager.out))  # the two fields do differ


# --------------------------------------------------------------------- 6. refusals
@pytest.mark.parametrize("H,W,P,Q,short", [(64, 64, 24, 12, 0), (64, 64, 8, 4, 0), (600, 600, 512, 256, 0),
                                           (48, 64, 64, 32, 0), (64, 64, 32, 0, 0), (64, 64, 32, 33, 0),
                                           (64, 64, 32, 16, 1)],
                         ids=["P24", "P8", "P512", "P>H", "Q0", "Q>P", "short-workspace"])
def test_refusals_leave_the_outputs_untouched(H, W, P, Q, short):
    d = dev()
    lib = _lib.load()
    a = torch.zeros((1, H, W), device=d)
    nbytes = spectra_workspace(1, 64, 64, 32, 16)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=d)
    out = torch.full((1, 4, 300), -7.0, device=d)
    nused = torch.full((1,), -3, dtype=torch.int32, device=d)
    rc = lib.srmi_spectra(ptr(a), ptr(a), 1, H, W, P, Q, ptr(ws), nbytes - short, ptr(out), ptr(nused),
                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == _lib.SRMI_ERR_ARG
    assert (out == -7.0).all() and int(nused.item()) == -3 and (ws == 0).all()
    if not short:
        n = C.c_size_t(5)
        assert lib.srmi_spectra_workspace(1, H, W, P, Q, C.byref(n)) == _lib.SRMI_ERR_ARG and n.value == 5
        with pytest.raises(ValueError):
            SpectralScore((1, H, W), P, Q, device=d)


# -------------------------------------------------------------------- 7. end to end
def _field(rng, C_, h, w):
    base = rng.randn(C_, h, w)
    return (base + np.roll(base, 1, 1) + np.roll(base, 1, 2)).astype(np.float32)


def test_score_spectra_is_score_plus_the_measure_of_its_images():
    d = dev()
    spec, model, flat = _small_rcan()
    rng = np.random.RandomState(51)
    hr = torch.tensor(_field(rng, 1, 160, 224) * 2 + 5, device=d)
    kw = dict(tile_lr=TILE, overlap=(4, 4), device=d)
    rs = RegionSuperResolver(spec, flat.to(d), (1, 40, 56), **kw)
    plain = RegionSuperResolver(spec, flat.to(d), (1, 40, 56), **kw)
    images, losses, spectra = rs.score_spectra(hr, window=64)
    images0, losses0 = plain.score(hr)
    assert set(spectra) == {"model", "interpolated"}
    for k in ("input", "interpolated", "model"):
        assert torch.equal(bits(images[k]), bits(images0[k]))
    for k in ("model", "interpolated"):
        assert torch.equal(bits(losses[k]), bits(losses0[k]))
    for k in ("model", "interpolated"):
        sc = SpectralScore((1, 160, 224), 64, device=d)
        assert sc.stride == 32
        m = sc.measure(images[k], hr)
        assert int(spectra[k]["nused"].item()) == 4 * 6
        for q in m:
            assert torch.equal(bits(m[q]), bits(spectra[k][q])), (k, q)
        assert torch.isfinite(spectra[k]["error_ratio"]).all()
    # a second call reuses the buffers and gives the same bits
    keep = {k: spectra[k]["power_error"].clone() for k in spectra}
    _, _, again = rs.score_spectra(hr, window=64)
    for k in keep:
        assert again[k]["power_error"].data_ptr() == spectra[k]["power_error"].data_ptr()
        assert torch.equal(bits(again[k]["power_error"]), bits(keep[k]))


def test_score_spectra_with_land_skips_the_coast():
    d = dev()
    spec, model, flat = _small_rcan()
    rng = np.random.RandomState(52)
    hr = _field(rng, 1, 160, 224) * 2 + 5
    hr[0, 40:72, 100:140] = np.nan  # land on whole LR pixels
    rs = RegionSuperResolver(spec, flat.to(d), (1, 40, 56), tile_lr=TILE, overlap=(4, 4), land=True, device=d)
    images, losses, spectra = rs.score_spectra(torch.tensor(hr, device=d), window=64)
    for k in ("model", "interpolated"):
        n = int((~so.skipped(images[k].cpu().numpy(), hr, 64, 32)).sum())
        print(f"{k}: {n} of 24 windows used")
        assert 0 < n < 24 and int(spectra[k]["nused"].item()) == n
        assert torch.isfinite(spectra[k]["power_error"]).all()
