"""The spectral score's definition on the CPU: the numpy oracle (tests/spectra_oracle.py)
against the properties the definition promises, the host helpers of srmi.spectra and
srmi.results, and the library's refusals where no GPU is needed."""
import ctypes as C

import numpy as np
import pytest

import spectra_oracle as so
from srmi import _lib
from srmi.results import SPECTRA_QUANTITIES, load_spectra, save_spectra
from srmi.spectra import effective_resolution, spectra_workspace

# (C, H, W, P, Q) -> (ny, nx): every supported P, every plan shape
PLANS = {(1, 16, 16, 16, 16): (1, 1), (2, 40, 56, 16, 12): (3, 5), (1, 48, 40, 32, 32): (2, 2),
         (2, 96, 80, 64, 32): (2, 2), (1, 160, 128, 128, 64): (2, 1), (1, 300, 272, 256, 128): (2, 2)}


def _fields(rng, C_, H, W):
    truth = (290.0 + 1.5 * rng.standard_normal((C_, H, W))).astype(np.float32)
    pred = (truth + 0.3 * rng.standard_normal((C_, H, W))).astype(np.float32)
    return pred, truth


@pytest.mark.parametrize("P", [16, 64, 256])
def test_parseval_over_all_bins(P):
    """The sum of a density over ALL bins (corners included) is the mean square of the
    detrended, tapered window over mean((h h)^2)."""
    rng = np.random.default_rng(1)
    pred, truth = _fields(rng, 1, P, P)
    dens = so.densities(pred[0], truth[0])
    h2 = np.outer(so.hann(P), so.hann(P)) ** 2
    ta, tb = so.tapered(pred[0]), so.tapered(truth[0])
    for got, ref in ((dens[0].sum(), (ta ** 2).mean() / h2.mean()), (dens[1].sum(), (tb ** 2).mean() / h2.mean()),
                     (dens[2].sum(), ((ta - tb) ** 2).mean() / h2.mean()), (dens[3].sum(), (ta * tb).mean() / h2.mean())):
        assert abs(got - ref) <= 1e-12 * abs(ref)


def test_plane_wave_lands_in_its_shell():
    """cos(2 pi (3 y + 4 x) / 64): |k| = 5.  The taper spreads each line over the
    neighbouring bins, so half of the power 0.5 stays in shell 5 and all of it in 4 .. 6."""
    P = 64
    y, x = np.mgrid[0:P, 0:P]
    f = np.cos(2 * np.pi * (3 * y + 4 * x) / P).astype(np.float32)[None]
    out, nused = so.spectra(f, f, P, P)
    assert nused == 1
    E = out[0, 0]
    assert abs(E.sum() - 0.5) < 1e-6
    assert abs(E[5] - 0.25) < 1e-3
    assert abs(E[4:7].sum() - 0.5) < 1e-6
    assert np.abs(np.delete(E, [4, 5, 6])).max() < 1e-12


def test_white_noise_keeps_pi_over_four():
    rng = np.random.default_rng(2)
    f = rng.standard_normal((1, 256, 256)).astype(np.float32)
    out, _ = so.spectra(f, f, 64, 32)
    assert abs(out[0, 0].sum() / f.var() - np.pi / 4) < 0.03


def test_equal_fields_have_no_error_and_unit_coherence():
    rng = np.random.default_rng(3)
    _, truth = _fields(rng, 2, 40, 56)
    out, nused = so.spectra(truth, truth, 16, 12)
    er, pr, coh = so.derived(out)
    assert nused == 15 and (out[:, 2] == 0).all() and (er == 0).all() and (pr == 1).all()
    assert np.abs(coh - 1).max() < 1e-12
    assert (out[:, 0] == out[:, 1]).all() and np.abs(out[:, 3] / out[:, 0] - 1).max() < 1e-14


def test_packed_transform_reproduces_both_fields():
    """Fa = (Z(k) + conj Z(-k)) / 2, Fb = (Z(k) - conj Z(-k)) / 2i for Z = FFT(a + i b)."""
    rng = np.random.default_rng(4)
    a, b = rng.standard_normal((2, 32, 32))
    Z = np.fft.fft2(a + 1j * b)
    Zm = np.conj(np.roll(Z[::-1, ::-1], 1, (0, 1)))
    scale = np.abs(Z).max()
    assert np.abs((Z + Zm) / 2 - np.fft.fft2(a)).max() < 1e-14 * scale
    assert np.abs((Z - Zm) / 2j - np.fft.fft2(b)).max() < 1e-14 * scale


@pytest.mark.parametrize("plan,count", list(PLANS.items()))
def test_window_counts(plan, count):
    from srmi.superres import lib_overlap_count
    _, H, W, P, Q = plan
    assert (len(so.origins(H, P, Q)), len(so.origins(W, P, Q))) == count
    assert (lib_overlap_count(H, P, Q), lib_overlap_count(W, P, Q)) == count
    assert so.origins(H, P, Q)[-1] == H - P and so.origins(W, P, Q)[-1] == W - P


def test_complex64_oracle_is_close_to_the_definition():
    rng = np.random.default_rng(5)
    pred, truth = _fields(rng, 1, 96, 80)
    o64, _ = so.spectra(pred, truth, 64, 32)
    o32, _ = so.spectra(pred, truth, 64, 32, dtype="complex64")
    e32 = (np.abs(o32 - o64) / (o64[:, 0] + o64[:, 1])[:, None]).max()
    assert 0 < e32 < 1e-6


def test_skip_rule_and_nused():
    """(2, 40, 56, 16, 12): origins y 0 12 24, x 0 12 24 36 40.  Pixel (13, 38) lies in the
    rows of windows 0 and 1 and in the columns of windows 2 (24 .. 39), 3 (36 .. 51): four
    windows, whichever field or channel holds the NaN."""
    rng = np.random.default_rng(6)
    pred, truth = _fields(rng, 2, 40, 56)
    full, n_full = so.spectra(pred, truth, 16, 12)
    assert n_full == 15
    p2 = pred.copy()
    p2[1, 13, 38] = np.nan
    skip = so.skipped(p2, truth, 16, 12)
    assert list(np.flatnonzero(skip)) == [2, 3, 7, 8]
    out, nused = so.spectra(p2, truth, 16, 12)
    assert nused == 11 and np.isfinite(out).all() and not np.allclose(out, full)
    t2 = truth.copy()
    t2[0, 13, 38] = np.inf
    out_t, nused_t = so.spectra(pred, t2, 16, 12)
    assert nused_t == 11 and np.array_equal(out_t, out)
    p3 = pred.copy()
    p3[0, ::8, ::8] = np.nan  # every window is dry
    out0, n0 = so.spectra(p3, truth, 16, 12)
    assert n0 == 0 and np.isnan(out0).all() and out0.shape == (2, 4, 9)


def test_effective_resolution():
    P = 16
    r = np.zeros((3, 9))
    r[0] = [9.0, 0.1, 0.2, 0.5, 0.9, 1, 1, 1, 1]     # shell 0 is not looked at; shell 3 reaches 0.5
    r[1] = [0.0, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.49]  # none does
    r[2] = [0.0, np.nan, 0.7, 0.1, 0.1, 0.1, 0.1, 0.1, 1.0]  # a NaN never reaches it
    assert effective_resolution(r, P) == [16 / 3, 2.0, 8.0]
    assert effective_resolution(r, P, threshold=0.9) == [4.0, 2.0, 2.0]
    import torch
    assert effective_resolution(torch.tensor(r), P) == [16 / 3, 2.0, 8.0]
    with pytest.raises(ValueError):
        effective_resolution(r, 32)


def test_save_spectra_round_trip(tmp_path):
    rng = np.random.default_rng(7)
    pred, truth = _fields(rng, 2, 40, 56)
    out, nused = so.spectra(pred, truth, 16, 12)
    er, pr, coh = so.derived(out)
    sp = {q: out[:, i].astype(np.float32) for i, q in enumerate(so.QUANTITIES)}
    sp.update(error_ratio=er.astype(np.float32), power_ratio=pr.astype(np.float32), coherence=coh.astype(np.float32),
              wavenumber=(np.arange(9) / 16).astype(np.float32), nused=np.array([nused], np.int32))
    sp["coherence"][1, 0] = np.nan
    path = save_spectra(str(tmp_path / "s.nc"), sp, 16, ["SST", "SSS"])
    back, window, names = load_spectra(path)
    assert window == 16 and names == ["SST", "SSS"] and int(back["nused"][0]) == 15
    for q in SPECTRA_QUANTITIES + ("wavenumber",):
        assert back[q].dtype == np.float32 and np.array_equal(back[q], sp[q], equal_nan=True), q
    from scipy.io import netcdf_file
    with netcdf_file(path, "r", mmap=False) as f:
        assert f.variables["power_error"].dimensions == ("channel", "shell")
        assert f.variables["wavenumber"].dimensions == ("shell",)
    with pytest.raises(ValueError):
        save_spectra(str(tmp_path / "t.nc"), {k: v for k, v in sp.items() if k != "cross"}, 16, ["SST", "SSS"])
    with pytest.raises(ValueError):
        save_spectra(str(tmp_path / "t.nc"), sp, 16, ["SST"])


REFUSED = [(1, 64, 64, 24, 12), (1, 64, 64, 8, 4), (1, 600, 600, 512, 256), (1, 48, 64, 64, 32), (1, 64, 48, 64, 32),
           (1, 64, 64, 32, 0), (1, 64, 64, 32, 33), (0, 64, 64, 32, 16)]


@pytest.mark.parametrize("args", REFUSED)
def test_library_refuses_bad_plans(args):
    lib = _lib.load()
    n = C.c_size_t(77)
    assert lib.srmi_spectra_workspace(*args, C.byref(n)) == _lib.SRMI_ERR_ARG and n.value == 77
    with pytest.raises(ValueError):
        spectra_workspace(*args)
    # srmi_spectra checks the plan before it touches a pointer or launches anything
    assert lib.srmi_spectra(None, None, *args, None, 0, None, None, None) == _lib.SRMI_ERR_ARG


def test_workspace_is_bounded_by_the_grid():
    """4096^2 at P = 256, Q = 128: 961 windows, but at most 512 scratch planes of 512 KiB."""
    lib = _lib.load()
    assert lib.srmi_spectra_workspace(1, 64, 64, 32, 16, None) == _lib.SRMI_ERR_ARG
    small = spectra_workspace(2, 300, 272, 256, 128)
    assert small < 8 * 2 ** 20
    big = spectra_workspace(2, 4096, 4096, 256, 128)
    partials = 961 * 2 * 4 * 129 * 8
    assert 512 * 2 ** 19 + partials <= big <= 512 * 2 ** 19 + partials + 2 ** 16
    assert spectra_workspace(2, 4096, 4096, 64, 32) < 2 ** 30  # no scratch planes below P = 128
