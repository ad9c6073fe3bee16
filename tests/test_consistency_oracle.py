"""The consistency oracle (tests/consistency_oracle.py) against torch's F.interpolate and
against itself (LR-space form == the literal HR-space loop, D U == the clamped stencil,
M E M contracts), the 'residual' variable of save_superres_results and the validation of
RegionSuperResolver(consistent=).  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import consistency_oracle as co

MODES = ("bilinear", "bicubic")
PAIRS = [(um, dm) for um in MODES for dm in MODES]


def gpu_masks(h, w):
    """The active patterns the GPU tests use on an [h, w] plane, by name."""
    full = np.ones((h, w), bool)
    corner = full.copy()
    corner[0, 0] = False
    one_wet = np.zeros((h, w), bool)
    one_wet[h // 2, w // 2] = True
    hole = full.copy()
    hole[h // 3, w // 2] = False
    return {"full": full, "dry_corner": corner, "one_wet": one_wet, "all_dry": np.zeros((h, w), bool), "hole": hole}


def masked_fields(rng, C, h, w, s, pattern):
    """(x [C, h s, w s], lr [C, h, w]) whose oracle active set is gpu_masks()[pattern] in
    every channel: dry cells are NaN in lr and over their whole HR block."""
    x = rng.randn(C, h * s, w * s)
    lr = rng.randn(C, h, w)
    dry = ~gpu_masks(h, w)[pattern]
    lr[:, dry] = np.nan
    x[:, np.repeat(np.repeat(dry, s, 0), s, 1)] = np.nan
    return x, lr


@pytest.mark.parametrize("s", [4, 8])
@pytest.mark.parametrize("mode", MODES)
def test_D_and_U_are_F_interpolate(s, mode):
    rng = np.random.RandomState(71)
    for h, w in ((1, 1), (2, 3), (5, 7), (13, 6)):
        x = rng.randn(2, 3, h * s, w * s)
        ref = F.interpolate(torch.tensor(x), scale_factor=1.0 / s, mode=mode, align_corners=False).numpy()
        assert np.max(np.abs(co.D(x, s, mode) - ref)) <= 1e-12
        r = rng.randn(2, 3, h, w)
        ref = F.interpolate(torch.tensor(r), scale_factor=float(s), mode=mode, align_corners=False).numpy()
        assert np.max(np.abs(co.U(r, s, mode) - ref)) <= 1e-12


@pytest.mark.parametrize("s", [4, 8])
@pytest.mark.parametrize("mode", MODES)
def test_D_reads_only_its_block(s, mode):
    """A NaN at a tap of D blanks that LR cell alone; one outside the taps blanks none."""
    x = np.random.RandomState(72).randn(3 * s, 4 * s)
    a = s // 2 - (2 if mode == "bicubic" else 1)
    y = x.copy()
    y[s + a, 2 * s + a] = np.nan
    bad = np.isnan(co.D(y, s, mode))
    assert bad.sum() == 1 and bad[1, 2]
    if a > 0:
        y = x.copy()
        y[s, 2 * s] = np.nan
        assert not np.isnan(co.D(y, s, mode)).any()


@pytest.mark.parametrize("um,dm", PAIRS)
@pytest.mark.parametrize("s", [4, 8])
def test_du_is_the_clamped_stencil(s, um, dm):
    g = co.du_coeffs(s, um, dm)
    assert abs(g.sum() - 1.0) <= 1e-14 and np.allclose(g, g[::-1], atol=1e-15)
    if um == "bilinear":
        assert g[0] == 0.0 and g[4] == 0.0
    for n in (1, 2, 3, 4, 5, 6, 11):  # fields narrower than the stencil included
        assert np.max(np.abs(co.du_dense(n, s, um, dm) - co.du_stencil_matrix(n, g))) <= 1e-14, n


@pytest.mark.parametrize("um,dm", PAIRS)
@pytest.mark.parametrize("s", [4, 8])
@pytest.mark.parametrize("pattern", ["full", "dry_corner", "hole", "one_wet"])
def test_lr_form_is_the_literal_loop(s, um, dm, pattern):
    rng = np.random.RandomState(73)
    x, lr = masked_fields(rng, 2, 6, 7, s, pattern)
    if pattern == "hole":  # a NaN under a finite LR cell as well
        x[1, 2 * s + s // 2, 3 * s + s // 2] = np.nan
    for K in (1, 3, 8):
        xk, r0, rk, active = co.correct(x, lr, s, um, dm, K)
        xl, rl = co.backproject_hr(x, lr, s, um, dm, K)
        assert np.array_equal(np.isnan(xk), np.isnan(x)) and np.array_equal(np.isnan(xl), np.isnan(x))
        fin = np.isfinite(x)
        assert np.max(np.abs(xk[fin] - xl[fin])) <= 1e-10
        assert np.max(np.abs(rk - rl)) <= 1e-10
        assert np.all(rk[~active] == 0.0) and np.all(r0[~active] == 0.0)


@pytest.mark.parametrize("um,dm", PAIRS)
@pytest.mark.parametrize("s", [4, 8])
def test_mem_contracts(s, um, dm, capsys):
    """The spectral radius of M E M is below 1 for every mode pair, scale and mask pattern
    of the GPU tests (and a random 30 % mask): what makes the end-to-end bar meaningful."""
    rng = np.random.RandomState(74)
    for h, w in ((5, 5), (13, 21)):
        masks = gpu_masks(h, w)
        masks["random30"] = rng.rand(h, w) >= 0.3
        for name, m in masks.items():
            rho = co.spectral_radius(m, s, um, dm)
            print(f"rho(M E M) s={s} U={um} D={dm} {h}x{w} {name}: {rho:.4f}")
            assert rho < 1.0, (name, rho)


def test_quoted_radii():
    """The radii the design quotes (16 x 16 LR field), to the digits quoted."""
    full = np.ones((16, 16), bool)
    want = {(4, "bicubic", "bicubic"): 0.033, (8, "bicubic", "bicubic"): 0.016, (4, "bicubic", "bilinear"): 0.162,
            (8, "bicubic", "bilinear"): 0.044, (4, "bilinear", "bicubic"): 0.286, (8, "bilinear", "bicubic"): 0.149,
            (4, "bilinear", "bilinear"): 0.434, (8, "bilinear", "bilinear"): 0.232}
    for (s, um, dm), rho in want.items():
        assert abs(co.spectral_radius(full, s, um, dm) - rho) <= 6e-4, (s, um, dm)


def test_superres_results_round_trip_with_residual(tmp_path):
    from functools import partial
    from srmi import results as R
    rng = np.random.RandomState(75)
    C, h, w, s = 2, 9, 14, 4
    images = {"input": rng.randn(C, h, w).astype(np.float32),
              "interpolated": rng.randn(C, h * s, w * s).astype(np.float32),
              "model": rng.randn(C, h * s, w * s).astype(np.float32),
              "residual": rng.randn(C, h, w).astype(np.float32),
              "residual_left": rng.randn(C, h, w).astype(np.float32)}
    images["residual"][1, 2, 3] = 0.0
    names = ["SSS", "SST"]

    def path_for(sub):
        return partial(R.results_path, str(tmp_path / sub), "swot", "superres-48", timestep=0, structure="image")

    paths = R.save_superres_results(lambda v: path_for("res")(varname=v), images, names, {"model": 0.5})
    for iv, p in enumerate(paths):
        back, bl = R.load_inference_results(p)
        assert bl == {"model": 0.5} and sorted(back) == ["input", "interpolated", "model", "residual"]
        for k in back:
            np.testing.assert_array_equal(back[k].values, images[k][iv].astype(np.float64))
        assert back["model"].dims == ("y", "x")
        from scipy.io import netcdf_file
        with netcdf_file(p, "r", mmap=False) as f:
            assert tuple(f.variables["residual"].dimensions) == tuple(f.variables["input"].dimensions) == ("ys", "xs")
    three = {k: images[k] for k in ("input", "interpolated", "model")}
    pa = R.save_superres_results(lambda v: path_for("three")(varname=v), three, names, {"model": 0.5})
    others = dict(three, residual_left=images["residual_left"])
    pb = R.save_superres_results(lambda v: path_for("left")(varname=v), others, names, {"model": 0.5})
    for a, b, c in zip(pa, pb, paths):
        assert open(a, "rb").read() == open(b, "rb").read() != open(c, "rb").read()


def test_consistent_argument_validation():
    from srmi.engine import NetSpec
    from srmi.superres import RegionSuperResolver, check_consistent
    assert check_consistent(0, 3, "nearest", "nearest") == 0  # K = 0 asks nothing of the task
    assert check_consistent(3, 4, "bicubic", "bicubic") == 3 and check_consistent(16, 2, "bilinear", "bicubic") == 16
    assert check_consistent(np.int64(2), 8, "bicubic", "bilinear") == 2
    for bad in (-1, 17, 1.0, True, "3", None):
        with pytest.raises(ValueError):
            check_consistent(bad, 4, "bicubic", "bicubic")
    for s, dm in ((2, "bicubic"), (3, "bilinear"), (5, "bicubic"), (1, "bilinear")):
        with pytest.raises(ValueError):
            check_consistent(1, s, dm, "bicubic")
    # the constructor refuses before it touches a device
    spec = NetSpec(arch="rcan", nchannels_in=1, nchannels_out=1, nlayers=1, nblocks=1, scale=2)
    params = torch.zeros(8)
    with pytest.raises(ValueError, match="consistent"):
        RegionSuperResolver(spec, params, (1, 64, 64), norm="lnorm", consistent=2)
    spec4 = NetSpec(arch="rcan", nchannels_in=1, nchannels_out=1, nlayers=1, nblocks=1, scale=4)
    with pytest.raises(ValueError, match="consistent"):
        RegionSuperResolver(spec4, params, (1, 64, 64), norm="lnorm", consistent=17)


def test_symbols_are_declared():
    from srmi import _lib
    lib = _lib.load()
    for name in ("srmi_consistency_residual", "srmi_consistency_iterate", "srmi_consistency_apply"):
        assert name in _lib.EXPORTED and hasattr(lib, name)
