"""The SSIM loss term's oracle (tests/ssim_loss_oracle.py) against torch.autograd, central
differences and the SSIM score's oracle; no GPU.  The closed-form gradient is the one the
device implements (include/srmi.h, "the SSIM loss term")."""
import os

import numpy as np
import pytest
import torch

import ssim_loss_oracle as slo
import ssim_oracle as so

SYMBOLS = ("srmi_ssim_loss_workspace", "srmi_ssim_loss_parts", "srmi_ssim_loss_from_parts", "srmi_ssim_loss_dy")


def smooth(shape, seed, mean=0.0, std=1.0, noise=0.3, gain=1.0, shift=0.0):
    """A smooth truth (a sum of a few waves plus white noise) at `mean` +- `std`, and a
    prediction gain * (truth - mean) + mean + shift + noise, fp32."""
    rng = np.random.default_rng(seed)
    H, W = shape[-2:]
    y, x = np.mgrid[:H, :W]
    t = np.zeros(shape)
    for idx in np.ndindex(*shape[:-2]):
        ph = rng.uniform(0, 2 * np.pi, 3)
        t[idx] = (np.sin(0.21 * y + ph[0]) * np.cos(0.13 * x + ph[1]) + 0.5 * np.sin(0.05 * (x + y) + ph[2])
                  + 0.3 * rng.standard_normal((H, W)))
    t = mean + std * t
    p = gain * (t - mean) + mean + shift + std * noise * rng.standard_normal(shape)
    return p.astype(np.float32), t.astype(np.float32)


def nan_case():
    p, t = smooth((2, 24, 32), 1)
    p[0, 3, 4] = np.nan
    t[0, 17, 25] = np.nan
    t[1, 12, 20] = np.inf
    return p, t


CASES = {
    "nan 24x32": lambda: nan_case() + (None,),
    "290 other mean": lambda: smooth((1, 40, 36), 2, mean=290.0, std=1.5, gain=0.8, shift=0.4) + (None,),
    "192 tile": lambda: smooth((1, 192, 192), 3) + (None,),
    "data_range 20": lambda: smooth((2, 30, 27), 4) + (20.0,),
}


def autograd(p, t, data_range):
    pt = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    loss, nused = slo.loss_torch(pt, torch.tensor(t, dtype=torch.float64), data_range)
    loss.backward()
    return float(loss.detach()), nused, pt.grad.numpy()


@pytest.mark.parametrize("name", list(CASES))
def test_closed_form_gradient_is_autograd(name):
    p, t, dr = CASES[name]()
    ref = slo.loss_and_grad(p, t, dr)
    loss, nused, g = autograd(p, t, dr)
    g = np.where(np.isfinite(g), g, 0.0)  # a NaN prediction pixel takes no gradient
    rel = float(np.linalg.norm(ref["grad"] - g) / np.linalg.norm(g))
    print(f"{name}: loss {ref['loss']:.12f} autograd {loss:.12f}, nused {nused}, gradient rel-L2 {rel:.3e}")
    assert nused == ref["nused"] > 0
    assert abs(ref["loss"] - loss) <= 1e-13
    assert rel <= 1e-12
    assert (ref["grad"][~ref["fin"]] == 0).all()


def test_closed_form_gradient_against_central_differences():
    p, t = nan_case()
    ref = slo.loss_and_grad(p, t)
    p64 = p.astype(np.float64)
    h = 1e-5
    for idx in ((0, 0, 0), (0, 8, 9), (0, 3, 9), (1, 12, 15), (1, 23, 31), (0, 20, 27)):
        assert ref["fin"][idx]
        up, dn = p64.copy(), p64.copy()
        up[idx] += h
        dn[idx] -= h
        fd = (slo.loss_and_grad(up, t)["loss"] - slo.loss_and_grad(dn, t)["loss"]) / (2 * h)
        print(f"pixel {idx}: closed form {ref['grad'][idx]:.6e}, central difference {fd:.6e}")
        assert abs(fd - ref["grad"][idx]) <= 1e-6 * np.abs(ref["grad"]).max() + 1e-9
    # fp64 inputs: the same r and L are needed for the differences to be of one function
    assert slo.plane_range(t[0])[0].dtype == np.float32


def test_one_plane_is_one_minus_the_score():
    for dr in (None, 20.0):
        p, t = smooth((1, 37, 70), 5, mean=290.0, std=1.5)
        score = so.ssim(p, t, dr)
        ref = slo.loss_and_grad(p, t, dr)
        assert ref["nused"] == score["nwin"][0] == 27 * 60
        assert abs((1.0 - ref["loss"]) - score["ssim"][0]) <= 1e-15
        assert np.array_equal(ref["ssim"][0], score["map"][0, 5:-5, 5:-5])
        # fp32: the same arithmetic as the score's fp32 oracle, bit for bit
        s32, r32 = so.ssim(p, t, dr, dtype=np.float32), slo.loss_and_grad(p, t, dr, dtype=np.float32)
        assert np.array_equal(r32["ssim"][0], s32["map"][0, 5:-5, 5:-5])


def test_equal_fields_give_zero_loss_and_no_gradient():
    _, t = smooth((2, 24, 40), 6, mean=290.0, std=1.5)
    ref = slo.loss_and_grad(t, t)
    assert ref["nused"] == 2 * 14 * 30
    assert abs(ref["loss"]) <= 1e-15
    # every first derivative of ssim vanishes at a == b: what is left is rounding, against a
    # gradient that is of the order 1 / (Nused * the target's spread) for an unrelated prediction
    other = slo.loss_and_grad(smooth((2, 24, 40), 7, mean=290.0, std=1.5)[0], t)
    print(f"a == b: largest |gradient| {np.abs(ref['grad']).max():.3e} against {np.abs(other['grad']).max():.3e}")
    assert np.abs(ref["grad"]).max() <= 1e-12 * np.abs(other["grad"]).max()


def test_no_used_position_is_zero_not_nan():
    p, t = smooth((2, 24, 32), 8)
    t[:, ::8, ::8] = np.nan
    for dtype in (np.float64, np.float32):
        ref = slo.loss_and_grad(p, t, dtype=dtype)
        assert ref["nused"] == 0 and ref["loss"] == 0.0 and ref["S"] == 0.0
        assert (ref["grad"] == 0).all() and (ref["counts"] == 0).all() and (ref["parts"] == 0).all()
    loss, nused, g = autograd(p, t, None)
    assert loss == 0.0 and nused == 0 and (g == 0).all()
    # a plane that is all NaN in the target: no finite pixel, r and L are NaN
    p, t = smooth((2, 24, 32), 8)
    t[1] = np.nan
    ref = slo.loss_and_grad(p, t)
    assert ref["counts"].tolist() == [14 * 22, 0] and (ref["grad"][1] == 0).all() and np.isfinite(ref["loss"])


def test_a_constant_target_plane_is_skipped():
    p, t = smooth((3, 24, 32), 9)
    t[1] = 2.5
    ref = slo.loss_and_grad(p, t)
    assert ref["counts"].tolist() == [14 * 22, 0, 14 * 22]
    assert ref["parts"][1] == 0 and (ref["grad"][1] == 0).all() and np.isfinite(ref["grad"]).all()
    only = slo.loss_and_grad(p[[0, 2]], t[[0, 2]])
    assert ref["loss"] == only["loss"] and np.array_equal(ref["grad"][[0, 2]], only["grad"])
    loss, nused, g = autograd(p, t, None)
    assert nused == ref["nused"] and abs(loss - ref["loss"]) <= 1e-13 and (g[1] == 0).all()
    # with a given data_range the plane has an L and takes part
    given = slo.loss_and_grad(p, t, 20.0)
    assert given["counts"].tolist() == [14 * 22] * 3 and np.abs(given["grad"][1]).max() > 0


def test_the_mean_is_over_positions_not_over_planes():
    p, t = smooth((2, 24, 32), 10)
    p[1] = t[1] + 3.0 * (p[1] - t[1])  # a much worse plane ...
    t[1, :8, :10] = np.nan             # ... with fewer used positions
    ref = slo.loss_and_grad(p, t)
    n0, n1 = ref["counts"]
    assert n0 == 14 * 22 and n1 == n0 - 8 * 10
    m0, m1 = ref["parts"][0] / n0, ref["parts"][1] / n1
    over_positions = 1.0 - (ref["parts"][0] + ref["parts"][1]) / (n0 + n1)
    over_planes = 1.0 - 0.5 * (m0 + m1)
    assert abs(ref["loss"] - over_positions) <= 1e-15
    assert abs(over_positions - over_planes) > 1e-3
    # the gradient of plane 0 carries 1 / (n0 + n1), not 1 / (2 n0)
    alone = slo.loss_and_grad(p[:1], t[:1])
    np.testing.assert_allclose(ref["grad"][0] * (n0 + n1), alone["grad"][0] * n0, rtol=1e-13, atol=1e-18)


def test_fp32_closed_form_is_close_and_not_identical():
    for name in ("nan 24x32", "290 other mean"):
        p, t, dr = CASES[name]()
        g64, g32 = slo.loss_and_grad(p, t, dr)["grad"], slo.loss_and_grad(p, t, dr, dtype=np.float32)["grad"]
        rel = float(np.linalg.norm(g32 - g64) / np.linalg.norm(g64))
        print(f"{name}: the fp32 closed form is {rel:.3e} rel-L2 from fp64")
        assert 0 < rel < 5e-6


def test_check_ssim_loss_config():
    from srmi.ssim import check_ssim_loss_config
    assert check_ssim_loss_config(1, None) == (1.0, 0.0)
    assert check_ssim_loss_config(0.0, 20) == (0.0, 20.0)
    assert check_ssim_loss_config(0.25, -3.0) == (0.25, 0.0) and check_ssim_loss_config(2.0, 0) == (2.0, 0.0)
    for bad in (-0.5, float("nan"), float("inf"), 1e39, "1", None, True):
        with pytest.raises(ValueError, match="weight"):
            check_ssim_loss_config(bad, None)
    for bad in (float("nan"), float("inf"), -float("inf"), 1e39, "20", True):
        with pytest.raises(ValueError, match="data_range"):
            check_ssim_loss_config(1.0, bad)


def test_symbols_are_bound_and_declared():
    from srmi import _lib
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "srmi.h")).read()
    for name in SYMBOLS:
        assert name in _lib.EXPORTED and hasattr(lib, name) and f"int {name}(" in header
