"""The gradient score's and the gradient loss term's oracle (tests/gradient_oracle.py) against
torch.autograd, central differences and fields whose gradients are known analytically; no
GPU.  The closed-form gradient is the one the device implements (include/srmi.h, "the gradient
loss term")."""
import os

import numpy as np
import pytest
import torch

import gradient_oracle as go

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("srmi_gradient_workspace", "srmi_gradient", "srmi_gradient_loss_workspace", "srmi_gradient_loss_parts",
           "srmi_gradient_loss_from_parts", "srmi_gradient_loss_dy")


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
    p, t = smooth((2, 14, 19), 1)
    p[0, 3, 4] = np.nan
    t[0, 9, 15] = np.nan
    t[1, 6, 10] = np.inf
    p[1, 0, 0] = -np.inf
    p[1, 13, 18] = np.nan
    return p, t


CASES = {
    "nan 14x19": nan_case,
    "290 other mean": lambda: smooth((1, 20, 17), 2, mean=290.0, std=1.5, gain=0.8, shift=0.4),
    "3x3": lambda: smooth((3, 3, 3), 3),
    "two planes 30x27": lambda: smooth((2, 30, 27), 4),
}


def autograd(p, t, eps=go.EPS):
    pt = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    loss, nused = go.loss_torch(pt, torch.tensor(t, dtype=torch.float64), eps)
    loss.backward()
    return float(loss.detach()), nused, pt.grad.numpy()


@pytest.mark.parametrize("name", list(CASES))
def test_closed_form_gradient_is_autograd(name):
    p, t = CASES[name]()
    ref = go.loss_and_grad(p, t)
    loss, nused, g = autograd(p, t)
    g = np.where(np.isfinite(g), g, 0.0)  # a NaN prediction pixel takes no gradient
    assert nused == ref["nused"] and nused > 0
    assert abs(loss - ref["loss"]) <= 1e-14 * abs(loss)
    err = np.abs(g - ref["grad"]).max()
    print(f"{name}: loss {loss:.6e} nused {nused} max |closed - autograd| {err:.2e}")
    assert err <= 1e-15
    assert (ref["grad"][~ref["fin"]] == 0).all()


def test_closed_form_gradient_is_central_difference():
    p, t = nan_case()
    ref = go.loss_and_grad(p, t)
    rng = np.random.default_rng(5)
    p64 = p.astype(np.float64)
    fin = np.argwhere(ref["fin"])
    h = 1e-5
    for idx in fin[rng.choice(len(fin), 24, replace=False)]:
        idx = tuple(idx)
        up, dn = p64.copy(), p64.copy()
        up[idx] += h
        dn[idx] -= h
        cd = (go.loss_and_grad(up, t)["loss"] - go.loss_and_grad(dn, t)["loss"]) / (2 * h)
        assert abs(cd - ref["grad"][idx]) <= 1e-8 + 1e-6 * abs(cd), (idx, cd, ref["grad"][idx])


def test_equal_fields_give_sqrt_eps_and_a_zero_gradient():
    _, t = smooth((2, 12, 13), 6, mean=290.0, std=1.5)
    for dtype in (np.float64, np.float32):
        r = go.loss_and_grad(t.copy(), t, eps=1e-6, dtype=dtype)
        assert abs(r["loss"] - np.sqrt(dtype(1e-6))) <= 1e-9
        assert (r["grad"] == 0).all()
        assert r["nused"] == 2 * 10 * 11


def test_no_used_position_gives_zero_not_nan():
    p, t = smooth((2, 5, 6), 7)
    t[:, 2, :] = np.nan  # every 3x3 window of a 5-row plane touches row 1, 2 or 3
    t[:, 1, :] = np.nan
    t[:, 3, :] = np.nan
    r = go.loss_and_grad(p, t)
    assert r["nused"] == 0 and r["loss"] == 0.0 and (r["grad"] == 0).all()
    pt = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    loss, n = go.loss_torch(pt, torch.tensor(t, dtype=torch.float64))
    loss.backward()
    assert n == 0 and float(loss.detach()) == 0.0 and (pt.grad.numpy() == 0).all()


def test_the_mean_is_over_positions_not_planes():
    p, t = smooth((2, 16, 16), 8)
    p[1] = t[1] + 3.0 * (p[1] - t[1])  # another error level on the plane that loses positions
    t[1, 4:12, 4:12] = np.nan
    r = go.loss_and_grad(p, t)
    c = r["counts"]
    assert c[0] == 14 * 14 and 0 < c[1] < c[0]
    per_plane = r["parts"] / c
    assert abs(r["loss"] - r["parts"].sum() / c.sum()) <= 1e-15
    assert abs(r["loss"] - per_plane.mean()) > 1e-3  # the mean of the plane means is another number
    # and the gradient of a pixel of plane 0 is scaled by the global count
    one = go.loss_and_grad(p[:1], t[:1])
    np.testing.assert_allclose(r["grad"][0] * c.sum(), one["grad"][0] * c[0], rtol=1e-12, atol=1e-18)


def test_fp32_closed_form_is_close_to_fp64_and_not_identical():
    p, t = smooth((1, 40, 36), 9, mean=290.0, std=1.5, gain=0.8, shift=0.4)
    r64, r32 = go.loss_and_grad(p, t), go.loss_and_grad(p, t, dtype=np.float32)
    rel = np.linalg.norm(r32["grad"] - r64["grad"]) / np.linalg.norm(r64["grad"])
    print(f"fp32 closed form against fp64: gradient rel-L2 {rel:.2e}, loss rel "
          f"{abs(r32['loss'] - r64['loss']) / r64['loss']:.2e}")
    assert 0 < rel < 1e-5
    assert abs(r32["loss"] - r64["loss"]) < 1e-6 * r64["loss"]


def test_score_of_planes_with_known_gradients():
    """f = alpha x + beta y has gx = alpha / dx and gy = beta / dy exactly; against a truth of
    another slope, sharpness = |g_p| / |g_t| and cosine = g_p . g_t / (|g_p| |g_t|)."""
    H, W = 9, 11
    y, x = np.mgrid[:H, :W].astype(np.float64)
    ap, bp, at, bt = 0.5, 0.25, 0.125, -0.75
    p = (ap * x + bp * y)[None].astype(np.float32)
    t = (at * x + bt * y + 3.0)[None].astype(np.float32)
    dy, dx = 2.0, 0.5
    for dtype in (np.float64, np.float32):
        r = go.score(p, t, spacing=(dy, dx), dtype=dtype)
        gp, gt = np.array([ap / dx, bp / dy]), np.array([at / dx, bt / dy])
        assert r["count"][0] == (H - 2) * (W - 2)
        np.testing.assert_allclose(r["mean_pred"][0], np.linalg.norm(gp), rtol=1e-7)
        np.testing.assert_allclose(r["mean_truth"][0], np.linalg.norm(gt), rtol=1e-7)
        np.testing.assert_allclose(r["sharpness"][0], np.linalg.norm(gp) / np.linalg.norm(gt), rtol=1e-7)
        np.testing.assert_allclose(r["cosine"][0], gp @ gt / (np.linalg.norm(gp) * np.linalg.norm(gt)), rtol=1e-7)
        np.testing.assert_allclose(r["rmse_vec"][0], np.linalg.norm(gp - gt), rtol=1e-7)
        np.testing.assert_allclose(r["rmse_mag"][0], abs(np.linalg.norm(gp) - np.linalg.norm(gt)), rtol=1e-6)
        m = r["gmag_pred"][0]
        assert np.isnan(m[0]).all() and np.isnan(m[-1]).all() and np.isnan(m[:, 0]).all() and np.isnan(m[:, -1]).all()
        np.testing.assert_allclose(m[1:-1, 1:-1], np.linalg.norm(gp), rtol=1e-7)


def test_score_mask_costs_a_one_pixel_rim_and_an_empty_channel_is_nan():
    p, t = smooth((2, 8, 9), 10)
    p[0, 4, 4] = np.nan
    t[1] = np.nan
    r = go.score(p, t)
    assert r["count"][0] == 6 * 7 - 9 and r["count"][1] == 0
    assert np.isnan(r["gmag_truth"][0][3:6, 3:6]).all() and np.isfinite(r["gmag_truth"][0][2, 2])
    assert all(np.isnan(r[k][1]) for k in go.STATS + go.SUMS)


def test_check_gradient_loss_config():
    from srmi.gradient import check_gradient_loss_config, check_spacing
    assert check_gradient_loss_config(1, 1e-6) == (1.0, 1e-6)
    assert check_gradient_loss_config(0.0, 0.5) == (0.0, 0.5)
    for w, e in ((-1.0, 1e-6), (float("nan"), 1e-6), (float("inf"), 1e-6), (1e39, 1e-6), ("1", 1e-6), (True, 1e-6),
                 (None, 1e-6), (1.0, 0.0), (1.0, -1e-6), (1.0, float("nan")), (1.0, float("inf")), (1.0, 1e-50),
                 (1.0, None), (1.0, "x"), (1.0, True)):
        with pytest.raises(ValueError):
            check_gradient_loss_config(w, e)
    assert check_spacing((2.0, 0.5)) == (0.5, 2.0)
    for s in ((0.0, 1.0), (1.0, -1.0), (float("nan"), 1.0), (1.0, float("inf")), (1.0,), 1.0, ("a", 1.0), (1e-45, 1.0)):
        with pytest.raises(ValueError):
            check_spacing(s)


def test_save_and_load_gradient_round_trip(tmp_path):
    from srmi.results import load_gradient, save_gradient
    p, t = smooth((2, 8, 9), 11)
    p[0, 4, 4] = np.nan
    t[1] = np.nan  # an empty channel: NaN scalars survive
    r = go.score(p, t, spacing=(2.0, 0.5), dtype=np.float32)
    full = {k: r[k] for k in go.STATS + ("count", "gmag_pred", "gmag_truth")}
    full["sums"] = np.stack([r[k] for k in go.SUMS], axis=1)
    path = save_gradient(str(tmp_path / "g.nc"), full, ["SST", "SSS"], spacing=(2.0, 0.5))
    back, names, spacing = load_gradient(path)
    assert names == ["SST", "SSS"] and spacing == (2.0, 0.5)
    assert back["count"].dtype == np.int64 and (back["count"] == r["count"]).all()
    for k in go.STATS + ("sums", "gmag_pred", "gmag_truth"):
        np.testing.assert_array_equal(back[k], full[k])
    scalars = {k: r[k] for k in go.STATS + ("count",)}
    back, _, _ = load_gradient(save_gradient(str(tmp_path / "s.nc"), scalars, ["SST", "SSS"]))
    assert "gmag_pred" not in back and "sums" not in back
    with pytest.raises(ValueError):
        save_gradient(str(tmp_path / "bad.nc"), {"count": r["count"]}, ["SST", "SSS"])


def test_the_tile_size_python_states_is_the_librarys():
    """GRADIENT_TILE places the GPU tests' seam cases: the score's workspace is 64 bytes per
    rectangle a workgroup owns, so its size says where one more row or column opens a new one."""
    import ctypes as C

    from srmi import _lib
    from srmi.gradient import GRADIENT_TILE
    lib = _lib.load()
    th, tw = GRADIENT_TILE

    def nbytes(H, W):
        n = C.c_size_t(0)
        assert lib.srmi_gradient_workspace(1, H, W, C.byref(n)) == 0
        return n.value
    assert nbytes(th, tw) == 64 and nbytes(th + 1, tw) == 128 and nbytes(th, tw + 1) == 128
    assert nbytes(2 * th, 3 * tw) == 6 * 64 and nbytes(2 * th + 1, 3 * tw + 1) == 12 * 64
    n1, n2 = C.c_size_t(0), C.c_size_t(0)  # the loss term's kernels tile alike: 8 + 4 bytes, each rounded up to 16
    assert lib.srmi_gradient_loss_workspace(1, th, tw, C.byref(n1)) == 0 and n1.value == 32
    assert lib.srmi_gradient_loss_workspace(1, th + 1, 2 * tw + 1, C.byref(n2)) == 0 and n2.value == 48 + 32


def test_symbols_are_declared_and_bound():
    from srmi import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "srmi.h")).read()
    for name in SYMBOLS:
        assert name in _lib.EXPORTED and hasattr(lib, name) and f"int {name}(" in header
    import srmi.gradient as sg
    for name in ("GradientScore", "GradientLoss", "check_gradient_loss_config"):
        assert hasattr(sg, name)

