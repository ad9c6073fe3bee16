"""The spectral loss oracle (tests/spectral_loss_oracle.py) against itself, on the CPU: the
closed-form gradient against autograd through torch.fft.fft2, the two degenerate inputs,
the skipping rule, the job plan and the scale of the term next to the RMSE."""
import numpy as np
import pytest
import torch

import overlap_oracle as oo
import spectral_loss_oracle as slo

PLANS = [(16, 8, 32, 48), (32, 32, 80, 72), (64, 32, 192, 192)]


def fields(P, Q, H, W, seed=0, N=1, C=2):
    rng = np.random.default_rng(200 + seed)
    t = rng.standard_normal((N, C, H, W))
    return t + 0.3 * rng.standard_normal((N, C, H, W)), t


@pytest.mark.parametrize("P,Q,H,W", PLANS)
def test_closed_form_gradient_is_autograd(P, Q, H, W):
    p, t = fields(P, Q, H, W)
    ref = slo.loss_and_grad(p, t, P, Q)
    pt = torch.tensor(p, requires_grad=True)
    loss, nused = slo.loss_torch(pt, torch.tensor(t), P, Q)
    loss.backward()
    rel = float(np.linalg.norm(pt.grad.numpy() - ref["grad"]) / np.linalg.norm(ref["grad"]))
    print(f"plan {(P, Q, H, W)}: loss {ref['loss']:.12f} torch {float(loss.detach()):.12f}, gradient rel-L2 {rel:.2e}")
    assert nused == ref["nused"] == 2 * len(slo.windows(H, W, P, Q))
    assert abs(float(loss.detach()) - ref["loss"]) <= 1e-12 * ref["loss"]
    assert rel <= 1e-12
    # the taper is 0 at its first point: no gradient on a plane's first row and column
    assert (ref["grad"][:, :, 0, :] == 0).all() and (ref["grad"][:, :, :, 0] == 0).all()


@pytest.mark.parametrize("P,Q,H,W", PLANS)
def test_equal_fields_give_p_sqrt_eps_and_no_gradient(P, Q, H, W):
    _, t = fields(P, Q, H, W)
    for eps in (1e-12, 1e-6):
        ref = slo.loss_and_grad(t, t, P, Q, eps)
        assert abs(ref["loss"] - P * np.sqrt(eps)) <= 1e-14 * P * np.sqrt(eps)
        assert (ref["grad"] == 0).all()


def test_a_window_with_a_nan_is_skipped_per_plane():
    P, Q, H, W = 16, 12, 40, 56  # 3 x 5 windows
    p, t = fields(P, Q, H, W)
    full = slo.loss_and_grad(p, t, P, Q)
    assert full["nused"] == 30 and (full["counts"] == 15).all()
    t2 = t.copy()
    t2[0, 1, 13, 38] = np.nan  # windows 2, 3, 7, 8 of channel 1 only
    ref = slo.loss_and_grad(p, t2, P, Q)
    used = slo.used_jobs(p, t2, P, Q)
    assert list(np.flatnonzero(~used[0, 1])) == [2, 3, 7, 8] and used[0, 0].all()
    assert ref["nused"] == 26 and list(ref["counts"][0]) == [15, 11]
    assert ref["parts"][0, 0] == full["parts"][0, 0] and ref["parts"][0, 1] < full["parts"][0, 1]
    assert np.isfinite(ref["loss"]) and np.isfinite(ref["grad"]).all() and ref["grad"][0, 1, 13, 38] == 0
    p2 = p.copy()
    p2[0, 1, 13, 38] = np.inf  # in the prediction: the same jobs
    assert (slo.used_jobs(p2, t, P, Q) == used).all()
    # nothing used: 0, not NaN
    none = slo.loss_and_grad(p, np.full_like(t, np.nan), P, Q)
    assert none["loss"] == 0.0 and none["nused"] == 0 and (none["grad"] == 0).all()
    lt_, n_ = slo.loss_torch(torch.tensor(p), torch.full(p.shape, float("nan"), dtype=torch.float64), P, Q)
    assert float(lt_) == 0.0 and n_ == 0


@pytest.mark.parametrize("P,Q,H,W", PLANS + [(16, 16, 16, 16), (16, 12, 40, 56), (32, 32, 48, 40), (64, 32, 96, 80)])
def test_job_count_follows_the_overlap_plan(P, Q, H, W):
    wins = slo.windows(H, W, P, Q)
    ys, xs = oo.origins(H, P, Q), oo.origins(W, P, Q)
    assert len(wins) == len(ys) * len(xs)
    assert wins == [(y, x) for y in ys for x in xs]
    assert wins[-1] == (H - P, W - P) and wins[0] == (0, 0)
    p, t = fields(P, Q, H, W, N=2, C=1)
    assert slo.loss_and_grad(p, t, P, Q)["nused"] == 2 * len(wins)


@pytest.mark.parametrize("P,Q,H,W", PLANS)
def test_white_error_is_on_the_scale_of_the_rmse(P, Q, H, W):
    """A sanity band around the 0.886-0.889 measured in fp64, not a parity bar."""
    p, t = fields(P, Q, H, W, seed=1)
    ratio = slo.loss_and_grad(p, t, P, Q)["loss"] / np.sqrt(((p - t) ** 2).mean())
    print(f"plan {(P, Q, H, W)}: L_spec / RMSE = {ratio:.4f}")
    assert 0.85 <= ratio <= 0.92


def test_complex64_variant_is_close_and_not_identical():
    P, Q, H, W = 32, 32, 80, 72
    p, t = (v.astype(np.float32) for v in fields(P, Q, H, W))
    r64, r32 = slo.loss_and_grad(p, t, P, Q), slo.loss_and_grad(p, t, P, Q, dtype="complex64")
    e = np.linalg.norm(r32["grad"] - r64["grad"]) / np.linalg.norm(r64["grad"])
    assert 0 < e < 1e-5 and 0 < abs(r32["loss"] - r64["loss"]) / r64["loss"] < 1e-5
