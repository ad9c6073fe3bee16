"""The oracle of training on tiles with land (tests/land_train_oracle.py) against torch
itself, and the host-side refusals of the land mode.  No GPU."""
import numpy as np
import pytest
import torch

import land_oracle as lo
import land_train_oracle as lt
from oracle import rcan_oracle as ro


@pytest.mark.parametrize("T,scale", [(32, 4), (96, 2), (128, 4), (192, 4), (256, 8)])
def test_fixture_conditions(T, scale):
    """The shared fixture at the sizes the GPU tests use: tile 0 all wet, land in the
    others, every LR plane keeps a wet pixel, no wet plane constant."""
    hr = lt.land_batch(3, 2, T, 5)
    assert np.isfinite(hr[0]).all() and not np.isfinite(hr[1:]).all(axis=(1, 2, 3)).any()
    lt.check_conditions(hr, scale)
    frac = np.isfinite(hr).mean(axis=(1, 2, 3))
    assert (frac >= 0.4).all(), frac


@pytest.mark.parametrize("T,scale", [(32, 4), (96, 2), (64, 8)])
def test_lr_dry_rule_is_torch_nan_propagation(T, scale):
    hr = lt.land_batch(3, 2, T, 6)
    got = ~np.isfinite(ro.downsample(torch.tensor(hr, dtype=torch.float64), scale).numpy())
    assert (got == lt.lr_dry(~np.isfinite(hr), scale)).all()
    assert got.any() and not got.all()


@pytest.mark.parametrize("loss_fn", ["l2", "charbonnier"])
def test_masked_dy_is_autograd_of_the_masked_loss(loss_fn):
    rng = np.random.RandomState(7)
    t = lt.land_batch(3, 2, 32, 8).astype(np.float64)
    p = torch.tensor(rng.randn(*t.shape), requires_grad=True)
    loss, count = lt.masked_loss(p, torch.tensor(t), loss_fn)
    loss.backward()
    assert count == int(np.isfinite(t).sum())
    dy = lt.masked_dy(p.detach().numpy(), t, loss_fn)
    assert (dy[~np.isfinite(t)] == 0).all()
    np.testing.assert_allclose(dy, p.grad.numpy(), rtol=1e-12, atol=1e-18)


def test_masked_loss_without_land_is_the_plain_loss():
    rng = np.random.RandomState(9)
    p, t = torch.tensor(rng.randn(2, 2, 16, 16)), torch.tensor(rng.randn(2, 2, 16, 16))
    for fn in ("l2", "charbonnier"):
        assert float(lt.masked_loss(p, t, fn)[0]) == pytest.approx(float(ro.single_product_loss(p, t, fn)), rel=1e-14)


def test_keep_flags_threshold():
    region = lo.coast_region()
    bad, nwet = lt.keep_flags(region, 16, 16, 256)
    assert (bad[0] == bad[1]).all()
    assert (bad[0] == (nwet < 256).any(axis=0)).all()
    # min_wet = the whole plane and a shared mask: the reference's "one NaN drops the tile"
    both = np.stack([region[0], region[0]])
    bad2, _ = lt.keep_flags(both, 16, 16, 256)
    nonfinite = np.array([[not np.isfinite(both[c, (t // 3) * 16:(t // 3) * 16 + 16, (t % 3) * 16:(t % 3) * 16 + 16]).all()
                           for t in range(6)] for c in range(2)])
    assert (bad2.astype(bool) == nonfinite).all()
    assert lt.keep_flags(region, 16, 16, 1)[0].sum() < bad.sum()


def test_prep_statistics_over_the_wet_pixels():
    raw = lt.land_batch(3, 2, 32, 10).astype(np.float64) * 3 + 5
    hr, o, d, nwet = lt.prep(raw, lt.LNORM, 5)
    wet = np.isfinite(hr)
    assert (nwet == np.isfinite(raw).sum(axis=(2, 3))).all()
    assert (wet == lt.flip(np.isfinite(raw), 5)).all()
    for b in range(3):
        for c in range(2):
            w = hr[b, c][wet[b, c]]
            assert abs(w.mean()) < 1e-12 and abs(w.std() - 1) < 1e-12
    hr, o, d, _ = lt.prep(raw, lt.LSCALE, 0)
    assert np.nanmin(hr) == 0.0 and np.nanmax(hr) == 1.0


def test_land_refuses_data_downsample():
    from srmi.engine import NetSpec
    from srmi.trainer import FusedTrainer
    with pytest.raises(ValueError, match="data_downsample"):
        FusedTrainer(NetSpec(), 2, land=True, task={"data_downsample": 2}, device=torch.device("cpu"))


def test_prep_batch_land_refuses_tile_statistics():
    from srmi.batch import prep_batch
    raw = torch.zeros(2, 1, 8, 8)
    for norm in ("tnorm", "tscale"):
        with pytest.raises(ValueError, match="land=True"):
            prep_batch(raw, norm=norm, land=True)


def test_library_exports_the_land_training_symbols():
    from srmi import _lib
    lib = _lib.load()
    names = ("srmi_tiles_dry", "srmi_tiles_fill", "srmi_batch_prep_masked", "srmi_tile_loss_parts_masked",
             "srmi_loss_from_parts_masked", "srmi_loss_dy_masked")
    assert all(n in _lib.EXPORTED and hasattr(lib, n) for n in names)
    E, S = _lib.SRMI_ERR_ARG, -10002
    # argument checks come before any launch: no device needed
    assert lib.srmi_tiles_dry(None, 1, 16, 16, 16, 16, 1, None, None, None) == E
    assert lib.srmi_tiles_fill(None, 1, 161, 160, None, None) == S
    assert lib.srmi_tiles_fill(None, 1, 160, 160, None, None) == E
    assert lib.srmi_batch_prep_masked(None, 1, 1, 8, 0, 2, 7, None, None, None, None, None, None, None, None) == E
    assert lib.srmi_tile_loss_parts_masked(None, None, 1, 16, 0, 0.0, None, None, None) == E
    assert lib.srmi_loss_from_parts_masked(None, None, 1, 0, None, None) == E
    assert lib.srmi_loss_dy_masked(None, None, 16, 0, 0.0, None, None, None) == E
