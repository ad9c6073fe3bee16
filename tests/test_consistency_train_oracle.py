"""The oracle of training through the consistency correction
(tests/consistency_train_oracle.py) against consistency_oracle and against torch autograd,
the binding of the three adjoint entry points, and the argument validation.  No GPU."""
import numpy as np
import pytest
import torch

import consistency_oracle as co
import consistency_train_oracle as cto
from test_consistency_oracle import PAIRS, gpu_masks

SHAPES = [(1, 1), (1, 2), (2, 3), (3, 1), (5, 4), (6, 7)]
ADJOINT_SYMBOLS = ("srmi_consistency_adjoint_gather", "srmi_consistency_adjoint_iterate",
                   "srmi_consistency_adjoint_apply")
# every scale and mode pair the layer accepts (a bicubic D at scale 2 reads outside its block)
COMBOS = [(s, um, dm) for s in (2, 4, 6, 8) for um, dm in PAIRS if not (s == 2 and dm == "bicubic")]


def fields(rng, C, h, w, s, pattern):
    """(x [C, h s, w s] finite, lr [C, h, w] with NaN at the cells gpu_masks()[pattern] leaves
    inactive)."""
    x, lr = rng.randn(C, h * s, w * s), rng.randn(C, h, w)
    lr[:, ~gpu_masks(h, w)[pattern]] = np.nan
    return x, lr


def patterns(h, w):
    return ["full"] if h * w == 1 else ["full", "dry_corner", "one_wet", "all_dry", "hole"]


@pytest.mark.parametrize("s,um,dm", COMBOS)
def test_torch_layer_is_the_oracle_correction(s, um, dm):
    rng = np.random.RandomState(91)
    for h, w in SHAPES:
        for pattern in patterns(h, w):
            x, lr = fields(rng, 2, h, w, s, pattern)
            for K in (1, 2, 3, 16):
                got = cto.layer(torch.tensor(x)[None], torch.tensor(lr)[None], s, um, dm, K)[0].numpy()
                ref = co.correct(x, lr, s, um, dm, K)[0]
                assert np.max(np.abs(got - ref)) <= 1e-12, (h, w, pattern, K)
    # a NaN pixel under a finite LR cell: the cell goes inactive, the pixel passes through
    x, lr = fields(rng, 1, 5, 4, s, "full")
    x[0, 2 * s + s // 2, s + s // 2] = np.nan
    got = cto.layer(torch.tensor(x)[None], torch.tensor(lr)[None], s, um, dm, 3)[0].numpy()
    ref = co.correct(x, lr, s, um, dm, 3)[0]
    assert np.array_equal(np.isnan(got), np.isnan(x)) and np.nanmax(np.abs(got - ref)) <= 1e-12


@pytest.mark.parametrize("s,um,dm", COMBOS)
def test_numpy_adjoint_is_the_autograd_vjp(s, um, dm):
    rng = np.random.RandomState(92)
    worst = 0.0
    for h, w in SHAPES:
        for pattern in patterns(h, w):
            x, lr = fields(rng, 2, h, w, s, pattern)
            g = rng.randn(2, h * s, w * s)
            active = np.broadcast_to(gpu_masks(h, w)[pattern], lr.shape)
            for K in (1, 2, 3, 16):
                xt = torch.tensor(x)[None].requires_grad_(True)
                cto.layer(xt, torch.tensor(lr)[None], s, um, dm, K).backward(torch.tensor(g)[None])
                g0, q, Q, ts = cto.adjoint(g, active, s, um, dm, K)
                err = float(np.max(np.abs(g0 - xt.grad[0].numpy())))
                worst = max(worst, err)
                assert err <= 1e-12, (h, w, pattern, K, err)
                assert len(ts) == K + 1 and np.array_equal(ts[0], q)
    print(f"adjoint against autograd s={s} U={um} D={dm}: worst {worst:.2e}")


@pytest.mark.parametrize("um,dm", PAIRS)
def test_adjoint_is_the_transposed_dense_jacobian(um, dm):
    """... and the dense Jacobian is the oracle correction's own (by differences: the map is
    affine, so a unit step is exact up to rounding)."""
    rng = np.random.RandomState(93)
    s, (h, w), K = 4, (3, 2), 3
    active = gpu_masks(h, w)["dry_corner"]
    J = cto.jacobian_dense(active, s, um, dm, K)
    x, lr = rng.randn(h * s, w * s), rng.randn(h, w)
    lr[~active] = np.nan
    base = co.correct(x, lr, s, um, dm, K)[0]
    for j in rng.permutation(x.size)[:12]:
        e = np.zeros(x.size)
        e[j] = 1.0
        col = co.correct(x + e.reshape(x.shape), lr, s, um, dm, K)[0] - base
        assert np.max(np.abs(col.reshape(-1) - J[:, j])) <= 1e-12
    g = rng.randn(h * s, w * s)
    g0 = cto.adjoint(g, active, s, um, dm, K)[0]
    assert np.max(np.abs(g0.reshape(-1) - J.T @ g.reshape(-1))) <= 1e-12


def test_structural_facts_the_kernels_rely_on():
    """An HR pixel of block c has U taps only on cells within 2 of c (1 for bilinear), and
    G^T has bandwidth 2 per axis."""
    for s in (2, 4, 6, 8):
        for n in (1, 2, 3, 5, 9):
            for um, rad in (("bicubic", 2), ("bilinear", 1)):
                m = co.interp_matrix(n, n * s, 1.0 / s, um)
                for X in range(n * s):
                    js = np.flatnonzero(m[X])
                    assert np.all(np.abs(js - X // s) <= rad), (s, n, um, X)
                for dm in ("bilinear", "bicubic"):
                    if s == 2 and dm == "bicubic":
                        continue
                    G = co.du_stencil_matrix(n, co.du_coeffs(s, um, dm))
                    i, j = np.nonzero(G)
                    assert np.all(np.abs(i - j) <= 2)


def test_train_step_without_the_layer_is_the_spectral_oracle_step():
    import spectral_loss_oracle as slo
    from oracle import rcan_oracle as ro
    model = ro.RCANOracle(nchannels_in=1, nchannels_out=1, nlayers=1, nblocks=1, nfeatures=8, cbottleneck=2).double()
    ro.init_params_numpy(model, 3)
    hr = ro.synthetic_hr(2, 1, 32, 5)
    a = cto.train_step(model, hr, 4, "l2", K=0)
    b = slo.train_step(model, hr, 4, "l2")
    assert a[0] == b[0] and all(torch.equal(a[2][k], b[2][k]) for k in b[2])
    # with the layer the output coarse-grains back to the LR batch, and g0 is J^T g
    l2, out, grads, info = cto.train_step(model, hr, 4, "charbonnier", K=2)
    left = np.abs(co.D(out.numpy(), 4, "bicubic") - info["lr"])
    raw = np.abs(co.D(info["out0"], 4, "bicubic") - info["lr"])
    assert left.max() < 0.05 * raw.max()
    g0 = cto.adjoint(info["g"], np.ones_like(info["lr"], bool), 4, "bicubic", "bicubic", 2)[0]
    assert np.max(np.abs(g0 - info["g0"])) <= 1e-12 * max(1.0, np.abs(info["g"]).max())


def test_symbols_are_bound_and_declared():
    import os
    from srmi import _lib
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "srmi.h")).read()
    for name in ADJOINT_SYMBOLS:
        assert name in _lib.EXPORTED and hasattr(lib, name) and f"int {name}(" in header


def test_argument_validation():
    from srmi.engine import NetSpec
    from srmi.superres import check_consistent
    from srmi.trainer import FusedTrainer
    for bad in (-1, 17, 2.0, True, "2", None):
        with pytest.raises(ValueError):
            check_consistent(bad, 4, "bicubic", "bicubic")
    with pytest.raises(ValueError):
        check_consistent(1, 2, "bicubic", "bicubic")
    with pytest.raises(ValueError):
        check_consistent(1, 3, "bilinear", "bilinear")

    def spec(scale=4, cin=2, cout=2):
        return NetSpec(arch="rcan", nchannels_in=cin, nchannels_out=cout, nlayers=1, nblocks=1, scale=scale)
    cpu = torch.device("cpu")  # every refusal comes before anything is allocated
    with pytest.raises(ValueError, match="consistent"):
        FusedTrainer(spec(), 2, (16, 16), device=cpu, consistent=17)
    with pytest.raises(ValueError, match="consistent"):
        FusedTrainer(spec(scale=2), 2, (16, 16), device=cpu, consistent=1)
    with pytest.raises(ValueError, match="consistent"):
        FusedTrainer(spec(cout=1), 2, (16, 16), device=cpu, consistent=2, interp_loss=False,
                     task={"input_variables": {"a": 0, "b": 1}, "target_variables": ["a"]})
    with pytest.raises(ValueError):
        FusedTrainer(spec(cout=1), 2, (16, 16), device=cpu, consistent=2, interp_loss=False)
