"""Training through the consistency correction on the HIP path: srmi_consistency_adjoint_gather
/ _adjoint_iterate / _adjoint_apply against the fp64 oracle (tests/consistency_train_oracle.py),
srmi.consistency.ConsistencyLayer, FusedTrainer(consistent=K) and TiledInference(consistent=K).

Bars, derived, not measured, in test_gpu_consistency's form c * 2^-24 * M: M the sum of the
absolute values of the terms (from the oracle), c the roundings on the longest path a term
takes, each of a partial result no larger than M (u = 2^-24).

gather    q = sum_Y wy (sum_X wx g).  A term is multiplied (1) and then rides at most 5 s
          additions along x (the 5 s pixels of the 5 neighbouring blocks), is multiplied
          again (1) and rides at most 5 s additions along y: c = 10 s + 2, rounded up to
          C_GATH(s) = 10 s + 4, M = sum |wy wx g|.  The weights: each tap weight is
          evaluated in fp32 as in srmi_consistency_apply and differs from the exact one by
          at most 36 u (test_gpu_consistency's derivation); taps that clamp onto one cell
          are added (at most 3 additions of partial sums below 1.5: 4.5 u), so a folded
          weight is off by at most 41 u per tap folded into it and a product of two by 82 u
          per tap pair: 82 * u * T more, T = sum over the pixels of (tap pairs of the pixel
          on the cell) |g|.  Bilinear weights are exact; the same bar is used.
iterate   t' = v - sum_i wy_i (sum_j wx_j v_ij), v = M t, 5 taps per axis.  A transposed
          weight is the sum of up to 5 of the g (a field one cell wide folds all five):
          rounding of g (1) and 4 additions, per axis: 10; product (1) and 4 additions per
          axis: 10; the subtraction: 21.  C_ITA = 22, M = |v| + sum |wy_i wx_j v_ij|.
          Q' = Q + t is one rounding (C_ACC = 1, M = |Q| + |t|); with first = 1 a bit copy.
apply     g' = g - (k_y k_x) Q: the product of two taps is exact in fp32, its product with Q
          (1) and the subtraction (1): C_ADA = 3, M = |g| + |k_y k_x Q|.
composed  ``adjoint_bars``: the three composed in the max norm as
          test_gpu_consistency.composed_bars composes the forward's.
Every test prints max err / bar."""
import functools
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import consistency_oracle as co  # noqa: E402
import consistency_train_oracle as cto  # noqa: E402
import land_train_oracle as lt  # noqa: E402
import test_gpu_model  # noqa: E402
from oracle import rcan_oracle as ro  # noqa: E402
from srmi import _lib  # noqa: E402
from srmi._lib import SRMI_ERR_ARG, SRMI_ERR_SHAPE, call, ptr  # noqa: E402
from srmi.consistency import ConsistencyLayer  # noqa: E402
from srmi.engine import NetSpec, downsample, param_table  # noqa: E402
from srmi.inference import TiledInference  # noqa: E402
from srmi.superres import INTERP_MODES  # noqa: E402
from srmi.trainer import FusedTrainer  # noqa: E402
from test_consistency_oracle import PAIRS, gpu_masks  # noqa: E402
from test_gpu_consistency import C_ACC, C_RES, UU, composed_bars, report, t32  # noqa: E402
from test_gpu_inference import _small_rcan  # noqa: E402
from test_gpu_model import flat_from_model, rel_l2  # noqa: E402
from test_gpu_overlap import _field, bits, dev, f64, st  # noqa: E402
from test_gpu_spectral_loss import SPECTRAL, init_flat, rcan_spec  # noqa: E402

C_ITA, C_ADA, C_GW = 22.0, 3.0, 82.0
SHAPES = [(1, 1), (1, 2), (2, 3), (3, 1), (5, 5), (13, 21)]
SENT = 777.25


def c_gath(s):
    return 10.0 * s + 4.0


# --------------------------------------------------------------------- device wrappers
def gather_dev(g, s, umode):
    C, H, W = g.shape
    q = torch.full((C, H // s, W // s), SENT, dtype=torch.float32, device=g.device)
    call("srmi_consistency_adjoint_gather", ptr(g), C, H // s, W // s, s, INTERP_MODES[umode], ptr(q), st())
    return q


def aiterate_dev(t, act, s, umode, dmode, first, Q):
    C, h, w = t.shape
    out = torch.full((C, h, w), SENT, dtype=torch.float32, device=t.device)
    call("srmi_consistency_adjoint_iterate", ptr(t), ptr(act), C, h, w, s, INTERP_MODES[umode], INTERP_MODES[dmode],
         int(first), ptr(Q), ptr(out), st())
    return out


def aapply_dev(Q, act, g, s, dmode):
    C, h, w = Q.shape
    call("srmi_consistency_adjoint_apply", ptr(Q), ptr(act), C, h, w, s, INTERP_MODES[dmode], ptr(g), st())
    return g


def act_dev(active, d):
    return torch.tensor(np.ascontiguousarray(active).astype(np.int32), device=d)


# ------------------------------------------------------------------------------- bars
def tap_pairs(n, s, umode):
    """[n s, n]: the number of U's taps of HR index X that (clamped) read LR cell j."""
    m = np.zeros((n * s, n))
    for d in range(n * s):
        src = (d + 0.5) / s - 0.5
        if umode == "bilinear":
            i0 = min(int(np.floor(max(src, 0.0))), n - 1)
            taps = (i0, min(i0 + 1, n - 1))
        else:
            i0 = int(np.floor(src))
            taps = [min(max(i0 - 1 + k, 0), n - 1) for k in range(4)]
        for j in taps:
            m[d, j] += 1.0
    return m


def gather_bar(g, s, umode, factor=1.0):
    g = np.asarray(g, np.float64)
    h, w = g.shape[-2] // s, g.shape[-1] // s
    T = tap_pairs(h, s, umode).T @ np.abs(g) @ tap_pairs(w, s, umode)
    return factor * UU * (c_gath(s) * cto.abs_adjoint_gather(g, s, umode) + C_GW * T)


def aiterate_bar(t, active, s, um, dm):
    return C_ITA * UU * cto.abs_adjoint_iterate(t, active, s, um, dm)


def aapply_bar(g, Q, active, s, dm):
    return C_ADA * UU * cto.abs_adjoint_apply(g, Q, active, s, dm)


def adjoint_bars(g, active, s, um, dm, K, factor=1.0):
    """Max-norm bar of the device's J^T g against the oracle's, and the oracle's results: an
    error dt of t passes an iteration as at most L dt, L = 1 + (max column sum |G|)^2 >= ||I -
    G^T||_inf; Q collects every dt_k and a rounding of its own per step; D^T passes dQ as at
    most (max column sum |D|)^2 dQ."""
    g0, q, Q, ts = cto.adjoint(g, active, s, um, dm, K)
    h, w = q.shape[-2:]
    gc = np.abs(co.du_coeffs(s, um, dm))
    L = 1.0 + float(np.max(co.du_stencil_matrix(h, gc).sum(axis=0)) * np.max(co.du_stencil_matrix(w, gc).sum(axis=0)))
    dt, dQ, Qk = float(np.max(gather_bar(g, s, um, factor))), 0.0, np.zeros_like(q)
    for k in range(K):
        Qk = Qk + ts[k]
        dQ += dt + C_ACC * UU * float(np.max(np.abs(Qk)))
        dt = L * dt + float(np.max(aiterate_bar(ts[k], active, s, um, dm)))
    nd = float(np.max(np.abs(co.interp_matrix(h * s, h, float(s), dm)).sum(axis=0))) ** 2
    return float(np.max(aapply_bar(g, Q, active, s, dm))) + nd * dQ, (g0, q, Q, ts)


# ---------------------------------------------------------------- 1. per-kernel parity
@functools.lru_cache(maxsize=None)
def grad_field(C, h, w, s, seed):
    g = (np.random.RandomState(seed).randn(C, h * s, w * s) * 2 + 0.5).astype(np.float32)
    g.setflags(write=False)
    return g


# the benchmark's tile once, and a field wider than the 64 columns of one strip of the gather
@pytest.mark.parametrize("hw,s", [(hw, s) for s in (4, 8) for hw in SHAPES] + [((48, 48), 4), ((3, 70), 4)])
def test_gather_matches_the_oracle(hw, s):
    d, (h, w) = dev(), hw
    for C in ((1,) if h * w > 300 or w > 64 else (1, 2)):
        g = grad_field(C, h, w, s, 101)
        gd = torch.tensor(g, device=d)
        for um in ("bicubic", "bilinear"):
            q = f64(gather_dev(gd, s, um))
            report(f"gather {h}x{w} s={s} C={C} U={um}", np.abs(q - cto.adjoint_gather(g, s, um)),
                   gather_bar(g, s, um))
        assert torch.equal(bits(gd), bits(torch.tensor(g, device=d)))  # g is read only


@pytest.mark.parametrize("planes", [64, 150])
def test_gather_bands_of_several_rows(planes):
    """The gather shrinks its band of LR rows while the grid would hold fewer than 256
    workgroups, so few planes run bands of one row; 64 planes of 13 x 21 run bands of 4 rows
    (the last of 1), 150 planes bands of 8 (the last of 5)."""
    d, (h, w), s = dev(), (13, 21), 4
    g = grad_field(planes, h, w, s, 114)
    for um in ("bicubic", "bilinear"):
        q = f64(gather_dev(torch.tensor(g, device=d), s, um))
        report(f"gather {planes} planes U={um}", np.abs(q - cto.adjoint_gather(g, s, um)), gather_bar(g, s, um))


@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("s", [4, 8])
def test_adjoint_iterate_matches_the_oracle(hw, s):
    d, (h, w) = dev(), hw
    rng = np.random.RandomState(102)
    for C in (1, 2):
        active = rng.rand(C, h, w) >= 0.25
        t = rng.randn(C, h, w).astype(np.float32)  # not masked: q = U^T g is not
        Q0 = rng.randn(C, h, w).astype(np.float32)
        td, ad = t32(t, d), act_dev(active, d)
        for um, dm in PAIRS:
            what = f"{h}x{w} s={s} C={C} U={um} D={dm}"
            ref = cto.adjoint_iterate(t.astype(np.float64), active, s, um, dm)
            bar = aiterate_bar(t.astype(np.float64), active, s, um, dm)
            for first in (1, 0):
                Q = torch.full((C, h, w), SENT, dtype=torch.float32, device=d) if first else t32(Q0, d)
                out = f64(aiterate_dev(td, ad, s, um, dm, first, Q))
                report(f"adjoint iterate {what} first={first}", np.abs(out - ref), bar)
                if first:
                    assert torch.equal(bits(Q), bits(td)), what  # a bit copy
                else:
                    report(f"adjoint accumulate {what}", np.abs(f64(Q) - (Q0.astype(np.float64) + t)),
                           C_ACC * UU * (np.abs(Q0) + np.abs(t)))


@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("s", [4, 8])
def test_adjoint_apply_matches_the_oracle(hw, s):
    d, (h, w) = dev(), hw
    rng = np.random.RandomState(103)
    for C in (1, 2):
        active = rng.rand(C, h, w) >= 0.25
        g, Q = grad_field(C, h, w, s, 104), rng.randn(C, h, w).astype(np.float32)
        for dm in ("bicubic", "bilinear"):
            out = aapply_dev(t32(Q, d), act_dev(active, d), torch.tensor(g, device=d), s, dm)
            ref = cto.adjoint_apply(g, Q.astype(np.float64), active, s, dm)
            report(f"adjoint apply {h}x{w} s={s} C={C} D={dm}", np.abs(f64(out) - ref),
                   aapply_bar(g.astype(np.float64), Q.astype(np.float64), active, s, dm))
            # pixels at non-tap phases and the blocks of inactive cells: not a bit changes
            nt = 4 if dm == "bicubic" else 2
            a = s // 2 - nt // 2
            tap = np.zeros(s, bool)
            tap[a:a + nt] = True
            ty, tx = np.tile(tap, h), np.tile(tap, w)
            keep = ~(ty[:, None] & tx[None, :])[None] | ~np.repeat(np.repeat(active, s, 1), s, 2)
            assert keep.any() or s == 4
            assert np.array_equal(out.cpu().numpy().view(np.uint32)[keep], g.view(np.uint32)[keep]), (hw, s, dm)


@pytest.mark.parametrize("pattern", ["dry_corner", "one_wet", "all_dry", "hole"])
@pytest.mark.parametrize("s", [4, 8])
def test_mask_patterns_through_the_three_adjoint_kernels(pattern, s):
    """Gather, three iterations and the apply step against the oracle's, each kernel fed the
    device's own previous result; then the same with NaN written into t and Q at the
    inactive cells: an inactive cell contributes an exact zero, so no other bit changes."""
    d, (h, w), C = dev(), (13, 21), 2
    active = np.broadcast_to(gpu_masks(h, w)[pattern], (C, h, w)).copy()
    g = grad_field(C, h, w, s, 105)
    ad = act_dev(active, d)
    for um, dm in PAIRS:
        what = f"{pattern} s={s} U={um} D={dm}"
        t = gather_dev(torch.tensor(g, device=d), s, um)
        Q = torch.full((C, h, w), SENT, dtype=torch.float32, device=d)
        tn = t.clone()
        tn[torch.tensor(~active, device=d)] = float("nan")
        Qn = torch.full((C, h, w), SENT, dtype=torch.float32, device=d)
        for k in range(3):
            tin = f64(t)
            t_next = aiterate_dev(t, ad, s, um, dm, k == 0, Q)
            report(f"adjoint iterate {k} {what}", np.abs(f64(t_next) - cto.adjoint_iterate(tin, active, s, um, dm)),
                   aiterate_bar(tin, active, s, um, dm))
            tn_next = aiterate_dev(tn, ad, s, um, dm, k == 0, Qn)
            assert torch.equal(bits(tn_next), bits(t_next)), what  # finite: the NaNs were never read as values
            t = t_next
            tn = t_next.clone()
            tn[torch.tensor(~active, device=d)] = float("nan")
        Qh = f64(Q)
        out = aapply_dev(Q, ad, torch.tensor(g, device=d), s, dm)
        report(f"adjoint apply {what}", np.abs(f64(out) - cto.adjoint_apply(g, Qh, active, s, dm)),
               aapply_bar(g.astype(np.float64), Qh, active, s, dm))
        assert bool(torch.isnan(Qn[torch.tensor(~active, device=d)]).all()) or active.all()
        outn = aapply_dev(Qn, ad, torch.tensor(g, device=d), s, dm)
        assert torch.equal(bits(outn), bits(out)), what


# ------------------------------------------------- 2. scalar forms and the plane loop
def test_scalar_forms_misaligned_buffers_and_other_even_scales():
    """A gradient buffer that is not 16-byte aligned, and the even scales 2 (bilinear D) and
    6, take the scalar forms.  At s = 6 the source fraction itself is rounded: twice the
    gather bar, as test_gpu_consistency allows its apply step."""
    d, (h, w), C = dev(), (5, 7), 2
    rng = np.random.RandomState(106)
    for s, dmodes in ((4, ("bicubic", "bilinear")), (2, ("bilinear",)), (6, ("bicubic", "bilinear"))):
        buf = torch.zeros(C * h * s * w * s + 1, dtype=torch.float32, device=d)
        gd = buf[1:].view(C, h * s, w * s)
        assert gd.data_ptr() % 16 == 4
        g = grad_field(C, h, w, s, 107)
        active = rng.rand(C, h, w) >= 0.25
        for um in ("bicubic", "bilinear"):
            gd.copy_(torch.tensor(g, device=d))
            q = gather_dev(gd, s, um)
            report(f"gather scalar s={s} U={um}", np.abs(f64(q) - cto.adjoint_gather(g, s, um)),
                   gather_bar(g, s, um, 2.0))
            for dm in dmodes:
                Q = torch.empty_like(q)
                out = aiterate_dev(q, act_dev(active, d), s, um, dm, 1, Q)
                report(f"adjoint iterate s={s} U={um} D={dm}",
                       np.abs(f64(out) - cto.adjoint_iterate(f64(q), active, s, um, dm)),
                       aiterate_bar(f64(q), active, s, um, dm))
                gd.copy_(torch.tensor(g, device=d))
                aapply_dev(Q, act_dev(active, d), gd, s, dm)
                report(f"adjoint apply scalar s={s} D={dm}",
                       np.abs(f64(gd) - cto.adjoint_apply(g, f64(Q), active, s, dm)),
                       aapply_bar(g.astype(np.float64), f64(Q), active, s, dm))
        assert float(buf[0]) == 0.0


def test_more_planes_than_a_grid_holds():
    """65 537 planes of LR 1 x 1 at s = 4: the blockIdx.y loop of all three kernels."""
    d, NC, s = dev(), 65537, 4
    rng = np.random.RandomState(108)
    g = (rng.randn(NC, s, s)).astype(np.float32)
    active = rng.rand(NC, 1, 1) >= 0.25
    q = gather_dev(torch.tensor(g, device=d), s, "bicubic")
    report("gather 65537 planes", np.abs(f64(q) - cto.adjoint_gather(g, s, "bicubic")), gather_bar(g, s, "bicubic"))
    Q = torch.empty_like(q)
    out = aiterate_dev(q, act_dev(active, d), s, "bicubic", "bicubic", 1, Q)
    report("adjoint iterate 65537 planes", np.abs(f64(out) - cto.adjoint_iterate(f64(q), active, s, "bicubic", "bicubic")),
           aiterate_bar(f64(q), active, s, "bicubic", "bicubic"))
    assert torch.equal(bits(Q), bits(q))
    gd = aapply_dev(Q, act_dev(active, d), torch.tensor(g, device=d), s, "bicubic")
    report("adjoint apply 65537 planes", np.abs(f64(gd) - cto.adjoint_apply(g, f64(Q), active, s, "bicubic")),
           aapply_bar(g.astype(np.float64), f64(Q), active, s, "bicubic"))


# ------------------------------------------------------------- 3. the adjoint identity
@pytest.mark.parametrize("K", [1, 3, 16])
@pytest.mark.parametrize("s", [4, 8])
def test_adjoint_identity_on_the_device(K, s):
    """<forward(x), g> = <x, backward(g)> with lr = 0 (the layer is then linear in x), summed
    in fp64 on the host, independent of the oracle's adjoint.  The device's forward is
    within b_x of the exact J x and its backward within b_g of the exact J^T g, per element
    (composed_bars, adjoint_bars), and <J x, g> = <x, J^T g> exactly, so the two sums differ
    by at most b_x sum |g| + b_g sum |x|."""
    d, (h, w), C = dev(), (13, 21), 2
    rng = np.random.RandomState(109)
    x = (rng.randn(C, h * s, w * s) * 2 + 0.5).astype(np.float32)
    g = grad_field(C, h, w, s, 110)
    lr = np.zeros((C, h, w), np.float32)
    for um, dm in PAIRS:
        layer = ConsistencyLayer((1, C, h, w), s, um, dm, K, device=d)
        fx = f64(layer.forward_(torch.tensor(x, device=d)[None], torch.tensor(lr, device=d)[None]))[0]
        bg = f64(layer.backward_(torch.tensor(g, device=d)[None]))[0]
        (_, _, bx), _ = composed_bars(x.astype(np.float64), lr.astype(np.float64), s, um, dm, K)
        b_g, _ = adjoint_bars(g.astype(np.float64), np.ones((C, h, w), bool), s, um, dm, K)
        lhs, rhs = float(np.sum(fx * g.astype(np.float64))), float(np.sum(x.astype(np.float64) * bg))
        bar = bx * float(np.abs(g).sum()) + b_g * float(np.abs(x).sum())
        print(f"adjoint identity K={K} s={s} U={um} D={dm}: |lhs - rhs| {abs(lhs - rhs):.3e} / bar {bar:.3e} = "
              f"{abs(lhs - rhs) / bar:.3f}; lhs {lhs:.6e}")
        assert abs(lhs - rhs) <= bar
        if K == 1:  # J is far from the identity (at larger K the composed bar grows like L^K)
            assert abs(lhs - float(np.sum(x.astype(np.float64) * g))) > 10 * bar


def test_layer_backward_matches_the_oracle_end_to_end():
    """ConsistencyLayer.backward_ against the oracle's J^T g within adjoint_bars, with NaN in
    lr (inactive cells), rows > 0 of the workspace, and forward_'s result within
    composed_bars."""
    d, (h, w), C, s, K = dev(), (13, 21), 2, 4, 3
    rng = np.random.RandomState(111)
    x = (rng.randn(2, C, h * s, w * s)).astype(np.float32)
    lr = rng.randn(2, C, h, w).astype(np.float32)
    lr[:, :, ~gpu_masks(h, w)["hole"]] = np.nan
    lr[1, 0, 0, 0] = np.nan
    g = rng.randn(2, C, h * s, w * s).astype(np.float32)
    for um, dm in PAIRS:
        layer = ConsistencyLayer((3, C, h, w), s, um, dm, K, device=d)
        xd, gd = torch.tensor(x, device=d), torch.tensor(g, device=d)
        layer.forward_(xd, torch.tensor(lr, device=d), rows=1)
        assert float(layer.active[0].sum()) == 0 and np.array_equal(layer.active[1:].cpu().numpy() != 0, np.isfinite(lr))
        layer.backward_(gd, rows=1)
        for n in range(2):
            (_, _, bx), (xk, _, _, active) = composed_bars(x[n].astype(np.float64), lr[n].astype(np.float64), s, um,
                                                           dm, K)
            b_g, (g0, _, Q, _) = adjoint_bars(g[n].astype(np.float64), active, s, um, dm, K)
            ex, eg = float(np.max(np.abs(f64(xd[n]) - xk))), float(np.max(np.abs(f64(gd[n]) - g0)))
            print(f"layer U={um} D={dm} tile {n}: forward {ex / bx:.3f} of its bar, backward {eg / b_g:.3f} of its bar")
            assert ex <= bx and eg <= b_g
            assert float(np.max(np.abs(g0 - g[n]))) > 100 * b_g  # the adjoint does something


# ----------------------------------------------------------- 4. refusals launch nothing
def test_symbols_and_refusals():
    lib, d = _lib.load(), dev()
    for name in ("srmi_consistency_adjoint_gather", "srmi_consistency_adjoint_iterate",
                 "srmi_consistency_adjoint_apply"):
        assert name in _lib.EXPORTED and hasattr(lib, name)
    C, h, w, s = 1, 3, 4, 4
    x = torch.full((C, h * s, w * s), SENT, dtype=torch.float32, device=d)
    a, b, c = (torch.full((C, h, w), SENT, dtype=torch.float32, device=d) for _ in range(3))
    act = torch.full((C, h, w), 1, dtype=torch.int32, device=d)
    ga, it, ap = (lib.srmi_consistency_adjoint_gather, lib.srmi_consistency_adjoint_iterate,
                  lib.srmi_consistency_adjoint_apply)
    S = st()
    assert ga(None, C, h, w, s, 2, ptr(a), S) == SRMI_ERR_ARG
    assert ga(ptr(x), C, h, w, s, 2, None, S) == SRMI_ERR_ARG
    assert ga(ptr(x), C, h, w, s, 3, ptr(a), S) == SRMI_ERR_ARG
    assert ga(ptr(x), C, h, w, 5, 2, ptr(a), S) == SRMI_ERR_SHAPE  # an odd scale
    assert ga(ptr(x), 0, h, w, s, 2, ptr(a), S) == SRMI_ERR_SHAPE
    assert ga(ptr(x), C, 1 << 14, 1 << 14, s, 2, ptr(a), S) == SRMI_ERR_SHAPE  # a plane of 2^32
    assert it(ptr(a), ptr(act), C, h, w, s, 2, 2, 1, ptr(b), ptr(a), S) == SRMI_ERR_ARG  # t_out is t
    assert it(ptr(a), ptr(act), C, h, w, s, 2, 2, 1, ptr(b), ptr(b), S) == SRMI_ERR_ARG  # t_out is Q
    assert it(ptr(a), ptr(act), C, h, w, s, 2, 2, 1, ptr(a), ptr(c), S) == SRMI_ERR_ARG  # Q is t
    assert it(ptr(a), None, C, h, w, s, 2, 2, 1, ptr(b), ptr(c), S) == SRMI_ERR_ARG
    assert it(None, ptr(act), C, h, w, s, 2, 2, 1, ptr(b), ptr(c), S) == SRMI_ERR_ARG
    assert it(ptr(a), ptr(act), C, h, w, s, 0, 2, 1, ptr(b), ptr(c), S) == SRMI_ERR_ARG
    assert it(ptr(a), ptr(act), C, h, w, s, 2, 4, 1, ptr(b), ptr(c), S) == SRMI_ERR_ARG
    assert it(ptr(a), ptr(act), C, h, w, 3, 2, 2, 1, ptr(b), ptr(c), S) == SRMI_ERR_SHAPE
    assert it(ptr(a), ptr(act), C, h, w, 2, 2, 2, 1, ptr(b), ptr(c), S) == SRMI_ERR_SHAPE  # bicubic D at s = 2
    assert it(ptr(a), ptr(act), C, h, 0, s, 2, 2, 1, ptr(b), ptr(c), S) == SRMI_ERR_SHAPE
    assert ap(None, ptr(act), C, h, w, s, 2, ptr(x), S) == SRMI_ERR_ARG
    assert ap(ptr(a), None, C, h, w, s, 2, ptr(x), S) == SRMI_ERR_ARG
    assert ap(ptr(a), ptr(act), C, h, w, s, 2, None, S) == SRMI_ERR_ARG
    assert ap(ptr(a), ptr(act), C, h, w, s, 4, ptr(x), S) == SRMI_ERR_ARG
    assert ap(ptr(a), ptr(act), C, h, w, 7, 2, ptr(x), S) == SRMI_ERR_SHAPE
    assert ap(ptr(a), ptr(act), C, h, w, 2, 2, ptr(x), S) == SRMI_ERR_SHAPE  # bicubic D at s = 2
    assert ap(ptr(a), ptr(act), C, -1, w, s, 2, ptr(x), S) == SRMI_ERR_SHAPE
    torch.cuda.synchronize()
    for t in (x, a, b, c):  # nothing was enqueued
        assert bool((t == SENT).all())
    for K, scale, um, dm in ((0, 4, "bicubic", "bicubic"), (17, 4, "bicubic", "bicubic"), (1, 2, "bicubic", "bicubic"),
                             (1, 4, "nearest", "bicubic"), (1, 5, "bilinear", "bilinear")):
        with pytest.raises(ValueError):
            ConsistencyLayer((1, 1, 4, 4), scale, um, dm, K, device=d)


# ---------------------------------------------------------- 5. determinism and capture
def test_two_runs_are_bit_identical_and_the_six_launches_replay_in_a_graph():
    d, (h, w), C, s, K = dev(), (13, 21), 2, 4, 3

    def inputs(seed):
        r = np.random.RandomState(seed)
        lr = r.randn(2, C, h, w).astype(np.float32)
        lr[0, 1, 2, 3] = np.nan
        return (torch.tensor(r.randn(2, C, h * s, w * s).astype(np.float32), device=d), torch.tensor(lr, device=d),
                torch.tensor(r.randn(2, C, h * s, w * s).astype(np.float32), device=d))
    layer = ConsistencyLayer((2, C, h, w), s, "bicubic", "bicubic", K, device=d)

    def eager(seed):
        x, lr, g = inputs(seed)
        layer.forward_(x, lr)
        layer.backward_(g)
        torch.cuda.synchronize()
        return x.clone(), g.clone()
    a, b = eager(1), eager(1)
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))
    x, lr, g = inputs(1)

    def stage():
        layer.forward_(x, lr)
        layer.backward_(g)
    stage()  # warm-up outside capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(device=d)
    side.wait_stream(torch.cuda.current_stream(d))
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            stage()
    torch.cuda.current_stream(d).wait_stream(side)
    for t, v in zip((x, lr, g), inputs(2)):
        t.copy_(v)
    graph.replay()
    torch.cuda.synchronize()
    ex, eg = eager(2)
    assert torch.equal(bits(x), bits(ex)) and torch.equal(bits(g), bits(eg))
    assert not torch.equal(bits(ex), bits(a[0]))


# ------------------------------------------------------------- 6. trainer, consistent=0
@pytest.mark.parametrize("loss_fn", ["l2", "charbonnier"])
@pytest.mark.parametrize("B,micro", [(2, 1), (4, 2)])
def test_consistent_zero_trainer_is_the_trainer_as_it_was(B, micro, loss_fn):
    spec = rcan_spec(1, 2)
    flat = init_flat(spec, 5)
    hr = torch.tensor(ro.synthetic_hr(B, 2, 192, 19), device=dev())
    res = []
    for kw in ({}, dict(consistent=0)):
        tr = FusedTrainer(spec, B, (48, 48), device=dev(), params=flat, micro=micro, loss_fn=loss_fn, **kw)
        assert tr.micro == micro and tr.layer is None and (tr.dy is None) == (loss_fn == "l2")
        rows = []
        for _ in range(2):
            out = tr.step(hr)
            torch.cuda.synchronize()
            assert set(out) == {"loss", "interp_loss"}
            rows.append((out["loss"].clone(), out["interp_loss"].clone(), tr.sr.clone(), tr.grads.clone(),
                         tr.params.clone()))
        res.append(rows)
        del tr
    for k, (a, b) in enumerate(zip(*res)):
        for x, y, what in zip(a, b, ("loss", "interp_loss", "sr", "grads", "params")):
            assert torch.equal(bits(x), bits(y)), (k, what)
    assert np.isfinite(float(res[0][1][0]))


# ------------------------------------------------------------ 7. trainer against fp64
K2 = 2


def consistent_drift_bounds(monkeypatch, model, hr, scale, loss_fn, land, spectral, g_ref):
    """test_gpu_model.drift_bounds itself with the oracle step it runs the bf16 emulation
    through replaced by the constrained one, as test_gpu_spectral_loss.spectral_drift_bounds
    does."""
    monkeypatch.setattr(test_gpu_model, "oracle_grads",
                        lambda m, h, s: cto.train_step(m, h, s, loss_fn, K2, land=land, spectral=spectral)[:3])
    return test_gpu_model.drift_bounds(model, hr, scale, g_ref)


def coarse_check(tr, info, what):
    """rms(D(tr.sr) - lr) over the active cells below the oracle's own ||E^K r0|| (E^K in fp64
    on the r0 the device's layer kept) plus the composed forward bar: the residual bar of a
    field of the output's magnitude (D in fp32), the bar of r_K, and the bar of x_K passed
    through D.  The magnitudes in the bars are the oracle's (they only scale u)."""
    s, um, dm = 4, "bicubic", "bicubic"
    lr = info["lr"]
    active = tr.layer.active.cpu().numpy() != 0
    assert np.array_equal(active, np.isfinite(lr)), what
    r0 = f64(tr.layer.r0)
    rk = r0
    for _ in range(K2):
        rk = co.iterate(rk, active, s, um, dm)
    bK = bx = 0.0
    for n in range(lr.shape[0]):
        (_, bKn, bxn), _ = composed_bars(info["out0"][n], lr[n], s, um, dm, K2)
        bK, bx = max(bK, bKn), max(bx, bxn)
    sr = f64(tr.sr)
    nd = float(np.max(np.sum(np.abs(co.interp_matrix(8 * s, 8, float(s), dm)), axis=1))) ** 2
    bres = C_RES * UU * float(np.max((np.abs(np.nan_to_num(lr)) + co.abs_D(sr, s, dm))[active]))
    left = (f64(downsample(tr.sr, s, mode=dm)) - np.nan_to_num(lr))[active]
    rms, bar = float(np.sqrt(np.mean(left ** 2))), float(np.sqrt(np.mean(rk[active] ** 2))) + bres + bK + nd * bx
    raw = float(np.sqrt(np.mean(r0[active] ** 2)))
    print(f"{what}: rms(D(sr) - lr) raw {raw:.3e}, after {K2} steps {rms:.3e} <= bar {bar:.3e}")
    assert rms <= bar and raw > 20 * bar  # the raw network is far from consistent: the test can fail


def check_grads(table, g, g_ref, bound, info, what):
    """Every gradient tensor within bound[name] rel-L2 of the oracle's -- but for a tensor whose
    exact gradient is identically zero, where a relative distance is not defined.  With every
    cell active that is the last conv's bias: the rows of G sum to 1, so E 1 = 0, P 1 = 1, and
    U 1 = D 1 = 1 give J 1 = 0 -- a constant added to the network's output is removed by the
    layer -- and d loss / d bias = <1, J^T g> = <J 1, g> = 0 (the oracle's is rounding, below
    1e-9 of sum |g0|).  The device forms it as the sum of dy; it is held to the same figure
    relative to the sum of the absolute terms instead, 1e-3 sum |g0| (the fixed part of
    drift_bounds and the fp32 engine's bar).  Returns the names so exempted."""
    scale = float(np.abs(info["g0"]).sum())
    exempt = []
    for name, off, n, shape in table:
        got, ref = g[off:off + n].view(shape), g_ref[name]
        if float(ref.abs().max()) <= 1e-9 * scale:
            exempt.append(name)
            r = float(got.abs().max()) / scale
            print(f"{what}: {name} has a zero exact gradient; |device| / sum |g0| = {r:.2e} (bar 1e-3)")
            assert r <= 1e-3, (name, r)
            continue
        r = rel_l2(got, ref)
        assert r <= bound[name], (name, r, bound[name])
    return exempt


def step_vs_oracle(monkeypatch, hr, loss_fn, land, spectral=None):
    d = dev()
    model = ro.RCANOracle(nchannels_in=2, nchannels_out=2, nlayers=2, nblocks=2, nfeatures=64, cbottleneck=2)
    ro.init_params_numpy(model, 22)
    spec = rcan_spec(2, 2)
    table = param_table(spec)
    flat = flat_from_model(model, table).to(d)
    model = model.double()
    l_ref, out_ref, g_ref, info = cto.train_step(model, hr, 4, loss_fn, K2, land=land, spectral=spectral)
    bound = consistent_drift_bounds(monkeypatch, model, hr, 4, loss_fn, land, spectral, g_ref)
    tr = FusedTrainer(spec, 3, (48, 48), device=d, params=flat, loss_fn=loss_fn, land=land, spectral=spectral,
                      consistent=K2)
    out = tr.step(torch.tensor(hr, device=d))
    torch.cuda.synchronize()
    keys = [("loss", l_ref)] + ([("pixel_loss", info["pixel_loss"]), ("spectral_loss", info["spectral_loss"])]
                                if spectral is not None else [])
    for key, ref in keys:
        got = float(out[key])
        print(f"{loss_fn} land={land} spectral={spectral is not None}: {key} {got:.6f} oracle {ref:.6f} "
              f"rel {abs(got - ref) / ref:.2e} (bar 2e-3)")
        assert abs(got - ref) / ref < 2e-3, key
    exempt = check_grads(table, tr.grads.cpu(), g_ref, bound, info, f"{loss_fn} land={land}")
    assert exempt == ([] if land else ["tail.1.bias"])  # on a coast some cells are inactive: J 1 != 0
    coarse_check(tr, info, f"{loss_fn} land={land}")
    # the layer changes the step: the unconstrained oracle's loss is elsewhere
    l_free = cto.train_step(model, hr, 4, loss_fn, 0, land=land, spectral=spectral)[0]
    assert abs(l_free - l_ref) / l_ref > 2e-2
    return tr, info


@pytest.mark.parametrize("loss_fn", ["l2", "charbonnier"])
def test_consistent_trainer_step_vs_oracle(loss_fn, monkeypatch):
    """test_land_trainer_step_vs_masked_oracle's bars: the loss 2e-3 relative, every gradient
    tensor within test_gpu_model.drift_bounds."""
    step_vs_oracle(monkeypatch, ro.synthetic_hr(3, 2, 192, 21), loss_fn, False)


@pytest.mark.parametrize("loss_fn", ["l2", "charbonnier"])
def test_consistent_land_trainer_step_vs_oracle(loss_fn, monkeypatch):
    hr = lt.land_batch(3, 2, 192, 21)
    lt.check_conditions(hr, 4)
    tr, info = step_vs_oracle(monkeypatch, hr, loss_fn, True)
    assert 0 < (~np.isfinite(info["lr"])).sum() < info["lr"].size
    dy = tr.dy.cpu().numpy()
    # +0.0f on land before the adjoint, and the adjoint touches the blocks of active cells
    # only, whose 4 x 4 children are all wet at s = 4: still +0.0f
    assert (dy[~np.isfinite(hr)].view(np.int32) == 0).all()
    r = rel_l2(dy, info["g0"])
    print(f"land {loss_fn}: dy after the adjoint against the oracle's g0, rel-L2 {r:.2e} (bar 2e-2, the bf16 "
          "model output's)")
    assert r < 2e-2 and rel_l2(info["g"], info["g0"]) > 0.2


def test_consistent_spectral_trainer_step_vs_oracle(monkeypatch):
    step_vs_oracle(monkeypatch, ro.synthetic_hr(3, 2, 192, 21), "l2", False, SPECTRAL)


def test_consistent_trainer_fp32_step_vs_oracle():
    """The exact-fp32 engine at test_gpu_fp32's bars: the loss and the output 1e-5 relative,
    every gradient tensor 1e-3 rel-L2; dy after the adjoint, the seed those gradients are
    linear in, against the oracle's g0 at that 1e-3."""
    d = dev()
    model = ro.RCANOracle(nchannels_in=2, nchannels_out=2, nlayers=2, nblocks=2, nfeatures=64, cbottleneck=2)
    ro.init_params_numpy(model, 23)
    spec = rcan_spec(2, 2, dtype="fp32")
    table = param_table(spec)
    hr = ro.synthetic_hr(3, 2, 192, 21)
    tr = FusedTrainer(spec, 3, (48, 48), device=d, params=flat_from_model(model, table).to(d), consistent=K2)
    l_ref, out_ref, g_ref, info = cto.train_step(model.double(), hr, 4, "l2", K2)
    out = tr.step(torch.tensor(hr, device=d))
    torch.cuda.synchronize()
    print(f"fp32: loss {float(out['loss']):.8f} oracle {l_ref:.8f} rel {abs(float(out['loss']) - l_ref) / l_ref:.2e}")
    assert abs(float(out["loss"]) - l_ref) / l_ref < 1e-5
    assert rel_l2(tr.sr, out_ref) < 1e-5
    exempt = check_grads(table, tr.grads.cpu(), g_ref, {name: 1e-3 for name in g_ref}, info, "fp32")
    assert exempt == ["tail.1.bias"]
    rdy = rel_l2(tr.dy, info["g0"])
    print(f"fp32 engine with the layer: dy rel-L2 {rdy:.2e} (bar 1e-3)")
    assert rdy < 1e-3
    coarse_check(tr, info, "fp32")


# ---------------------------------------------------- 8. micro-batch and rank split
def test_consistent_micro_batch_split():
    """test_spectral_micro_batch_split's bars: the losses bit-identical, the gradients to 1e-5
    rel-L2; every micro-batch works in its own rows of the layer's workspace."""
    spec = rcan_spec(1, 2)
    flat = init_flat(spec, 5)
    hr = torch.tensor(lt.land_batch(4, 2, 192, 24), device=dev())
    res = []
    for micro in (1, 2):
        tr = FusedTrainer(spec, 4, (48, 48), device=dev(), params=flat, micro=micro, land=True, spectral=SPECTRAL,
                          consistent=K2)
        out = tr.step(hr)
        torch.cuda.synchronize()
        res.append(([float(out[k]) for k in ("loss", "pixel_loss", "spectral_loss")], tr.grads.clone(),
                    tr.layer.r0.clone()))
        del tr
    (l1, g1, r1), (l2, g2, r2) = res
    assert l1 == l2 and all(np.isfinite(l1)) and l1[2] > 0
    assert rel_l2(g2, g1) < 1e-5
    assert torch.equal(bits(r1), bits(r2))


def _dp_worker(rank, port, q):
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(root, "super-resolution-climate_amd"), root, os.path.join(root, "tests")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK="0")
    import torch.distributed as dist
    from srmi.dist import init_from_env, shard_range
    info = init_from_env("gloo")
    d = torch.device("cuda", 0)
    torch.cuda.set_device(d)
    spec = rcan_spec(1, 2)
    flat = init_flat(spec, 5)
    hr_all = torch.tensor(lt.land_batch(4, 2, 192, 25), device=d)
    a, b = shard_range(4, info)
    tr = FusedTrainer(spec, b - a, (48, 48), device=d, params=flat, micro=2, info=info, land=True, consistent=K2)
    out = tr.step(hr_all[a:b].contiguous())
    torch.cuda.synchronize()
    q.put((rank, [float(out[k]) for k in ("loss", "interp_loss")], tr.grads.cpu().numpy(), tr.params.cpu().numpy()))
    dist.destroy_process_group()


def test_consistent_dp_world2_matches_single_process():
    """test_spectral_dp_world2_matches_single_process's conventions and bars (gloo, both ranks
    on cuda:0, the staged data-parallel backward; gradients 2e-4 rel-L2)."""
    import multiprocessing as mp
    hr_np = lt.land_batch(4, 2, 192, 25)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 47000 + random.randint(0, 2000)
    ps = [ctx.Process(target=_dp_worker, args=(r, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = sorted([q.get(timeout=100) for _ in ps], key=lambda t: t[0])
    for p in ps:
        p.join(timeout=30)
        assert p.exitcode == 0
    d = dev()
    spec = rcan_spec(1, 2)
    tr = FusedTrainer(spec, 4, (48, 48), device=d, params=init_flat(spec, 5), micro=1, land=True, consistent=K2)
    out = tr.step(torch.tensor(hr_np, device=d))
    torch.cuda.synchronize()
    losses, g = [float(out[k]) for k in ("loss", "interp_loss")], tr.grads.cpu().numpy()
    for rank, l_r, g_r, p_r in res:
        assert l_r == losses, (rank, l_r, losses)
        assert np.linalg.norm(g_r - g) / np.linalg.norm(g) < 2e-4
    np.testing.assert_array_equal(res[0][3], res[1][3])  # replicas stay identical after Adam


# ------------------------------------------------------------------ 9. TiledInference
K3 = 3
_TI = {}


def ti_case():
    """The consistent=0 and consistent=3 runs the inference checks share (made once)."""
    if not _TI:
        d = dev()
        spec, model, flat = _small_rcan()
        region = torch.tensor(_field(np.random.RandomState(113), 1, 2 * 192 + 17, 3 * 192 + 9), device=d)
        _TI.update(spec=spec, flat=flat.to(d), region=region)
        t0 = TiledInference(spec, _TI["flat"], region.shape, (192, 192), device=d, graph=False, consistent=0)
        im0, l0 = t0.process_region(region)
        _TI.update(sr0=t0.sr.clone(), lr0=t0.lr.clone(), tiles=t0.tiles.clone(), im0={k: v.clone() for k, v in im0.items()},
                   l0={k: v.clone() for k, v in l0.items()})
        t3 = TiledInference(spec, _TI["flat"], region.shape, (192, 192), device=d, graph=False, consistent=K3)
        im3, l3 = t3.process_region(region)
        _TI.update(sr3=t3.sr.clone(), im3={k: v.clone() for k, v in im3.items()}, l3={k: v.clone() for k, v in l3.items()})
    return _TI


def test_tiled_inference_consistent_zero_is_the_object_as_it_was():
    e = ti_case()
    t = TiledInference(e["spec"], e["flat"], e["region"].shape, (192, 192), device=dev(), graph=False)
    im, lo = t.process_region(e["region"])
    assert t.layer is None
    for k in im:
        assert torch.equal(bits(im[k]), bits(e["im0"][k])), k
    for k in lo:
        assert torch.equal(bits(lo[k]), bits(e["l0"][k])), k
    assert torch.equal(bits(t.sr), bits(e["sr0"]))


def test_tiled_inference_corrects_every_tile_and_scores_the_corrected_tiles():
    e = ti_case()
    n = e["sr0"].shape[0]
    assert n == 6
    worst = 0.0
    for t in range(n):
        x0, lr = f64(e["sr0"][t]), f64(e["lr0"][t])
        (_, _, bx), (xk, _, _, active) = composed_bars(x0, lr, 4, "bicubic", "bicubic", K3)
        assert active.all()
        err = float(np.max(np.abs(f64(e["sr3"][t]) - xk)))
        worst = max(worst, err / bx)
        assert err <= bx, t
    print(f"TiledInference(consistent={K3}): worst tile max err / bar = {worst:.3f}")
    # the reported loss is the loss of those corrected tiles (one batch of 6 <= 36 tiles: RMSE)
    ref = float(np.sqrt(np.mean((f64(e["sr3"]) - f64(e["tiles"])) ** 2)))
    got = float(e["l3"]["model"])
    assert abs(got - ref) <= 1e-5 * ref and abs(got - float(e["l0"]["model"])) > 1e-3 * ref
    assert torch.equal(bits(e["l3"]["interpolated"]), bits(e["l0"]["interpolated"]))
    for k in ("input", "target", "interpolated"):
        assert torch.equal(bits(e["im3"][k]), bits(e["im0"][k])), k
    assert not torch.equal(bits(e["im3"]["model"]), bits(e["im0"]["model"]))


def test_tiled_inference_consistent_graph_and_compacted_paths():
    e = ti_case()
    d = dev()
    tg = TiledInference(e["spec"], e["flat"], e["region"].shape, (192, 192), device=d, graph=True, consistent=K3)
    for _ in range(2):  # the capture's warm-up and first replay, then a second replay
        im, lo = tg.process_region(e["region"])
        assert torch.equal(bits(tg.sr), bits(e["sr3"])) and torch.equal(bits(lo["model"]), bits(e["l3"]["model"]))
        assert torch.equal(bits(im["model"]), bits(e["im3"]["model"]))
    # one tile made non-finite: the compacted path; the kept tiles' results do not change
    region = e["region"].clone()
    region[0, 200, 10] = float("nan")  # tile (1, 0) -> id 3
    im, lo = tg.process_region(region)
    assert tg.n_kept == 5
    keep = [0, 1, 2, 4, 5]
    assert torch.equal(bits(tg.sr[:5]), bits(e["sr3"][keep]))
    assert bool(torch.isnan(im["model"][0, 192:384, :192]).all()) and np.isfinite(float(lo["model"]))


# ---------------------------------------------------------------- 10. trainer refusals
def test_trainer_refusals_come_before_any_allocation():
    d = dev()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(d)

    def spec(scale=4, cout=2):
        return NetSpec(arch="rcan", nchannels_in=2, nchannels_out=cout, nfeatures=64, nlayers=1, nblocks=1,
                       cbottleneck=2, scale=scale)
    with pytest.raises(ValueError, match="consistent"):
        FusedTrainer(spec(), 2, (48, 48), device=d, consistent=17)
    with pytest.raises(ValueError, match="consistent"):
        FusedTrainer(spec(scale=2), 2, (48, 48), device=d, consistent=1)
    with pytest.raises(ValueError, match="consistent"):
        FusedTrainer(spec(cout=1), 2, (48, 48), device=d, consistent=1,
                     task={"input_variables": {"a": 0, "b": 1}, "target_variables": ["a"]})
    with pytest.raises(ValueError, match="consistent"):
        FusedTrainer(spec(cout=1), 2, (48, 48), device=d, consistent=1)
    with pytest.raises(ValueError, match="consistent"):
        TiledInference(spec(scale=2), torch.zeros(8, device="cpu"), (2, 192, 192), (96, 96), device=d, consistent=1)
    assert torch.cuda.memory_allocated(d) == before
