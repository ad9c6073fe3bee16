"""The gradient loss term on the HIP path: srmi_gradient_loss_* / srmi.gradient.GradientLoss and
FusedTrainer(gradient=...) against the oracle (tests/gradient_oracle.py).

Bars of the kernel tests.  The device works in fp32, so it is held to the error of the SAME
arithmetic done in numpy on the very case under test (the rule of tests/test_gpu_ssim.py):
  * e32 is the distance of the fp32 oracle's plane mean (or L_grad) from the fp64 oracle's.  Per
    plane |parts / n - the fp64 oracle's| <= 10 e32 + 9 u |mean|, u = 2^-24; L_grad takes the same
    bar.  The floor counts the roundings of the defined sequence, each u relative: e = p - t (1)
    and the operator's three (the doubling and the division by 8 are exact) make 4 u on a and on
    b, so 4 u on phi (homogeneous of degree <= 1); the two squares, their sum and + eps 4 u
    under the root, so 2 u; the root 1 u; the one rounding of parts 1 u and that of L_grad to
    fp32 1 u: 9 u.
  * The gradient of a plane may be 10 x the fp32 closed-form oracle's own rel-L2 error from
    fp64 off, and 10 x its largest absolute error, no floor.
  * cparts, Nused and 1 / Nused are exact; the gradient of pred == target is exactly 0.
Every test prints its figures before it asserts.  Measured on an MI355X over the 30 cases
(DESIGN.md "Gradient loss"): the plane means 2.6e-11 .. 2.0e-8 off, at most 0.09 of their bar,
L_grad at most 0.10 of its bar; the gradient of the 52 planes that have one is the fp32
oracle's (1.00 x its rel-L2 error, 2.7e-8 .. 9.8e-8, and 1.00 x its largest absolute error).

The shapes are the smallest at which the kernels can go wrong: one position; one row of
positions over several column tiles; a ragged plane (W % 4 != 0: the scalar path); one position
more than the 16 x 64 rectangle a workgroup owns, both ways, and one pixel row more without a
position (the 16-byte path with a partial tile); and the training tile.

Bars of the trainer tests: those of tests/test_gpu_ssim_loss.py, named at each test."""
import ctypes as C
import functools
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gradient_oracle as go  # noqa: E402
import land_train_oracle as lt  # noqa: E402
import test_gpu_model  # noqa: E402
from oracle import rcan_oracle as ro  # noqa: E402
from srmi import _lib  # noqa: E402
from srmi._lib import ptr, stream_handle  # noqa: E402
from srmi.engine import param_table  # noqa: E402
from srmi.gradient import GradientLoss, GradientScore  # noqa: E402
from srmi.trainer import FusedTrainer  # noqa: E402
from test_gpu_gradient import TILE_H, TILE_W, scatter_nonfinite  # noqa: E402
from test_gpu_model import flat_from_model, rel_l2  # noqa: E402
from test_gpu_spectral_loss import SPECTRAL, init_flat, rcan_spec  # noqa: E402
from test_gpu_ssim_loss import SSIM, bits, dev, nbits, shape4, sid  # noqa: E402

SHAPES = [(2, 3, 3), (2, 3, 300), (3, 12, 75), (2, TILE_H + 2, TILE_W + 2), (2, TILE_H + 1, TILE_W + 4), (4, 192, 192)]
KINDS = ["zero", "k290", "nan", "allnan", "equal"]
BASE = 0.75
KEYS = ("parts", "cparts", "grad4", "total", "dy")
U = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def fields(shape, kind):
    """(pred, target) [N, C, H, W] fp32.  zero: a smooth truth plus noise at mean 0, pred = truth +
    noise; k290: the same at 290 +- 1.5 with a prediction of another mean and gain; nan: zero with
    scattered NaN / Inf in both, some on the plane's corners and on the workgroups' seams; allnan:
    zero with the LAST target plane all NaN; equal: pred == target."""
    n, H, W = shape
    rng = np.random.default_rng(700 + 10 * SHAPES.index(shape) + KINDS.index(kind))
    y, x = np.mgrid[:H, :W]
    t = np.zeros((n, H, W))
    for k in range(n):
        ph = rng.uniform(0, 2 * np.pi, 3)
        t[k] = (np.sin(0.21 * y + ph[0]) * np.cos(0.13 * x + ph[1]) + 0.5 * np.sin(0.05 * (x + y) + ph[2])
                + 0.3 * rng.standard_normal((H, W)))
    noise = 0.3 * rng.standard_normal((n, H, W))
    if kind == "k290":
        p, t = 290.4 + 1.5 * (0.8 * t + noise), 290.0 + 1.5 * t
    elif kind == "equal":
        p = t.copy()
    else:
        p = t + noise
    p, t = p.astype(np.float32), t.astype(np.float32)
    if kind == "nan":
        scatter_nonfinite(p, t, rng)
    if kind == "allnan":
        t[-1] = np.nan
    p, t = p.reshape(shape4(shape)), t.reshape(shape4(shape))
    p.setflags(write=False)
    t.setflags(write=False)
    return p, t


@functools.lru_cache(maxsize=None)
def oracle_pair(shape, kind):
    p, t = fields(shape, kind)
    return go.loss_and_grad(p, t), go.loss_and_grad(p, t, dtype=np.float32)


def run(p, t, eps=1e-6, weight=1.0, dy0=None, splits=None, base=BASE, fill=0xFF):
    """numpy p, t [N, C, H, W] -> dict of numpy results; dy0: what dy holds before add_dy (zeros
    when None); splits: tile ranges the batch goes through parts / add_dy in; fill: what the
    workspace holds before (it need not be initialised)."""
    d = dev()
    N = p.shape[0]
    gl = GradientLoss(p.shape, weight, eps, device=d)
    gl.workspace.fill_(fill)
    gl.gparts.fill_(-7.0)
    pd, td = torch.tensor(p, device=d), torch.tensor(t, device=d)
    dy = torch.zeros(p.shape, device=d) if dy0 is None else torch.tensor(dy0, device=d)
    b = torch.tensor([base], device=d)
    splits = splits or [(0, N)]
    for i, j in splits:
        gl.parts(pd[i:j], td[i:j], rows=i)
    gl.finalize(b)
    for i, j in splits:
        gl.add_dy(dy[i:j], pd[i:j], td[i:j], rows=slice(i, j))
    torch.cuda.synchronize()
    parts, cparts = gl.views()
    Cn = p.shape[1]
    return dict(parts=parts.cpu().numpy().reshape(N, Cn), cparts=cparts.cpu().numpy().reshape(N, Cn),
                grad4=gl.grad4.cpu().numpy(), total=gl.total.cpu().numpy(), dy=dy.cpu().numpy(),
                base=b.cpu().numpy())


@functools.lru_cache(maxsize=None)
def plain_run(shape, kind):
    return run(*fields(shape, kind))


def same_bits(a, b):
    for key in KEYS:
        assert np.array_equal(nbits(a[key]), nbits(b[key])), key


# ------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_parts_counts_term_and_gradient_match_the_oracle(shape, kind):
    p, t = fields(shape, kind)
    o64, o32 = oracle_pair(shape, kind)
    res = plain_run(shape, kind)
    tag = f"{sid(shape)} {kind}"
    H, W = shape[1:]
    full = (H - 2) * (W - 2)
    n = o64["counts"]
    live = n > 0
    if kind in ("zero", "k290", "equal"):
        assert (n == full).all()
    if kind == "allnan":
        assert n.reshape(-1)[-1] == 0 and n.reshape(-1)[0] == full
    if kind == "nan" and H * W > 9:
        assert (n < full).all()
    assert np.array_equal(res["cparts"], n.astype(np.float32))
    assert (nbits(res["parts"])[~live] == 0).all()
    if live.any():
        m64, m32 = o64["parts"][live] / n[live], o32["parts"][live] / n[live]
        e32 = np.abs(m32 - m64)
        bar = 10.0 * e32 + 9 * U * np.abs(m64)
        err = np.abs(res["parts"].astype(np.float64)[live] / n[live] - m64)
        print(f"{tag}: plane means off by {float(err.max()):.3e}, e32 {float(e32.max()):.3e}, worst "
              f"{float((err / bar).max()):.3f} of its bar")
        assert (err <= bar).all()
    # the term
    g4 = res["grad4"]
    if o64["nused"]:
        assert g4[1] == o64["nused"] and nbits(g4[2]) == nbits(np.float32(1.0 / o64["nused"]))
        e32 = abs(o32["loss"] - o64["loss"])
        bar = 10.0 * e32 + 9 * U * abs(o64["loss"])
        lerr = abs(float(g4[3]) - o64["loss"])
        print(f"{tag}: L_grad {g4[3]:.8f} oracle {o64['loss']:.8f} off by {lerr:.3e}, e32 {e32:.3e} ({lerr / bar:.3f} of "
              f"the bar)")
        assert lerr <= bar and abs(float(g4[0]) - o64["S"]) <= bar * o64["nused"]
    else:
        assert (nbits(g4) == 0).all()
    if kind == "equal":  # phi = sqrt(eps) at every position
        assert abs(float(g4[3]) - 1e-3) <= 9 * U * 1e-3
    # total = fma(weight, L_grad, base): the exact product, one rounding
    assert nbits(res["total"])[0] == nbits(np.float32(np.float64(np.float32(BASE)) + np.float64(g4[3])))[0]
    assert res["base"][0] == np.float32(BASE)  # only read
    # the gradient, plane by plane
    g64, g32 = o64["grad"].reshape(-1, H, W), o32["grad"].reshape(-1, H, W)
    dy = res["dy"].reshape(-1, H, W).astype(np.float64)
    assert np.isfinite(res["dy"]).all()
    for k in range(shape[0]):
        nrm = np.linalg.norm(g64[k])
        if kind == "equal" or not live.reshape(-1)[k] or not o64["nused"]:
            assert nrm == 0 and (dy[k] == 0).all()  # exactly 0
            continue
        e_l2, e_max = np.linalg.norm(g32[k] - g64[k]) / nrm, np.abs(g32[k] - g64[k]).max()
        d_l2, d_max = np.linalg.norm(dy[k] - g64[k]) / nrm, np.abs(dy[k] - g64[k]).max()
        print(f"{tag} plane {k}: gradient rel-L2 fp32 oracle {e_l2:.3e}, device {d_l2:.3e} ({d_l2 / e_l2:.2f} x); "
              f"max-abs fp32 oracle {e_max:.3e}, device {d_max:.3e} ({d_max / e_max:.2f} x)")
        assert d_l2 <= 10.0 * e_l2 and d_max <= 10.0 * e_max
    # a pixel that is not finite in both takes nothing
    assert (nbits(res["dy"])[~o64["fin"]] == 0).all()


# ----------------------------------------------------------- 2. into a random dy
@pytest.mark.parametrize("shape,kind", [(SHAPES[1], "zero"), (SHAPES[3], "nan"), (SHAPES[5], "k290")],
                         ids=["3x300", "18x66 nan", "192 k290"])
def test_add_dy_adds_to_what_dy_holds(shape, kind):
    p, t = fields(shape, kind)
    rng = np.random.default_rng(7)
    dy0 = (1e-3 * rng.standard_normal(p.shape)).astype(np.float32)
    dy0.flat[::5] = -0.0
    res = run(p, t, dy0=dy0)
    g = plain_run(shape, kind)["dy"].astype(np.float64)  # 0 + the gradient: the gradient, rounded once
    want = dy0.astype(np.float64) + g
    # dy = fma(scale, sum, dy0): the rounding of g (not made here) and the rounding of the result
    err = np.abs(res["dy"].astype(np.float64) - want)
    print(f"{sid(shape)} {kind}: largest error {float((err / (U * (np.abs(g) + np.abs(want)) + 1e-300)).max()):.3f} of the bar")
    assert (err <= U * (np.abs(g) + np.abs(want))).all()
    assert np.abs(g).max() > 0


# ------------------------------------------------------------------ 3. weight 0
@pytest.mark.parametrize("shape,kind", [(SHAPES[2], "nan"), (SHAPES[5], "zero")], ids=["12x75 nan", "192 zero"])
def test_weight_zero_leaves_dy_as_it_is(shape, kind):
    p, t = fields(shape, kind)
    rng = np.random.default_rng(8)
    dy0 = rng.standard_normal(p.shape).astype(np.float32)
    dy0.flat[::3] = -0.0
    dy0.flat[1::7] = np.nan
    res = run(p, t, weight=0.0, dy0=dy0)
    ref = plain_run(shape, kind)
    assert np.array_equal(nbits(res["dy"]), nbits(dy0))
    for key in ("parts", "cparts", "grad4"):
        assert np.array_equal(nbits(res[key]), nbits(ref[key])), key
    assert nbits(res["total"])[0] == nbits(np.float32(BASE))[0]


# ------------------------------------------------- 4. non-finite pixels, unused planes
@pytest.mark.parametrize("shape", SHAPES[1:], ids=sid)
def test_non_finite_pixels_keep_the_bits_of_dy(shape):
    p, t = fields(shape, "nan")
    fin = np.isfinite(p) & np.isfinite(t)
    assert (~fin).any()
    dy0 = np.full(p.shape, -0.0, np.float32)
    dy0.reshape(-1)[::2] = np.float32(np.nan)
    pat = nbits(dy0).copy()
    pat[np.isnan(dy0)] = -4194304 + 0x12345  # 0xffc12345: the sign bit and a payload
    dy0 = pat.view(np.float32)
    res = run(p, t, dy0=dy0)
    assert np.array_equal(nbits(res["dy"])[~fin], nbits(dy0)[~fin])
    assert (plain_run(shape, "nan")["cparts"] > 0).any()
    # another NaN, and Inf for NaN: the same bits everywhere
    t2 = nbits(t).copy()
    t2[np.isnan(t)] = -4194304 + 0x54321
    t2 = t2.view(np.float32)
    p2 = np.where(np.isnan(p), np.float32(-np.inf), p)
    same_bits(run(p2, t2), plain_run(shape, "nan"))


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_no_used_position_is_zero_not_nan(shape):
    p, t = (v.copy() for v in fields(shape, "zero"))
    t[:, :, 1::3, 1::3] = np.nan  # every 3 x 3 window holds one
    rng = np.random.default_rng(9)
    dy0 = rng.standard_normal(p.shape).astype(np.float32)
    dy0.flat[::3] = 0.0
    res = run(p, t, dy0=dy0)
    assert (res["cparts"] == 0).all() and (nbits(res["parts"]) == 0).all() and (nbits(res["grad4"]) == 0).all()
    assert nbits(res["total"])[0] == nbits(np.float32(BASE))[0]
    assert np.array_equal(nbits(res["dy"]), nbits(dy0))


# ------------------------------------------------------------- 5. determinism
@pytest.mark.parametrize("kind", ["k290", "nan", "allnan"])
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_bit_identical_runs_plane_ranges_and_workspace_contents(shape, kind):
    p, t = fields(shape, kind)
    a = plain_run(shape, kind)
    same_bits(a, run(p, t))
    same_bits(a, run(p, t, fill=0x00))  # whatever the workspace held
    same_bits(a, run(p, t, fill=0x7F))
    N = p.shape[0]
    if N > 1:  # the batch in two calls over tile ranges, the later range first
        same_bits(a, run(p, t, splits=[(1, N), (0, 1)]))


def test_the_16_byte_and_the_scalar_path_give_the_same_bits():
    """The training tile through buffers that are 4 bytes off a 16-byte boundary."""
    d = dev()
    shape = SHAPES[5]
    p, t = fields(shape, "nan")
    a = plain_run(shape, "nan")
    gl = GradientLoss(p.shape, device=d)
    n = p.size

    def off(v):
        buf = torch.zeros(n + 4, device=d)
        buf[1:1 + n].copy_(torch.tensor(v, device=d).reshape(-1))
        return buf[1:1 + n].view(p.shape)
    pd, td, dy = off(p), off(t), off(np.zeros_like(p))
    assert ptr(pd) % 16 == 4 and pd.is_contiguous()
    gl.parts(pd, td)
    gl.finalize(torch.tensor([BASE], device=d))
    gl.add_dy(dy, pd, td)
    torch.cuda.synchronize()
    assert np.array_equal(nbits(gl.grad4.cpu().numpy()), nbits(a["grad4"]))
    assert np.array_equal(nbits(gl.views()[0].cpu().numpy().reshape(a["parts"].shape)), nbits(a["parts"]))
    assert np.array_equal(nbits(dy.cpu().numpy()), nbits(a["dy"]))


# ------------------------------------------------------------ 6. chaining and the score
def test_from_parts_chains_onto_a_given_base():
    shape = SHAPES[3]
    p, t = fields(shape, "zero")
    ref = plain_run(shape, "zero")
    for base, weight in ((0.0, 1.0), (-3.5, 1.0), (1.2345678, 0.3), (1e-3, 2.5)):
        res = run(p, t, weight=weight, base=base)
        assert np.array_equal(nbits(res["grad4"]), nbits(ref["grad4"]))
        want = np.float32(np.float64(np.float32(base)) + np.float64(np.float32(weight)) * np.float64(res["grad4"][3]))
        assert nbits(res["total"])[0] == nbits(want)[0], (base, weight)
        assert res["base"][0] == np.float32(base)
    # the gradient follows the weight
    res = run(p, t, weight=2.5)
    assert rel_l2(res["dy"], 2.5 * ref["dy"].astype(np.float64)) < 4 * U


# (the normaliser's multiplier m, the scalars before weight, whether l = 1 - S / (N m)) of srmi_<term>_loss_from_parts
FROM_PARTS = {"spectral": (32.0, (32,), False), "ssim": (1.0, (), True), "gradient": (1.0, (), False)}


def from_parts_expected(parts, cparts, m, one_minus, weight, base):
    """srmi.h's order restated with Python floats (fp64, nothing fused): 256 contiguous shares of
    ceil(nplanes / 256) planes, each summed left to right, then the 256 share sums left to right;
    the record and l rounded to fp32 once each.  total = fma(weight, l, base): with weight 1 or
    0.5 the product is exact, the fp64 sum of two fp32 values within 2^29 of each other is exact,
    and one rounding to fp32 is left."""
    n = len(parts)
    share = -(-n // 256)
    S = N = 0.0
    for k in range(256):
        s = c = 0.0
        for i in range(min(k * share, n), min((k + 1) * share, n)):
            s += float(parts[i])
            c += float(cparts[i])
        S += s
        N += c
    rec = np.zeros(4, np.float32)
    if N > 0.0:
        q = S / (N * m)
        rec[:] = [S, N, 1.0 / (N * m), 1.0 - q if one_minus else q]
    total = np.float32(float(np.float32(base)) + float(np.float32(weight)) * float(rec[3]))
    return rec, total


@pytest.mark.parametrize("nplanes", [1, 255, 256, 257, 1000])
@pytest.mark.parametrize("term", list(FROM_PARTS))
def test_from_parts_groups_the_planes_as_documented_bit_for_bit(term, nplanes):
    """The three finalize launches on host-made parts (positive, of order 1) and counts (whole
    numbers in 1 .. 2^20, or all zero): the record and the total are the bits of the host
    restatement above, which never sees the code under test.  1, 255 and 256 planes are the plain
    sum in plane order, 257 the first size with shares of two planes (and empty shares behind
    them), 1000 shares of four with a ragged end."""
    d = dev()
    m, scalars, one_minus = FROM_PARTS[term]
    f = getattr(_lib.load(), f"srmi_{term}_loss_from_parts")
    rng = np.random.default_rng(1000 * list(FROM_PARTS).index(term) + nplanes)
    parts = rng.uniform(0.5, 1.5, nplanes).astype(np.float32)
    counts = rng.integers(1, 2 ** 20 + 1, nplanes).astype(np.float32)
    for weight, base, cparts in ((1.0, 0.75, counts), (0.5, 1.2345678, counts), (1.0, 0.75, np.zeros_like(counts))):
        l4 = torch.tensor([-7.0, -7.0, -7.0, base], device=d)  # a finalised pixel loss: [3] is the base
        rec, tot = torch.full((4,), -7.0, device=d), torch.full((1,), -7.0, device=d)
        pd, cd = torch.tensor(parts, device=d), torch.tensor(cparts, device=d)
        assert f(ptr(pd), ptr(cd), nplanes, *scalars, weight, ptr(l4[3:4]), ptr(rec), ptr(tot), stream_handle()) == 0
        torch.cuda.synchronize()
        want_rec, want_tot = from_parts_expected(parts, cparts, m, one_minus, weight, base)
        got_rec, got_tot = rec.cpu().numpy(), tot.cpu().numpy()
        print(f"{term} nplanes={nplanes} weight={weight} N={want_rec[1]:.0f}: record {got_rec.tolist()} want "
              f"{want_rec.tolist()}; total {got_tot[0]!r} want {want_tot!r}")
        assert np.array_equal(nbits(got_rec), nbits(want_rec)), (weight, got_rec, want_rec)
        assert nbits(got_tot)[0] == nbits(want_tot)[0], (weight, got_tot, want_tot)
        assert cparts.any() or (not got_rec.any() and got_tot[0] == np.float32(base))  # no used position: 0, not NaN
        assert np.array_equal(l4.cpu().numpy(), np.array([-7.0, -7.0, -7.0, base], np.float32))  # only read


@pytest.mark.parametrize("shape,kind", [(SHAPES[0], "zero"), (SHAPES[3], "zero"), (SHAPES[3], "nan"), (SHAPES[5], "zero")],
                         ids=["3x3", "18x66", "18x66 nan", "192"])
def test_one_plane_is_the_mean_of_phi_from_the_scores_path(shape, kind):
    """Against a zero truth the score's |g_p| is sqrt(Gx[p]^2 + Gy[p]^2), the term's phi without
    eps: with eps far below |g|^2 in fp32 (1e-30) the two paths agree, L_grad = mean_pred, to
    the roundings of either (7 u and 9 u of the value, see the two modules' bars)."""
    p, t = fields(shape, kind)
    with np.errstate(invalid="ignore"):
        e = (p.astype(np.float64) - t).astype(np.float32).reshape(-1, *shape[1:])[:1]  # NaN / Inf where either is
    z = np.zeros_like(e)
    d = dev()
    m = GradientScore(e.shape, device=d).measure(torch.tensor(e, device=d), torch.tensor(z, device=d))
    res = run(e[None], z[None], eps=1e-30)
    got, want = float(res["grad4"][3]), float(m["mean_pred"][0])
    print(f"{sid(shape)} {kind}: L_grad {got:.9f}, the score's mean_pred {want:.9f}, apart {abs(got - want):.3e} (bar "
          f"{16 * U * want:.3e})")
    assert res["grad4"][1] == float(m["count"][0]) > 0
    assert abs(got - want) <= 16 * U * want


# ------------------------------------------------------------------- capture
def test_the_launches_are_capturable_and_replay_on_new_inputs():
    d = dev()
    shape = SHAPES[3]
    p, t = (torch.tensor(v, device=d) for v in fields(shape, "nan"))
    p2 = (p + 0.1 * torch.arange(p.shape[-1], device=d)).contiguous()
    gl = GradientLoss(p.shape, device=d)
    pa, dy, b = p.clone(), torch.zeros_like(p), torch.tensor([BASE], device=d)

    def stage():
        gl.parts(pa, t)
        gl.finalize(b)
        gl.add_dy(dy, pa, t)
    stage()  # warm-up outside capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(device=d)
    s.wait_stream(torch.cuda.current_stream(d))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            stage()
    torch.cuda.current_stream(d).wait_stream(s)
    pa.copy_(p2)
    dy.zero_()
    gl.grad4.fill_(-7.0)
    g.replay()
    torch.cuda.synchronize()
    eager = run(p2.cpu().numpy(), t.cpu().numpy())
    assert np.array_equal(nbits(gl.grad4.cpu().numpy()), nbits(eager["grad4"])) and eager["grad4"][1] > 0
    assert np.array_equal(nbits(dy.cpu().numpy()), nbits(eager["dy"]))
    assert np.array_equal(nbits(gl.total.cpu().numpy()), nbits(eager["total"]))
    assert not np.array_equal(eager["grad4"], plain_run(shape, "nan")["grad4"])  # the inputs do differ


# ----------------------------------------------------------- 7. refused arguments
def test_refused_arguments_launch_nothing():
    lib = _lib.load()
    d = dev()
    E = _lib.SRMI_ERR_ARG
    H, W = 24, 40
    n = C.c_size_t(0)
    wsz = lib.srmi_gradient_loss_workspace
    assert wsz(2, H, W, C.byref(n)) == 0 and n.value > 0 and n.value % 32 == 0
    nbytes = n.value
    one = C.c_size_t(0)
    assert wsz(1, H, W, C.byref(one)) == 0 and 2 * one.value == nbytes  # plane by plane
    for bad in ((2, 2, W), (2, H, 2), (0, H, W), (-1, H, W), (1, 4096, 4097), (1, 3, (1 << 24) // 3 + 1)):
        assert wsz(*bad, C.byref(n)) == E, bad
    assert wsz(1, 4096, 4096, C.byref(n)) == 0
    assert wsz(2, H, W, None) == E
    p = torch.randn(2, 1, H, W, device=d)
    t = torch.randn(2, 1, H, W, device=d)
    ws = torch.full((nbytes + 16,), 0x5A, dtype=torch.uint8, device=d)
    parts, cparts = torch.full((2,), -7.0, device=d), torch.full((2,), -7.0, device=d)
    base = torch.full((1,), -7.0, device=d)
    g4, tot = torch.full((4,), -7.0, device=d), torch.full((1,), -7.0, device=d)
    dy = torch.full((2, 1, H, W), -7.0, device=d)
    st = stream_handle()
    nan, inf = float("nan"), float("inf")
    f = lib.srmi_gradient_loss_parts
    ok = dict(pred=ptr(p), target=ptr(t), nplanes=2, H=H, W=W, eps=1e-6, parts=ptr(parts), cparts=ptr(cparts),
              ws=ptr(ws), nbytes=nbytes)
    for change in (dict(H=2), dict(W=2), dict(nplanes=0), dict(eps=0.0), dict(eps=-1e-6), dict(eps=nan), dict(eps=inf),
                   dict(pred=None), dict(target=None), dict(parts=None), dict(cparts=None), dict(ws=None),
                   dict(nbytes=nbytes - 1), dict(ws=ptr(ws) + 4), dict(H=4096, W=4097)):
        a = dict(ok, **change)
        assert f(a["pred"], a["target"], a["nplanes"], a["H"], a["W"], a["eps"], a["parts"], a["cparts"], a["ws"],
                 a["nbytes"], st) == E, change
    f = lib.srmi_gradient_loss_from_parts
    ok = dict(parts=ptr(parts), cparts=ptr(cparts), nplanes=2, weight=1.0, base=ptr(base), g4=ptr(g4), total=ptr(tot))
    for change in (dict(nplanes=0), dict(weight=-1.0), dict(weight=inf), dict(weight=nan), dict(parts=None),
                   dict(cparts=None), dict(base=None), dict(g4=None), dict(total=None)):
        a = dict(ok, **change)
        assert f(a["parts"], a["cparts"], a["nplanes"], a["weight"], a["base"], a["g4"], a["total"], st) == E, change
    f = lib.srmi_gradient_loss_dy  # it recomputes U and V: no workspace to refuse
    ok = dict(pred=ptr(p), target=ptr(t), nplanes=2, H=H, W=W, eps=1e-6, weight=1.0, g4=ptr(g4), dy=ptr(dy))
    for change in (dict(H=2), dict(W=2), dict(nplanes=0), dict(weight=-1.0), dict(weight=nan), dict(weight=inf),
                   dict(eps=0.0), dict(eps=nan), dict(eps=inf), dict(pred=None), dict(target=None), dict(g4=None),
                   dict(dy=None), dict(H=4096, W=4097)):
        a = dict(ok, **change)
        assert f(a["pred"], a["target"], a["nplanes"], a["H"], a["W"], a["eps"], a["weight"], a["g4"], a["dy"],
                 st) == E, change
    torch.cuda.synchronize()
    # nothing was launched: every output still holds what it was filled with
    assert (parts == -7.0).all() and (cparts == -7.0).all() and (g4 == -7.0).all() and (tot == -7.0).all()
    assert (dy == -7.0).all() and (ws == 0x5A).all() and (base == -7.0).all()
    # the Python layer says which value it refuses
    for kw, what in ((dict(weight=-1.0), "weight -1.0"), (dict(weight=nan), "weight nan"), (dict(eps=0.0), "eps 0.0"),
                     (dict(eps=inf), "eps inf")):
        with pytest.raises(ValueError, match=what):
            GradientLoss((2, 1, H, W), device=d, **kw)
    with pytest.raises(ValueError, match="the window"):
        GradientLoss((2, 1, 2, 48), device=d)
    with pytest.raises(ValueError, match="global batch"):
        GradientLoss((2, 1, H, W), device=d, global_batch=1)


# ===================================================================== the trainer
WEIGHT = 1.0  # weight * L_grad is 0.54 (l2) and 0.68 (charbonnier) of the pixel loss in the fp64 oracle
GRADIENT = dict(weight=WEIGHT)
NAMES = ("loss", "pixel_loss", "gradient_loss")


# ------------------------------------------------- T1. weight 0 is the plain trainer
@pytest.mark.parametrize("loss_fn", ["l2", "charbonnier"])
@pytest.mark.parametrize("B,micro", [(2, 1), (4, 2)])
def test_weight_zero_trainer_is_the_plain_trainer(B, micro, loss_fn):
    """The parts and the finalise run, add_dy launches nothing, total = loss4[3] + 0 * L_grad,
    and the backward takes the pixel loss's dy as it is: every bit of two steps is the plain
    trainer's."""
    spec = rcan_spec(1, 2)
    flat = init_flat(spec, 5)
    hr = torch.tensor(ro.synthetic_hr(B, 2, 192, 19), device=dev())
    res = []
    for gradient in (None, dict(weight=0.0)):
        tr = FusedTrainer(spec, B, (48, 48), device=dev(), params=flat, micro=micro, loss_fn=loss_fn, gradient=gradient)
        assert tr.micro == micro and (tr.gradient is None) == (gradient is None)
        assert gradient is None or tr.dy is not None
        rows = []
        for _ in range(2):
            out = tr.step(hr)
            torch.cuda.synchronize()
            assert set(out) == ({"loss", "interp_loss"} if gradient is None else
                                {"loss", "interp_loss", "pixel_loss", "gradient_loss"})
            rows.append((out["loss"].clone(), out["interp_loss"].clone(), tr.sr.clone(), tr.grads.clone(),
                         tr.params.clone()))
        if gradient is not None:
            assert torch.equal(bits(out["pixel_loss"]), bits(out["loss"])) and float(out["gradient_loss"]) > 0
        res.append(rows)
        del tr
    for k, (a, b) in enumerate(zip(*res)):
        for x, y, what in zip(a, b, ("loss", "interp_loss", "sr", "grads", "params")):
            assert torch.equal(bits(x), bits(y)), (k, what, float((x - y).abs().max()))
    assert np.isfinite(float(res[0][1][0]))


# --------------------------------------------------------- T2. / T4. against fp64
def gradient_drift_bounds(monkeypatch, model, hr, scale, g_ref, **kw):
    """test_gpu_model.drift_bounds itself (3 x the drift of the same fp64 step with bf16-rounded
    conv operands, + 1e-3) with the oracle step it runs the emulation through replaced by the
    one with the term(s), as test_gpu_ssim_loss.ssim_drift_bounds does."""
    monkeypatch.setattr(test_gpu_model, "oracle_grads", lambda m, h, s: go.train_step(m, h, s, **kw)[:3])
    return test_gpu_model.drift_bounds(model, hr, scale, g_ref)


def used_positions(hr):
    """[B, C]: the used positions of every plane when the prediction is finite everywhere."""
    fin = np.isfinite(hr)
    return np.array([[go.used_positions(fin[b, c]).sum() for c in range(hr.shape[1])] for b in range(hr.shape[0])])


def step_vs_oracle(monkeypatch, hr, loss_fn, land, spectral=None, ssim=None, consistent=0):
    d = dev()
    model = ro.RCANOracle(nchannels_in=2, nchannels_out=2, nlayers=2, nblocks=2, nfeatures=64, cbottleneck=2)
    ro.init_params_numpy(model, 22)
    spec = rcan_spec(2, 2)
    table = param_table(spec)
    flat = flat_from_model(model, table).to(d)
    model = model.double()
    kw = dict(loss_fn=loss_fn, gradient_cfg=GRADIENT, ssim_cfg=ssim, spectral_cfg=spectral, consistent=consistent)
    l_ref, _, g_ref, info = go.train_step(model, hr, 4, **kw)
    share = WEIGHT * info["gradient_loss"] / info["pixel_loss"]
    print(f"{loss_fn} land={land}: weight * L_grad is {share:.3f} of the pixel loss in the fp64 oracle")
    assert share >= 0.1  # the term is a real share of the loss
    bound = gradient_drift_bounds(monkeypatch, model, hr, 4, g_ref, **kw)
    tr = FusedTrainer(spec, 3, (48, 48), device=d, params=flat, loss_fn=loss_fn, land=land, gradient=GRADIENT,
                      ssim=ssim, spectral=spectral, consistent=consistent)
    assert tr.dy is not None
    hr_d = torch.tensor(hr, device=d)
    out = tr.step(hr_d)
    torch.cuda.synchronize()
    keys = [("loss", l_ref), ("pixel_loss", info["pixel_loss"]), ("gradient_loss", info["gradient_loss"])]
    if spectral is not None:
        keys.append(("spectral_loss", info["spectral_loss"]))
    if ssim is not None:
        keys.append(("ssim_loss", info["ssim_loss"]))
    assert set(out) == {k for k, _ in keys} | {"interp_loss"}
    for key, ref in keys:
        got = float(out[key])
        print(f"{loss_fn} land={land} spectral={spectral is not None} ssim={ssim is not None} K={consistent}: {key} "
              f"{got:.6f} oracle {ref:.6f} rel {abs(got - ref) / ref:.2e} (bar 2e-3)")
        assert abs(got - ref) / ref < 2e-3, key
    assert float(tr.gradient.grad4[1]) == info["nused"] == used_positions(hr).sum()
    g = tr.grads.cpu()
    if consistent:
        # behind the layer the last conv's bias has an exact gradient of zero: see
        # test_gpu_ssim_loss.step_vs_oracle
        from test_gpu_consistency_train import check_grads
        assert check_grads(table, g, g_ref, bound, info, f"{loss_fn} K={consistent}") == ["tail.1.bias"]
    else:
        worst = 0.0
        for name, off, n, shape in table:
            r = rel_l2(g[off:off + n].view(shape), g_ref[name])
            worst = max(worst, r / bound[name])
            assert r <= bound[name], (name, r, bound[name])
        print(f"{loss_fn} land={land}: worst gradient tensor at {worst:.2f} of its drift bound")
    dy = tr.dy.cpu().numpy().copy()
    out = tr.step(hr_d)
    torch.cuda.synchronize()
    assert torch.isfinite(tr.params).all() and np.isfinite(float(out["loss"]))
    return tr, dy, info


@pytest.mark.parametrize("loss_fn", ["l2", "charbonnier"])
def test_gradient_trainer_step_vs_oracle(loss_fn, monkeypatch):
    """test_ssim_trainer_step_vs_oracle's bars: the losses 2e-3 relative, every gradient tensor
    within test_gpu_model.drift_bounds."""
    tr, _, info = step_vs_oracle(monkeypatch, ro.synthetic_hr(3, 2, 192, 21), loss_fn, False)
    assert info["nused"] == 3 * 2 * 190 * 190


@pytest.mark.parametrize("loss_fn", ["l2", "charbonnier"])
def test_gradient_land_trainer_step_vs_oracle(loss_fn, monkeypatch):
    hr = lt.land_batch(3, 2, 192, 21)
    lt.check_conditions(hr, 4)
    used = used_positions(hr)
    assert used.tolist() == [[36100, 36100], [19616, 19616], [19616, 19616]] and 190 * 190 == 36100
    tr, dy, info = step_vs_oracle(monkeypatch, hr, loss_fn, True)
    assert 0 < info["nused"] < 3 * 2 * 36100
    assert (dy[~np.isfinite(hr)].view(np.int32) == 0).all()  # +0.0f on land


def test_all_terms_consistent_trainer_step_vs_oracle(monkeypatch):
    """Spectral + SSIM + gradient + consistent=2 against the composed oracle: the term chains
    onto the SSIM term's total, and its gradient enters before the layer's adjoint."""
    step_vs_oracle(monkeypatch, ro.synthetic_hr(3, 2, 192, 21), "l2", False, spectral=SPECTRAL, ssim=SSIM, consistent=2)


def test_gradient_chains_onto_the_spectral_term_without_an_ssim_term(monkeypatch):
    """The chain with a gap, spectral + gradient and no SSIM term, against the composed oracle
    at the bars above: the gradient term's total is the spectral term's + weight * L_grad (one
    fp32 fma; with weight 1 the fp64 sum of the two floats, rounded once), as the spectral
    term's is the pixel loss + its own."""
    tr, _, _ = step_vs_oracle(monkeypatch, ro.synthetic_hr(3, 2, 192, 21), "l2", False, spectral=SPECTRAL, ssim=None)
    assert tr.ssim is None and [t.name for t in tr.terms] == ["spectral", "gradient"] and WEIGHT == 1.0
    base, l, total = (float(v) for v in (tr.spectral.total, tr.gradient.grad4[3], tr.gradient.total))
    want = np.float32(base + WEIGHT * l)
    print(f"spectral total {base!r} + {WEIGHT} * L_grad {l!r} = {float(want)!r}, the gradient term's total {total!r}")
    assert nbits(np.float32(total))[0] == nbits(want)[0]
    spec_want = np.float32(float(tr.loss4[3]) + float(tr.spectral.weight) * float(tr.spectral.spec4[3]))
    assert tr.spectral.weight == 1.0 and nbits(np.float32(base))[0] == nbits(spec_want)[0]


# ------------------------------------------------------------- T3. the fp32 engine
def test_gradient_trainer_fp32_step_vs_oracle():
    """test_ssim_trainer_fp32_step_vs_oracle's bars: the losses and the output 1e-5 relative,
    every gradient tensor 1e-3 rel-L2."""
    d = dev()
    model = ro.RCANOracle(nchannels_in=2, nchannels_out=2, nlayers=2, nblocks=2, nfeatures=64, cbottleneck=2)
    ro.init_params_numpy(model, 23)
    spec = rcan_spec(2, 2, dtype="fp32")
    table = param_table(spec)
    hr = ro.synthetic_hr(3, 2, 192, 21)
    tr = FusedTrainer(spec, 3, (48, 48), device=d, params=flat_from_model(model, table).to(d), gradient=GRADIENT)
    l_ref, out_ref, g_ref, info = go.train_step(model.double(), hr, 4, "l2", GRADIENT)
    out = tr.step(torch.tensor(hr, device=d))
    torch.cuda.synchronize()
    for key, ref in (("loss", l_ref), ("pixel_loss", info["pixel_loss"]), ("gradient_loss", info["gradient_loss"])):
        print(f"fp32: {key} {float(out[key]):.8f} oracle {ref:.8f} rel {abs(float(out[key]) - ref) / ref:.2e}")
        assert abs(float(out[key]) - ref) / ref < 1e-5, key
    assert rel_l2(tr.sr, out_ref) < 1e-5
    g = tr.grads.cpu()
    worst = max(rel_l2(g[off:off + n].view(shape), g_ref[name]) for name, off, n, shape in table)
    print(f"fp32 engine with the gradient term: worst per-tensor grad rel-L2 {worst:.2e} (bar 1e-3)")
    assert worst < 1e-3


# -------------------------------------------------------- T5. micro-batch split
def test_gradient_micro_batch_split():
    """test_ssim_micro_batch_split's bars: the losses equal as floats (sums and counts in plane
    order), the gradients to 1e-5 rel-L2."""
    spec = rcan_spec(1, 2)
    flat = init_flat(spec, 5)
    hr = torch.tensor(lt.land_batch(4, 2, 192, 24), device=dev())
    res = []
    for micro in (1, 2):
        tr = FusedTrainer(spec, 4, (48, 48), device=dev(), params=flat, micro=micro, land=True, gradient=GRADIENT)
        out = tr.step(hr)
        torch.cuda.synchronize()
        res.append(([float(out[k]) for k in NAMES], tr.grads.clone()))
        del tr
    (l1, g1), (l2, g2) = res
    print(f"micro 1 {l1}, micro 2 {l2}, gradients apart {rel_l2(g2, g1):.2e} (bar 1e-5)")
    assert l1 == l2 and all(np.isfinite(l1)) and l1[2] > 0
    assert rel_l2(g2, g1) < 1e-5


# ---------------------------------------------------------------- T6. data parallel
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
    tr = FusedTrainer(spec, b - a, (48, 48), device=d, params=flat, micro=2, info=info, land=True, gradient=GRADIENT)
    out = tr.step(hr_all[a:b].contiguous())
    torch.cuda.synchronize()
    q.put((rank, [float(out[k]) for k in NAMES], tr.grads.cpu().numpy(), tr.params.cpu().numpy()))
    dist.destroy_process_group()


def test_gradient_dp_world2_matches_single_process():
    """test_ssim_dp_world2_matches_single_process's conventions and bars (gloo, both ranks on
    cuda:0; gradients 2e-4 rel-L2): the ranks' used counts differ; sums and counts go through
    one all-reduce."""
    import multiprocessing as mp
    hr_np = lt.land_batch(4, 2, 192, 25)
    used = used_positions(hr_np).sum(axis=1)
    assert used[:2].sum() == 111432 and used[2:].sum() == 78464
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 49000 + random.randint(0, 2000)
    ps = [ctx.Process(target=_dp_worker, args=(r, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = sorted([q.get(timeout=100) for _ in ps], key=lambda t: t[0])
    for p in ps:
        p.join(timeout=30)
        assert p.exitcode == 0
    d = dev()
    spec = rcan_spec(1, 2)
    tr = FusedTrainer(spec, 4, (48, 48), device=d, params=init_flat(spec, 5), micro=1, land=True, gradient=GRADIENT)
    out = tr.step(torch.tensor(hr_np, device=d))
    torch.cuda.synchronize()
    losses, g = [float(out[k]) for k in NAMES], tr.grads.cpu().numpy()
    assert float(tr.gradient.grad4[1]) == used.sum()
    for rank, l_r, g_r, p_r in res:
        print(f"rank {rank}: losses {l_r} single process {losses}, gradients apart "
              f"{np.linalg.norm(g_r - g) / np.linalg.norm(g):.2e} (bar 2e-4)")
        assert l_r == losses, (rank, l_r, losses)
        assert np.linalg.norm(g_r - g) / np.linalg.norm(g) < 2e-4
    np.testing.assert_array_equal(res[0][3], res[1][3])  # replicas stay identical after Adam


# ------------------------------------------------------------------ T7. construction
@pytest.mark.parametrize("gradient,what", [
    (dict(weight=-0.5), "weight -0.5"), (dict(weight=float("nan")), "weight nan"),
    (dict(weight=float("inf")), "weight inf"), (dict(weight="1"), "weight '1'"),
    (dict(eps=0.0), "eps 0.0"), (dict(eps=float("nan")), "eps nan"), (dict(eps=float("inf")), "eps inf"),
    (dict(eps=-1e-6), "eps -1e-06"), (dict(wieght=1.0), "wieght"), (dict(window=3), "window"), ([1.0], "a dict")])
def test_trainer_refuses_a_bad_gradient_config(gradient, what):
    with pytest.raises(ValueError, match=what):
        FusedTrainer(rcan_spec(1, 1), 2, (48, 48), device=dev(), gradient=gradient)
    # an HR tile below the window in either dimension, before anything is allocated
    with pytest.raises(ValueError, match="larger than the HR tile"):
        FusedTrainer(rcan_spec(1, 1, scale=2), 2, (1, 16), device=dev(), gradient=dict(weight=1.0))
    with pytest.raises(ValueError, match="larger than the HR tile"):
        FusedTrainer(rcan_spec(1, 1, scale=2), 2, (16, 1), device=dev(), gradient={})
