"""The gradient score on the HIP path: srmi_gradient / srmi.gradient.GradientScore and
RegionSuperResolver.score_gradient against the oracle (tests/gradient_oracle.py).

Bars.  The device works in fp32, so it is held to the error of the SAME arithmetic done in
numpy on the very case under test (the rule of tests/test_gpu_ssim.py), plus a floor counted
from the defined operation sequence, each rounding 2^-24 relative (u):
  * |g| = sqrt(gx gx + gy gy) with gx = Gx inv_dx: the three roundings of the operator (the
    doubling and the division by 8 are exact) and the factor make 4 u on gx and on gy, which is
    4 u on |g| (it is homogeneous of degree 1), the two squares and their sum 3 u under the
    root, so 1.5 u, and the root 1 u: 6.5 u, taken as 7 u of the value for mean_pred and
    mean_truth, 14 u for their ratio, sharpness.
  * rmse_mag, rmse_vec: the same 7 u on each magnitude or component, so at most 7 u sqrt(2
    (sum |g_p|^2 + sum |g_t|^2) / n) on a root mean square of their differences.
  * cosine: 7 u on each factor of each of the three sums, 14 u of the numerator's bound and 14
    u of the denominator: 28 u.
  Each derived value is within 10 e32 + its floor of the fp64 oracle's, e32 the fp32 oracle's
  distance from the fp64 oracle on that value.  The sums are fp64 on the device, so nothing
  more is rounded.
  * The maps of a plane: within 10 x the fp32 oracle's own rel-L2 error and 10 x its largest
    absolute error; the NaN pattern equal.
  * count: exact.
Every test prints its figures before it asserts.  Measured on an MI355X over the 35 cases
(DESIGN.md "Gradient score"): the device's maps are the fp32 oracle's on all 152 planes that
have one (1.00 x its rel-L2 error, 3.7e-9 .. 8.4e-8, and 1.00 x its largest absolute error);
the 190 derived values sit 0 .. 6.4e-8 from the fp64 oracle, equal to e32 and at most 0.067 of
their bar.

The shapes are the smallest at which the kernel can go wrong: one position; one row of
positions over several column tiles; a ragged plane (W % 4 != 0: the scalar path); one position
more than the 16 x 64 rectangle a workgroup owns, both ways, and one pixel row more without a
position (the 16-byte path with a partial tile); the training tile; and one 256 x 256 case."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gradient_oracle as go  # noqa: E402
from srmi import _lib  # noqa: E402
from srmi._lib import ptr, stream_handle  # noqa: E402
from srmi.distribution import DistributionScore, contingency  # noqa: E402
from srmi.gradient import GRADIENT_TILE, GradientScore  # noqa: E402
from test_gpu_ssim_loss import dev, nbits, sid  # noqa: E402

TILE_H, TILE_W = GRADIENT_TILE  # checked against the library by test_gradient_oracle.py
SHAPES = [(2, 3, 3), (2, 3, 300), (3, 12, 75), (2, TILE_H + 2, TILE_W + 2), (2, TILE_H + 1, TILE_W + 4),
          (4, 192, 192), (2, 256, 256)]
KINDS = ["zero", "k290", "nan", "allnan", "equal"]
SPACING = (2.0, 0.5)
U = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def fields(shape, kind):
    """(pred, truth) [C, H, W] fp32.  zero: a smooth truth plus noise at mean 0, pred = truth +
    noise; k290: the same at 290 +- 1.5 with a prediction of another mean and gain; nan: zero
    with scattered NaN / Inf in both, some on the plane's corners and on the seams of the
    workgroups' rectangles; allnan: zero with the LAST truth plane all NaN; equal: pred ==
    truth."""
    n, H, W = shape
    rng = np.random.default_rng(900 + 10 * SHAPES.index(shape) + KINDS.index(kind))
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
    p.setflags(write=False)
    t.setflags(write=False)
    return p, t


def scatter_nonfinite(p, t, rng):
    """NaN / Inf into p and t [n, H, W]: scattered, and on corners and workgroup seams."""
    n, H, W = p.shape
    m = max(1, H * W // 300)
    for k in range(n):
        for arr, val in ((p, np.nan), (t, np.nan), (t, np.inf), (p, -np.inf)):
            idx = rng.choice(H * W, m, replace=False)
            arr[k].reshape(-1)[idx] = val
    if H * W > 9:
        p[0, 0, 0] = np.nan
        t[-1, H - 1, W - 1] = np.inf
        for ys in range(TILE_H, H, TILE_H):   # on and beside a horizontal seam
            t[0, ys, W // 2] = np.nan
            p[-1, ys - 1, W // 3] = np.nan
        for xs in range(TILE_W, W, TILE_W):   # and a vertical one
            p[0, H // 2, xs] = np.inf
            t[-1, H // 3, xs - 1] = np.nan


@functools.lru_cache(maxsize=None)
def oracle_pair(shape, kind):
    p, t = fields(shape, kind)
    return go.score(p, t, SPACING), go.score(p, t, SPACING, dtype=np.float32)


def measure(p, t, maps=True, spacing=SPACING, fill=0xFF):
    d = dev()
    gs = GradientScore(p.shape, spacing, maps, device=d)
    gs.workspace.fill_(fill)
    res = gs.measure(torch.tensor(p, device=d), torch.tensor(t, device=d))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in res.items()}


@functools.lru_cache(maxsize=None)
def plain(shape, kind):
    return measure(*fields(shape, kind))


def floors(o64):
    """The floor of every derived value, from the fp64 oracle's sums (see the module docstring)."""
    n = np.maximum(o64["count"], 1)
    rms = np.sqrt(2.0 * (o64["sum_pred2"] + o64["sum_truth2"]) / n)
    return dict(mean_pred=7 * U * np.abs(o64["mean_pred"]), mean_truth=7 * U * np.abs(o64["mean_truth"]),
                sharpness=14 * U * np.abs(o64["sharpness"]), rmse_mag=7 * U * rms, rmse_vec=7 * U * rms,
                cosine=28 * U * np.ones_like(rms))


# ------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_score_matches_the_oracle(shape, kind):
    p, t = fields(shape, kind)
    o64, o32 = oracle_pair(shape, kind)
    res = plain(shape, kind)
    tag = f"{sid(shape)} {kind}"
    n, H, W = shape
    full = (H - 2) * (W - 2)
    assert res["count"].dtype == np.int64 and np.array_equal(res["count"], o64["count"])
    if kind in ("zero", "k290", "equal"):
        assert (o64["count"] == full).all()
    if kind == "allnan":
        assert o64["count"][-1] == 0 and o64["count"][0] == full
    if kind == "nan" and H * W > 9:
        assert (o64["count"] < full).all()
    live = o64["count"] > 0
    fl = floors(o64)
    for key in go.STATS:
        got = res[key]
        assert got.dtype == np.float64
        assert np.isnan(got[~live]).all()
        if kind == "equal" and key in ("rmse_mag", "rmse_vec"):
            assert (got[live] == 0).all()
            continue
        if not live.any():
            continue
        e32 = np.abs(o32[key] - o64[key])[live]
        err = np.abs(got - o64[key])[live]
        bar = 10.0 * e32 + fl[key][live]
        print(f"{tag}: {key} {got[live]} off by {err.max():.3e}, e32 {e32.max():.3e}, worst {float((err / bar).max()):.3f} "
              f"of its bar")
        assert (err <= bar).all(), key
    assert np.isnan(res["sums"][~live]).all()
    for i, key in enumerate(go.SUMS):  # the sums the derived values were formed from, to the same bars
        if live.any():
            got, ref = res["sums"][live, i], o64[key][live]
            scale = 28 * U * np.maximum(np.abs(ref), (o64["sum_pred2"] + o64["sum_truth2"])[live])
            assert (np.abs(got - ref) <= 10.0 * np.abs(o32[key] - o64[key])[live] + scale).all(), key
    if kind == "equal":
        assert (res["sharpness"][live] == 1).all() and np.abs(res["cosine"][live] - 1).max() <= 28 * U
    # the maps, plane by plane: the NaN pattern equal
    for key in ("gmag_pred", "gmag_truth"):
        m, m64, m32 = res[key], o64[key], o32[key]
        assert m.dtype == np.float32 and np.array_equal(np.isnan(m), np.isnan(m64))
        assert not np.isinf(m).any()
        for k in range(n):
            if not live[k]:
                continue
            ok = ~np.isnan(m64[k])
            ref = m64[k][ok]
            e_l2 = np.linalg.norm(m32[k][ok] - ref) / np.linalg.norm(ref)
            e_max = np.abs(m32[k][ok] - ref).max()
            d_l2 = np.linalg.norm(m[k][ok] - ref) / np.linalg.norm(ref)
            d_max = np.abs(m[k][ok] - ref).max()
            print(f"{tag} {key} plane {k}: rel-L2 fp32 oracle {e_l2:.3e}, device {d_l2:.3e} ({d_l2 / e_l2:.2f} x); max-abs "
                  f"fp32 oracle {e_max:.3e}, device {d_max:.3e} ({d_max / e_max:.2f} x)")
            assert d_l2 <= 10.0 * e_l2 and d_max <= 10.0 * e_max


def test_analytic_planes():
    """f = alpha x + beta y: gx = alpha / dx, gy = beta / dy, in fp32 exactly for these slopes."""
    H, W = 21, 70
    y, x = np.mgrid[:H, :W].astype(np.float64)
    ap, bp, at, bt = 0.5, 0.25, 0.125, -0.75
    p = (ap * x + bp * y)[None].astype(np.float32)
    t = (at * x + bt * y + 3.0)[None].astype(np.float32)
    res = measure(p, t)
    gp, gt = np.array([ap / SPACING[1], bp / SPACING[0]]), np.array([at / SPACING[1], bt / SPACING[0]])
    want = dict(mean_pred=np.linalg.norm(gp), mean_truth=np.linalg.norm(gt),
                sharpness=np.linalg.norm(gp) / np.linalg.norm(gt), rmse_vec=np.linalg.norm(gp - gt),
                rmse_mag=abs(np.linalg.norm(gp) - np.linalg.norm(gt)),
                cosine=gp @ gt / (np.linalg.norm(gp) * np.linalg.norm(gt)))
    assert res["count"][0] == (H - 2) * (W - 2)
    for key, ref in want.items():
        print(f"analytic planes: {key} {res[key][0]:.9f} closed form {ref:.9f}")
        assert abs(res[key][0] - ref) <= 4 * U * max(abs(ref), np.linalg.norm(gp) + np.linalg.norm(gt)), key


# ------------------------------------------------------------- 2. determinism, options
@pytest.mark.parametrize("shape,kind", [(SHAPES[2], "nan"), (SHAPES[4], "k290"), (SHAPES[5], "nan")],
                         ids=["12x75 nan", "17x68 k290", "192 nan"])
def test_bit_identical_runs_workspace_contents_and_without_maps(shape, kind):
    p, t = fields(shape, kind)
    a = plain(shape, kind)
    for other in (measure(p, t), measure(p, t, fill=0x00), measure(p, t, maps=False)):
        for key in ("count", "sums") + go.STATS:
            assert np.array_equal(other[key].view(np.int64), a[key].view(np.int64)), key
    assert "gmag_pred" not in measure(p, t, maps=False)
    # one map alone, and buffers that are not 16-byte aligned (the scalar path): the same bits
    d = dev()
    lib = _lib.load()
    Cn, H, W = shape
    gs = GradientScore(shape, SPACING, True, device=d)
    buf = torch.zeros(2 * Cn * H * W + 2, device=d)
    off = torch.tensor(p, device=d).reshape(-1)
    pa = buf[1:1 + Cn * H * W]
    pa.copy_(off)
    td = torch.tensor(t, device=d)
    gs.gmag_truth.fill_(-7.0)
    rc = lib.srmi_gradient(ptr(pa), ptr(td), Cn, H, W, gs.inv_dy, gs.inv_dx, ptr(gs.workspace), gs.workspace.numel(),
                           ptr(gs.count), ptr(gs.sums), ptr(gs.stats), ptr(gs.gmag_pred), None, stream_handle())
    torch.cuda.synchronize()
    assert rc == 0
    assert np.array_equal(gs.sums.cpu().numpy().view(np.int64), a["sums"].view(np.int64))
    assert np.array_equal(nbits(gs.gmag_pred.cpu().numpy()), nbits(a["gmag_pred"]))
    assert (gs.gmag_truth == -7.0).all()


def test_the_launches_are_capturable_and_replay_on_new_inputs():
    d = dev()
    shape = SHAPES[4]
    p, t = (torch.tensor(v, device=d) for v in fields(shape, "nan"))
    p2 = (p + 0.1 * torch.arange(p.shape[-1], device=d)).contiguous()
    gs = GradientScore(shape, SPACING, True, device=d)
    pa = p.clone()
    gs.measure(pa, t)  # warm-up outside capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(device=d)
    s.wait_stream(torch.cuda.current_stream(d))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            gs.measure(pa, t)
    torch.cuda.current_stream(d).wait_stream(s)
    pa.copy_(p2)
    gs.stats.fill_(-7.0)
    g.replay()
    torch.cuda.synchronize()
    eager = measure(p2.cpu().numpy(), t.cpu().numpy())
    assert np.array_equal(gs.stats.cpu().numpy().view(np.int64),
                          np.stack([eager[k] for k in go.STATS], axis=1).view(np.int64))
    assert np.array_equal(nbits(gs.gmag_pred.cpu().numpy()), nbits(eager["gmag_pred"]))
    assert not np.array_equal(eager["mean_pred"], plain(shape, "nan")["mean_pred"])  # the inputs do differ


# ----------------------------------------------------------- 3. refused arguments
def test_refused_arguments_launch_nothing():
    lib = _lib.load()
    d = dev()
    E = _lib.SRMI_ERR_ARG
    Cn, H, W = 2, 20, 24
    n = C.c_size_t(0)
    wsz = lib.srmi_gradient_workspace
    assert wsz(Cn, H, W, C.byref(n)) == 0 and n.value > 0
    nbytes = n.value
    for bad in ((Cn, 2, W), (Cn, H, 2), (0, H, W), (-1, H, W), (1, 1 << 16, 1 << 15)):
        assert wsz(*bad, C.byref(n)) == E, bad
    assert wsz(1, 4096, 4096, C.byref(n)) == 0
    assert wsz(Cn, H, W, None) == E
    p, t = torch.randn(Cn, H, W, device=d), torch.randn(Cn, H, W, device=d)
    ws = torch.full((nbytes + 16,), 0x5A, dtype=torch.uint8, device=d)
    count = torch.full((Cn,), -7, dtype=torch.int64, device=d)
    sums = torch.full((Cn, 7), -7.0, dtype=torch.float64, device=d)
    stats = torch.full((Cn, 6), -7.0, dtype=torch.float64, device=d)
    gp, gt = torch.full((Cn, H, W), -7.0, device=d), torch.full((Cn, H, W), -7.0, device=d)
    st = stream_handle()
    nan, inf = float("nan"), float("inf")
    ok = dict(pred=ptr(p), truth=ptr(t), C=Cn, H=H, W=W, idy=1.0, idx=1.0, ws=ptr(ws), nbytes=nbytes, count=ptr(count),
              sums=ptr(sums), stats=ptr(stats), gp=ptr(gp), gt=ptr(gt))
    for change in (dict(H=2), dict(W=2), dict(C=0), dict(idy=0.0), dict(idy=-1.0), dict(idy=nan), dict(idy=inf),
                   dict(idx=0.0), dict(idx=-2.0), dict(idx=nan), dict(idx=inf), dict(pred=None), dict(truth=None),
                   dict(ws=None), dict(count=None), dict(sums=None), dict(stats=None), dict(nbytes=nbytes - 1),
                   dict(ws=ptr(ws) + 8)):
        a = dict(ok, **change)
        assert lib.srmi_gradient(a["pred"], a["truth"], a["C"], a["H"], a["W"], a["idy"], a["idx"], a["ws"], a["nbytes"],
                                 a["count"], a["sums"], a["stats"], a["gp"], a["gt"], st) == E, change
    torch.cuda.synchronize()
    assert (count == -7).all() and (sums == -7.0).all() and (stats == -7.0).all()
    assert (gp == -7.0).all() and (gt == -7.0).all() and (ws == 0x5A).all()
    # the Python layer refuses before anything is allocated
    for kw in (dict(spacing=(0.0, 1.0)), dict(spacing=(1.0, nan)), dict(spacing=(1.0, -1.0)), dict(spacing=1.0)):
        with pytest.raises(ValueError, match="spacing"):
            GradientScore((Cn, H, W), device=d, **kw)
    with pytest.raises(ValueError, match="the window"):
        GradientScore((Cn, 2, W), device=d)
    gs = GradientScore((Cn, H, W), device=d)
    with pytest.raises(ValueError, match="pred"):
        gs.measure(p[:, :-1], t)


# ------------------------------------------------------- 4. RegionSuperResolver
@functools.lru_cache(maxsize=None)
def region_scores():
    """One small land region through score, score_gradient (maps, distribution) once; shared."""
    from srmi.superres import RegionSuperResolver
    from test_gpu_inference import _small_rcan
    d = dev()
    spec, _, flat = _small_rcan()
    rng = np.random.RandomState(63)
    f0 = rng.randn(1, 160, 224)
    hr = ((f0 + np.roll(f0, 1, 1) + np.roll(f0, 1, 2)) * 2 + 5).astype(np.float32)
    hr[0, 40:72, 100:140] = np.nan  # land on whole LR pixels
    hr_d = torch.tensor(hr, device=d)
    rs = RegionSuperResolver(spec, flat.to(d), (1, 40, 56), tile_lr=(16, 32), overlap=(4, 4), land=True, device=d)
    images, losses = rs.score(hr_d)
    base = {k: v.clone() for k, v in images.items()}, {k: v.clone() for k, v in losses.items()}
    dcfg = dict(bins=64, joint=8)
    images, losses, grad = rs.score_gradient(hr_d, spacing=SPACING, distribution=dcfg)
    torch.cuda.synchronize()
    return rs, hr_d, base, images, losses, grad, dcfg


def test_score_gradient_images_and_losses_are_scores_bits():
    from test_gpu_ssim_loss import bits
    rs, hr_d, (images0, losses0), images, losses, grad, _ = region_scores()
    assert set(images) == set(images0) and set(losses) == set(losses0)
    for k in images0:
        assert torch.equal(bits(images[k]), bits(images0[k])), k
    for k in losses0:
        assert torch.equal(bits(losses[k]), bits(losses0[k])), k
    assert set(grad) == {"model", "interpolated"}
    hr = hr_d.cpu().numpy()
    for name in grad:
        ref = go.score(images[name].cpu().numpy(), hr, SPACING, dtype=np.float32)
        g = grad[name]
        assert np.array_equal(g["count"].cpu().numpy(), ref["count"]) and (ref["count"] > 0).all()
        assert (ref["count"] < 158 * 222).all()  # the coast costs positions
        assert np.array_equal(np.isnan(g["gmag_truth"].cpu().numpy()), np.isnan(ref["gmag_truth"]))
        sharp = g["sharpness"].cpu().numpy()
        print(f"score_gradient {name}: count {ref['count']}, sharpness {sharp}, cosine {g['cosine'].cpu().numpy()}")
        assert np.abs(sharp - ref["sharpness"]).max() <= 1e-6 * np.abs(ref["sharpness"]).max()
    # the scorers are cached per argument key; without maps or distribution no map is returned
    key_count = len(rs._gradient)
    _, _, again = rs.score_gradient(hr_d, spacing=SPACING, distribution=dict(bins=64, joint=8))
    assert len(rs._gradient) == key_count
    _, _, bare = rs.score_gradient(hr_d, spacing=SPACING)
    torch.cuda.synchronize()
    assert len(rs._gradient) == key_count + 1 and "gmag_pred" not in bare["model"] and "distribution" not in bare["model"]
    assert torch.equal(bare["model"]["sums"], again["model"]["sums"])
    with pytest.raises(ValueError, match="unknown keys"):
        rs.score_gradient(hr_d, distribution=dict(bin=3))
    with pytest.raises(ValueError, match="spacing"):
        rs.score_gradient(hr_d, spacing=(0.0, 1.0))


def test_score_gradient_distribution_equals_distribution_score_by_hand():
    rs, hr_d, _, images, losses, grad, dcfg = region_scores()
    d = dev()
    for name in ("model", "interpolated"):
        g = grad[name]
        ds = DistributionScore(tuple(g["gmag_pred"].shape), dcfg["bins"], dcfg["joint"], device=d)
        by_hand = ds.measure(g["gmag_pred"], g["gmag_truth"])
        torch.cuda.synchronize()
        for key, v in by_hand.items():
            a, b = g["distribution"][key].cpu().numpy(), v.cpu().numpy()
            assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), (name, key)
        assert np.array_equal(g["distribution"]["count"].cpu().numpy(), g["count"].cpu().numpy())
        table = contingency(g["distribution"]["joint"], dcfg["joint"] // 2)
        print(f"score_gradient {name}: fronts above the middle of the truth's range: "
              f"{ {k: np.asarray(v).tolist() for k, v in table.items()} }")
