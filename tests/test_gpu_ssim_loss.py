"""The SSIM loss term on the HIP path: srmi_ssim_loss_* / srmi.ssim.SSIMLoss and
FusedTrainer(ssim=...) against the oracle (tests/ssim_loss_oracle.py).

Bars of the kernel tests.  The device works in fp32, so it is held to the error of the SAME
arithmetic done in numpy on the very case under test (the rule of tests/test_gpu_ssim.py):
  * e32 is the largest per-position difference between the fp32 and the fp64 oracle's ssim.
    Per plane |parts / n - the fp64 oracle's| <= 10 e32 + 2^-23 (parts is rounded to fp32 by the
    ABI, 2^-24 of a mean that is at most 1, and the term once more); L_ssim takes the same bar.
  * The gradient of a plane may be 10 x the fp32 closed-form oracle's own rel-L2 error from
    fp64 off, and 10 x its largest absolute error, no floor.
  * cparts, Nused and 1 / Nused are exact.
Every test prints its figures before it asserts.  Measured on an MI355X over the 50 cases, 45
of them with used positions (DESIGN.md "SSIM loss"): e32 4.1e-8 .. 6.1e-6 with the plane means
2.7e-9 .. 1.1e-7 off, at most 0.09 of their bar; the gradient of the 103 planes that have one at
0.37 .. 2.45 x the fp32 oracle's rel-L2 error and 0.29 .. 3.29 x its largest absolute error.

The shapes are the smallest at which the kernels can go wrong: one position; one row of
positions over several column tiles; a ragged plane; one position more than the 24 x 64
rectangle a workgroup owns, both ways; and the training tile.

Bars of the trainer tests: those of tests/test_gpu_spectral_loss.py, named at each test."""
import ctypes as C
import functools
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import land_train_oracle as lt  # noqa: E402
import ssim_loss_oracle as slo  # noqa: E402
import ssim_oracle as so  # noqa: E402
import test_gpu_model  # noqa: E402
from oracle import rcan_oracle as ro  # noqa: E402
from srmi import _lib  # noqa: E402
from srmi._lib import ptr, stream_handle  # noqa: E402
from srmi.engine import param_table  # noqa: E402
from srmi.ssim import SSIMLoss, SSIMScore  # noqa: E402
from srmi.trainer import FusedTrainer  # noqa: E402
from test_gpu_model import flat_from_model, rel_l2  # noqa: E402
from test_gpu_spectral_loss import SPECTRAL, init_flat, rcan_spec  # noqa: E402

SHAPES = [(1, 11, 11), (2, 11, 300), (3, 12, 75), (2, 35, 75), (4, 192, 192)]
KINDS = ["zero", "k290", "nan", "allnan", "const"]
RANGES = [None, 20.0]
BASE = 0.75
KEYS = ("parts", "cparts", "ssim4", "total", "dy")


def sid(s):
    return "x".join(map(str, s))


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def bits(t):
    return t.contiguous().view(torch.int32)


def nbits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def shape4(shape):
    n, H, W = shape
    return ((2, 2) if n == 4 else (n, 1)) + (H, W)


@functools.lru_cache(maxsize=None)
def fields(shape, kind):
    """(pred, target) [N, C, H, W] fp32.  zero: a smooth truth plus noise at mean 0, pred = truth +
    noise; k290: the same at 290 +- 1.5 with a prediction of another mean and gain; nan: zero with
    scattered NaN / Inf in both; allnan / const: zero with the LAST target plane all NaN / constant."""
    n, H, W = shape
    rng = np.random.default_rng(500 + 10 * SHAPES.index(shape) + KINDS.index(kind))
    y, x = np.mgrid[:H, :W]
    t = np.zeros((n, H, W))
    for k in range(n):
        ph = rng.uniform(0, 2 * np.pi, 3)
        t[k] = (np.sin(0.21 * y + ph[0]) * np.cos(0.13 * x + ph[1]) + 0.5 * np.sin(0.05 * (x + y) + ph[2])
                + 0.3 * rng.standard_normal((H, W)))
    noise = 0.3 * rng.standard_normal((n, H, W))
    if kind == "k290":
        p, t = 290.4 + 1.5 * (0.8 * t + noise), 290.0 + 1.5 * t
    else:
        p = t + noise
    p, t = p.astype(np.float32), t.astype(np.float32)
    if kind == "nan":
        m = max(1, H * W // 600)
        for k in range(n):
            for arr, val in ((p, np.nan), (t, np.nan), (t, np.inf)):
                idx = rng.choice(H * W, m, replace=False)
                arr[k].reshape(-1)[idx] = val
    if kind == "allnan":
        t[-1] = np.nan
    if kind == "const":
        t[-1] = 2.5
    p, t = p.reshape(shape4(shape)), t.reshape(shape4(shape))
    p.setflags(write=False)
    t.setflags(write=False)
    return p, t


@functools.lru_cache(maxsize=None)
def oracle_pair(shape, kind, dr):
    """(the fp64 oracle, the fp32 oracle, e32 of the ssim map) on this very case."""
    p, t = fields(shape, kind)
    o64, o32 = slo.loss_and_grad(p, t, dr), slo.loss_and_grad(p, t, dr, dtype=np.float32)
    assert np.array_equal(np.isnan(o32["ssim"]), np.isnan(o64["ssim"]))
    d = np.abs(o32["ssim"].astype(np.float64) - o64["ssim"])
    e32 = float(np.nanmax(d)) if np.isfinite(d).any() else 0.0
    return o64, o32, e32


def run(p, t, dr=None, weight=1.0, dy0=None, splits=None, base=BASE, fill=0xFF):
    """numpy p, t [N, C, H, W] -> dict of numpy results; dy0: what dy holds before add_dy (zeros
    when None); splits: tile ranges the batch goes through parts / add_dy in; fill: what the
    workspace holds before (it need not be initialised)."""
    d = dev()
    N = p.shape[0]
    sl = SSIMLoss(p.shape, weight, dr, device=d)
    sl.workspace.fill_(fill)
    sl.gparts.fill_(-7.0)
    pd, td = torch.tensor(p, device=d), torch.tensor(t, device=d)
    dy = torch.zeros(p.shape, device=d) if dy0 is None else torch.tensor(dy0, device=d)
    b = torch.tensor([base], device=d)
    splits = splits or [(0, N)]
    for i, j in splits:
        sl.parts(pd[i:j], td[i:j], rows=i)
    sl.finalize(b)
    for i, j in splits:
        sl.add_dy(dy[i:j], pd[i:j], td[i:j], rows=slice(i, j))
    torch.cuda.synchronize()
    parts, cparts = sl.views()
    Cn = p.shape[1]
    return dict(parts=parts.cpu().numpy().reshape(N, Cn), cparts=cparts.cpu().numpy().reshape(N, Cn),
                ssim4=sl.ssim4.cpu().numpy(), total=sl.total.cpu().numpy(), dy=dy.cpu().numpy(),
                base=b.cpu().numpy())


@functools.lru_cache(maxsize=None)
def plain_run(shape, kind, dr):
    return run(*fields(shape, kind), dr)


def same_bits(a, b):
    for key in KEYS:
        assert np.array_equal(nbits(a[key]), nbits(b[key])), key


# ------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("dr", RANGES, ids=["range_target", "range_20"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_parts_counts_term_and_gradient_match_the_oracle(shape, kind, dr):
    p, t = fields(shape, kind)
    o64, o32, e32 = oracle_pair(shape, kind, dr)
    res = plain_run(shape, kind, dr)
    tag = f"{sid(shape)} {kind} L={dr}"
    n = o64["counts"]
    live = n > 0
    if kind in ("zero", "k290"):
        assert (n == (shape[1] - 10) * (shape[2] - 10)).all()
    if kind == "allnan" or (kind == "const" and dr is None):
        assert n.reshape(-1)[-1] == 0 and (shape[0] == 1 or n.reshape(-1)[0] > 0)
    if kind == "const" and dr is not None:
        assert live.all()
    if kind == "nan" and shape[0] > 1:
        assert (n < (shape[1] - 10) * (shape[2] - 10)).any()
    assert np.array_equal(res["cparts"], n.astype(np.float32))
    assert (nbits(res["parts"])[~live] == 0).all()
    bar = 10.0 * e32 + 2.0 ** -23
    if live.any():
        err = np.abs(res["parts"].astype(np.float64)[live] / n[live] - o64["parts"][live] / n[live])
        print(f"{tag}: e32 {e32:.3e}, plane means off by {float(err.max()):.3e} ({float(err.max()) / bar:.2f} of the bar)")
        assert (err <= bar).all()
    # the term
    s4 = res["ssim4"]
    if o64["nused"]:
        assert s4[1] == o64["nused"] and nbits(s4[2]) == nbits(np.float32(1.0 / o64["nused"]))
        lerr = abs(float(s4[3]) - o64["loss"])
        print(f"{tag}: L_ssim {s4[3]:.8f} oracle {o64['loss']:.8f} off by {lerr:.3e} ({lerr / bar:.2f} of the bar)")
        assert lerr <= bar and abs(float(s4[0]) - o64["S"]) <= bar * o64["nused"]
    else:
        assert (nbits(s4) == 0).all()
    # total = fma(weight, L_ssim, base): the exact product, one rounding
    assert nbits(res["total"])[0] == nbits(np.float32(np.float64(np.float32(BASE)) + np.float64(s4[3])))[0]
    assert res["base"][0] == np.float32(BASE)  # only read
    # the gradient, plane by plane
    H, W = shape[1:]
    g64, g32 = o64["grad"].reshape(-1, H, W), o32["grad"].reshape(-1, H, W)
    dy = res["dy"].reshape(-1, H, W).astype(np.float64)
    assert np.isfinite(res["dy"]).all()
    for k in range(shape[0]):
        nrm = np.linalg.norm(g64[k])
        if not live.reshape(-1)[k] or not o64["nused"]:
            assert nrm == 0 and (nbits(res["dy"].reshape(-1, H, W)[k]) == 0).all()
            continue
        e_l2, e_max = np.linalg.norm(g32[k] - g64[k]) / nrm, np.abs(g32[k] - g64[k]).max()
        d_l2, d_max = np.linalg.norm(dy[k] - g64[k]) / nrm, np.abs(dy[k] - g64[k]).max()
        print(f"{tag} plane {k}: gradient rel-L2 fp32 oracle {e_l2:.3e}, device {d_l2:.3e} ({d_l2 / e_l2:.2f} x); "
              f"max-abs fp32 oracle {e_max:.3e}, device {d_max:.3e} ({d_max / e_max:.2f} x)")
        assert d_l2 <= 10.0 * e_l2 and d_max <= 10.0 * e_max
    # a pixel that is not finite in both takes nothing
    assert (nbits(res["dy"])[~o64["fin"]] == 0).all()


# ----------------------------------------------------------- 2. into a random dy
@pytest.mark.parametrize("shape,kind", [(SHAPES[1], "zero"), (SHAPES[3], "nan"), (SHAPES[4], "k290")],
                         ids=["11x300", "35x75 nan", "192 k290"])
def test_add_dy_adds_to_what_dy_holds(shape, kind):
    p, t = fields(shape, kind)
    rng = np.random.default_rng(7)
    dy0 = (1e-3 * rng.standard_normal(p.shape)).astype(np.float32)
    dy0.flat[::5] = -0.0
    res = run(p, t, dy0=dy0)
    g = plain_run(shape, kind, None)["dy"].astype(np.float64)  # 0 + the gradient: the gradient, rounded once
    want = dy0.astype(np.float64) + g
    # dy = fma(scale, sum, dy0): the rounding of g (not made here) and the rounding of the result
    U = 2.0 ** -24
    err = np.abs(res["dy"].astype(np.float64) - want)
    print(f"{sid(shape)} {kind}: largest error {float((err / (U * (np.abs(g) + np.abs(want)) + 1e-300)).max()):.3f} of the bar")
    assert (err <= U * (np.abs(g) + np.abs(want))).all()
    assert np.abs(g).max() > 0


# ------------------------------------------------------------------ 3. weight 0
@pytest.mark.parametrize("shape,kind", [(SHAPES[2], "nan"), (SHAPES[4], "zero")], ids=["12x75 nan", "192 zero"])
def test_weight_zero_leaves_dy_as_it_is(shape, kind):
    p, t = fields(shape, kind)
    rng = np.random.default_rng(8)
    dy0 = rng.standard_normal(p.shape).astype(np.float32)
    dy0.flat[::3] = -0.0
    dy0.flat[1::7] = np.nan
    res = run(p, t, weight=0.0, dy0=dy0)
    ref = plain_run(shape, kind, None)
    assert np.array_equal(nbits(res["dy"]), nbits(dy0))
    for key in ("parts", "cparts", "ssim4"):
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
    live = plain_run(shape, "nan", None)["cparts"] > 0
    assert live.any()
    # another NaN, and Inf for NaN: the same bits everywhere
    t2 = nbits(t).copy()
    t2[np.isnan(t)] = -4194304 + 0x54321
    t2 = t2.view(np.float32)
    p2 = np.where(np.isnan(p), np.float32(-np.inf), p)
    same_bits(run(p2, t2), plain_run(shape, "nan", None))


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_no_used_position_is_zero_not_nan(shape):
    p, t = (v.copy() for v in fields(shape, "zero"))
    t[:, :, ::8, ::8] = np.nan
    rng = np.random.default_rng(9)
    dy0 = rng.standard_normal(p.shape).astype(np.float32)
    dy0.flat[::3] = -0.0
    res = run(p, t, dy0=dy0)
    assert (res["cparts"] == 0).all() and (nbits(res["parts"]) == 0).all() and (nbits(res["ssim4"]) == 0).all()
    assert nbits(res["total"])[0] == nbits(np.float32(BASE))[0]
    assert np.array_equal(nbits(res["dy"]), nbits(dy0))


# ------------------------------------------------------------- 5. determinism
@pytest.mark.parametrize("kind", ["k290", "nan", "const"])
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_bit_identical_runs_plane_ranges_and_workspace_contents(shape, kind):
    p, t = fields(shape, kind)
    a = plain_run(shape, kind, None)
    same_bits(a, run(p, t))
    same_bits(a, run(p, t, fill=0x00))  # whatever the workspace held
    same_bits(a, run(p, t, fill=0x7F))
    N = p.shape[0]
    if N > 1:  # the batch in two calls over tile ranges, the later range first
        same_bits(a, run(p, t, splits=[(1, N), (0, 1)]))


# ------------------------------------------------------------ 6. chaining and the score
def test_from_parts_chains_onto_a_given_base():
    shape = SHAPES[3]
    p, t = fields(shape, "zero")
    ref = plain_run(shape, "zero", None)
    for base, weight in ((0.0, 1.0), (-3.5, 1.0), (1.2345678, 0.3), (1e-3, 2.5)):
        res = run(p, t, weight=weight, base=base)
        assert np.array_equal(nbits(res["ssim4"]), nbits(ref["ssim4"]))
        want = np.float32(np.float64(np.float32(base)) + np.float64(np.float32(weight)) * np.float64(res["ssim4"][3]))
        assert nbits(res["total"])[0] == nbits(want)[0], (base, weight)
        assert res["base"][0] == np.float32(base)
    # the gradient follows the weight
    res = run(p, t, weight=2.5)
    assert rel_l2(res["dy"], 2.5 * ref["dy"].astype(np.float64)) < 4 * 2.0 ** -24


@pytest.mark.parametrize("dr", RANGES, ids=["range_target", "range_20"])
@pytest.mark.parametrize("shape,kind", [(SHAPES[0], "k290"), (SHAPES[3], "k290"), (SHAPES[3], "nan"), (SHAPES[4], "zero")],
                         ids=["11x11", "35x75 k290", "35x75 nan", "192"])
def test_one_plane_is_one_minus_the_score(shape, kind, dr):
    p, t = fields(shape, kind)
    p, t = p.reshape(-1, *shape[1:])[:1], t.reshape(-1, *shape[1:])[:1]
    d = dev()
    sc = SSIMScore(p.shape, dr, device=d)
    m = sc.measure(torch.tensor(p, device=d), torch.tensor(t, device=d))
    res = run(p[None], t[None], dr)
    o64, o32 = so.ssim(p, t, dr), so.ssim(p, t, dr, dtype=np.float32)
    e32 = float(np.nanmax(np.abs(o32["map"].astype(np.float64) - o64["map"])))
    got, want = 1.0 - float(res["ssim4"][3]), float(m["ssim"][0])
    print(f"{sid(shape)} {kind} L={dr}: 1 - L_ssim {got:.8f}, the score {want:.8f}, apart {abs(got - want):.3e} "
          f"(bar {20 * e32 + 2.0 ** -22:.3e})")
    assert res["ssim4"][1] == float(m["nwin"][0]) > 0
    assert abs(got - want) <= 20.0 * e32 + 2.0 ** -22


# ------------------------------------------------------------------- capture
def test_the_launches_are_capturable_and_replay_on_new_inputs():
    d = dev()
    shape = SHAPES[3]
    p, t = (torch.tensor(v, device=d) for v in fields(shape, "nan"))
    p2 = (p + 0.1).contiguous()
    sl = SSIMLoss(p.shape, device=d)
    pa, dy, b = p.clone(), torch.zeros_like(p), torch.tensor([BASE], device=d)

    def stage():
        sl.parts(pa, t)
        sl.finalize(b)
        sl.add_dy(dy, pa, t)
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
    sl.ssim4.fill_(-7.0)
    g.replay()
    torch.cuda.synchronize()
    eager = run(p2.cpu().numpy(), t.cpu().numpy())
    assert np.array_equal(nbits(sl.ssim4.cpu().numpy()), nbits(eager["ssim4"])) and eager["ssim4"][1] > 0
    assert np.array_equal(nbits(dy.cpu().numpy()), nbits(eager["dy"]))
    assert np.array_equal(nbits(sl.total.cpu().numpy()), nbits(eager["total"]))
    assert not np.array_equal(eager["ssim4"], plain_run(shape, "nan", None)["ssim4"])  # the inputs do differ


# ----------------------------------------------------------- 7. refused arguments
def test_refused_arguments_launch_nothing():
    lib = _lib.load()
    d = dev()
    E = _lib.SRMI_ERR_ARG
    H, W = 24, 40
    n = C.c_size_t(0)
    wsz = lib.srmi_ssim_loss_workspace
    assert wsz(2, H, W, C.byref(n)) == 0 and n.value >= 2 * 3 * 14 * 30 * 4 and n.value % 32 == 0
    nbytes = n.value
    one = C.c_size_t(0)
    assert wsz(1, H, W, C.byref(one)) == 0 and 2 * one.value == nbytes  # plane by plane
    for bad in ((2, 10, W), (2, H, 10), (0, H, W), (-1, H, W), (1, 4096, 4097), (1, 11, (1 << 24) // 11 + 1)):
        assert wsz(*bad, C.byref(n)) == E, bad
    assert wsz(1, 4096, 4096, C.byref(n)) == 0
    assert wsz(2, H, W, None) == E
    p = torch.randn(2, 1, H, W, device=d)
    t = torch.randn(2, 1, H, W, device=d)
    ws = torch.full((nbytes + 16,), 0x5A, dtype=torch.uint8, device=d)
    parts, cparts = torch.full((2,), -7.0, device=d), torch.full((2,), -7.0, device=d)
    base = torch.full((1,), -7.0, device=d)
    s4, tot = torch.full((4,), -7.0, device=d), torch.full((1,), -7.0, device=d)
    dy = torch.full((2, 1, H, W), -7.0, device=d)
    st = stream_handle()
    nan, inf = float("nan"), float("inf")
    f = lib.srmi_ssim_loss_parts
    ok = dict(pred=ptr(p), target=ptr(t), nplanes=2, H=H, W=W, dr=0.0, parts=ptr(parts), cparts=ptr(cparts),
              ws=ptr(ws), nbytes=nbytes)
    for change in (dict(H=10), dict(W=10), dict(nplanes=0), dict(dr=nan), dict(dr=inf), dict(dr=-inf),
                   dict(pred=None), dict(target=None), dict(parts=None), dict(cparts=None), dict(ws=None),
                   dict(nbytes=nbytes - 1), dict(ws=ptr(ws) + 4), dict(H=4096, W=4097)):
        a = dict(ok, **change)
        assert f(a["pred"], a["target"], a["nplanes"], a["H"], a["W"], a["dr"], a["parts"], a["cparts"], a["ws"],
                 a["nbytes"], st) == E, change
    f = lib.srmi_ssim_loss_from_parts
    ok = dict(parts=ptr(parts), cparts=ptr(cparts), nplanes=2, weight=1.0, base=ptr(base), s4=ptr(s4), total=ptr(tot))
    for change in (dict(nplanes=0), dict(weight=-1.0), dict(weight=inf), dict(weight=nan), dict(parts=None),
                   dict(cparts=None), dict(base=None), dict(s4=None), dict(total=None)):
        a = dict(ok, **change)
        assert f(a["parts"], a["cparts"], a["nplanes"], a["weight"], a["base"], a["s4"], a["total"], st) == E, change
    f = lib.srmi_ssim_loss_dy
    ok = dict(ws=ptr(ws), nbytes=nbytes, pred=ptr(p), target=ptr(t), nplanes=2, H=H, W=W, weight=1.0, s4=ptr(s4),
              dy=ptr(dy))
    for change in (dict(H=10), dict(W=10), dict(nplanes=0), dict(weight=-1.0), dict(weight=nan), dict(weight=inf),
                   dict(ws=None), dict(pred=None), dict(target=None), dict(s4=None), dict(dy=None),
                   dict(nbytes=nbytes - 1), dict(ws=ptr(ws) + 8), dict(H=4096, W=4097)):
        a = dict(ok, **change)
        assert f(a["ws"], a["nbytes"], a["pred"], a["target"], a["nplanes"], a["H"], a["W"], a["weight"], a["s4"],
                 a["dy"], st) == E, change
    torch.cuda.synchronize()
    # nothing was launched: every output still holds what it was filled with
    assert (parts == -7.0).all() and (cparts == -7.0).all() and (s4 == -7.0).all() and (tot == -7.0).all()
    assert (dy == -7.0).all() and (ws == 0x5A).all() and (base == -7.0).all()
    # the Python layer says which value it refuses
    for kw, what in ((dict(weight=-1.0), "weight -1.0"), (dict(weight=nan), "weight nan"),
                     (dict(data_range=inf), "data_range inf")):
        with pytest.raises(ValueError, match=what):
            SSIMLoss((2, 1, H, W), device=d, **kw)
    with pytest.raises(ValueError, match="the window"):
        SSIMLoss((2, 1, 10, 48), device=d)
    with pytest.raises(ValueError, match="global batch"):
        SSIMLoss((2, 1, H, W), device=d, global_batch=1)


# ===================================================================== the trainer
SSIM = dict(weight=1.0)


# ------------------------------------------------- T1. weight 0 is the plain trainer
@pytest.mark.parametrize("loss_fn", ["l2", "charbonnier"])
@pytest.mark.parametrize("B,micro", [(2, 1), (4, 2)])
def test_weight_zero_trainer_is_the_plain_trainer(B, micro, loss_fn):
    """The parts and the finalise run, add_dy launches nothing, total = loss4[3] + 0 * L_ssim,
    and the backward takes the pixel loss's dy as it is: every bit of two steps is the plain
    trainer's."""
    spec = rcan_spec(1, 2)
    flat = init_flat(spec, 5)
    hr = torch.tensor(ro.synthetic_hr(B, 2, 192, 19), device=dev())
    res = []
    for ssim in (None, dict(weight=0.0)):
        tr = FusedTrainer(spec, B, (48, 48), device=dev(), params=flat, micro=micro, loss_fn=loss_fn, ssim=ssim)
        assert tr.micro == micro and (tr.ssim is None) == (ssim is None)
        rows = []
        for _ in range(2):
            out = tr.step(hr)
            torch.cuda.synchronize()
            assert set(out) == ({"loss", "interp_loss"} if ssim is None else
                                {"loss", "interp_loss", "pixel_loss", "ssim_loss"})
            rows.append((out["loss"].clone(), out["interp_loss"].clone(), tr.sr.clone(), tr.grads.clone(),
                         tr.params.clone()))
        if ssim is not None:
            assert torch.equal(bits(out["pixel_loss"]), bits(out["loss"])) and float(out["ssim_loss"]) > 0
        res.append(rows)
        del tr
    for k, (a, b) in enumerate(zip(*res)):
        for x, y, what in zip(a, b, ("loss", "interp_loss", "sr", "grads", "params")):
            assert torch.equal(bits(x), bits(y)), (k, what, float((x - y).abs().max()))
    assert np.isfinite(float(res[0][1][0]))


# --------------------------------------------------------- T2. / T4. against fp64
def ssim_drift_bounds(monkeypatch, model, hr, scale, g_ref, **kw):
    """test_gpu_model.drift_bounds itself (3 x the drift of the same fp64 step with bf16-rounded
    conv operands, + 1e-3) with the oracle step it runs the emulation through replaced by the
    one with the term(s), as test_gpu_spectral_loss.spectral_drift_bounds does."""
    monkeypatch.setattr(test_gpu_model, "oracle_grads", lambda m, h, s: slo.train_step(m, h, s, **kw)[:3])
    return test_gpu_model.drift_bounds(model, hr, scale, g_ref)


def used_positions(hr):
    """[B, C]: the used positions of every plane when the prediction is finite everywhere."""
    fin = np.isfinite(hr)
    return np.array([[(so.window_bad_count(~fin[b, c]) == 0).sum() for c in range(hr.shape[1])]
                     for b in range(hr.shape[0])])


def step_vs_oracle(monkeypatch, hr, loss_fn, land, spectral=None, consistent=0):
    d = dev()
    model = ro.RCANOracle(nchannels_in=2, nchannels_out=2, nlayers=2, nblocks=2, nfeatures=64, cbottleneck=2)
    ro.init_params_numpy(model, 22)
    spec = rcan_spec(2, 2)
    table = param_table(spec)
    flat = flat_from_model(model, table).to(d)
    model = model.double()
    kw = dict(loss_fn=loss_fn, ssim_cfg=SSIM, spectral_cfg=spectral, consistent=consistent, land=land)
    l_ref, _, g_ref, info = slo.train_step(model, hr, 4, **kw)
    bound = ssim_drift_bounds(monkeypatch, model, hr, 4, g_ref, **kw)
    tr = FusedTrainer(spec, 3, (48, 48), device=d, params=flat, loss_fn=loss_fn, land=land, ssim=SSIM,
                      spectral=spectral, consistent=consistent)
    hr_d = torch.tensor(hr, device=d)
    out = tr.step(hr_d)
    torch.cuda.synchronize()
    keys = [("loss", l_ref), ("pixel_loss", info["pixel_loss"]), ("ssim_loss", info["ssim_loss"])]
    if spectral is not None:
        keys.append(("spectral_loss", info["spectral_loss"]))
    assert set(out) == {k for k, _ in keys} | {"interp_loss"}
    for key, ref in keys:
        got = float(out[key])
        print(f"{loss_fn} land={land} spectral={spectral is not None} K={consistent}: {key} {got:.6f} oracle "
              f"{ref:.6f} rel {abs(got - ref) / ref:.2e} (bar 2e-3)")
        assert abs(got - ref) / ref < 2e-3, key
    assert float(tr.ssim.ssim4[1]) == info["nused"] == used_positions(hr).sum()
    assert info["ssim_loss"] > 0.1 * info["pixel_loss"]  # the term is a real share of the loss
    g = tr.grads.cpu()
    if consistent:
        # behind the layer the last conv's bias has an exact gradient of zero (a constant added to
        # the network's output is removed by the layer), where a relative distance is not defined:
        # test_gpu_consistency_train.check_grads is the composed step's bar, that tensor included
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
def test_ssim_trainer_step_vs_oracle(loss_fn, monkeypatch):
    """test_spectral_trainer_step_vs_oracle's bars: the losses 2e-3 relative, every gradient
    tensor within test_gpu_model.drift_bounds."""
    tr, _, info = step_vs_oracle(monkeypatch, ro.synthetic_hr(3, 2, 192, 21), loss_fn, False)
    assert info["nused"] == 3 * 2 * 182 * 182


@pytest.mark.parametrize("loss_fn", ["l2", "charbonnier"])
def test_ssim_land_trainer_step_vs_oracle(loss_fn, monkeypatch):
    hr = lt.land_batch(3, 2, 192, 21)
    lt.check_conditions(hr, 4)
    used = used_positions(hr)
    assert used.tolist() == [[33124, 33124], [16153, 16153], [16153, 16153]] and 182 * 182 == 33124
    tr, dy, info = step_vs_oracle(monkeypatch, hr, loss_fn, True)
    assert 0 < info["nused"] < 3 * 2 * 33124
    assert (dy[~np.isfinite(hr)].view(np.int32) == 0).all()  # +0.0f on land


def test_ssim_spectral_consistent_trainer_step_vs_oracle(monkeypatch):
    """All three together against the composed oracle, with the bars of
    test_consistent_spectral_trainer_step_vs_oracle: the SSIM term chains onto the spectral
    term's total, and its gradient enters before the layer's adjoint."""
    step_vs_oracle(monkeypatch, ro.synthetic_hr(3, 2, 192, 21), "l2", False, spectral=SPECTRAL, consistent=2)


# ------------------------------------------------------------- T3. the fp32 engine
def test_ssim_trainer_fp32_step_vs_oracle():
    """test_spectral_trainer_fp32_step_vs_oracle's bars: the losses and the output 1e-5 relative,
    every gradient tensor 1e-3 rel-L2."""
    d = dev()
    model = ro.RCANOracle(nchannels_in=2, nchannels_out=2, nlayers=2, nblocks=2, nfeatures=64, cbottleneck=2)
    ro.init_params_numpy(model, 23)
    spec = rcan_spec(2, 2, dtype="fp32")
    table = param_table(spec)
    hr = ro.synthetic_hr(3, 2, 192, 21)
    tr = FusedTrainer(spec, 3, (48, 48), device=d, params=flat_from_model(model, table).to(d), ssim=SSIM)
    l_ref, out_ref, g_ref, info = slo.train_step(model.double(), hr, 4, "l2", SSIM)
    out = tr.step(torch.tensor(hr, device=d))
    torch.cuda.synchronize()
    for key, ref in (("loss", l_ref), ("pixel_loss", info["pixel_loss"]), ("ssim_loss", info["ssim_loss"])):
        print(f"fp32: {key} {float(out[key]):.8f} oracle {ref:.8f} rel {abs(float(out[key]) - ref) / ref:.2e}")
        assert abs(float(out[key]) - ref) / ref < 1e-5, key
    assert rel_l2(tr.sr, out_ref) < 1e-5
    g = tr.grads.cpu()
    worst = max(rel_l2(g[off:off + n].view(shape), g_ref[name]) for name, off, n, shape in table)
    print(f"fp32 engine with the SSIM term: worst per-tensor grad rel-L2 {worst:.2e} (bar 1e-3)")
    assert worst < 1e-3


# -------------------------------------------------------- T5. micro-batch split
def test_ssim_micro_batch_split():
    """test_spectral_micro_batch_split's bars: the losses equal as floats (sums and counts in
    plane order), the gradients to 1e-5 rel-L2."""
    spec = rcan_spec(1, 2)
    flat = init_flat(spec, 5)
    hr = torch.tensor(lt.land_batch(4, 2, 192, 24), device=dev())
    res = []
    for micro in (1, 2):
        tr = FusedTrainer(spec, 4, (48, 48), device=dev(), params=flat, micro=micro, land=True, ssim=SSIM)
        out = tr.step(hr)
        torch.cuda.synchronize()
        res.append(([float(out[k]) for k in ("loss", "pixel_loss", "ssim_loss")], tr.grads.clone()))
        del tr
    (l1, g1), (l2, g2) = res
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
    tr = FusedTrainer(spec, b - a, (48, 48), device=d, params=flat, micro=2, info=info, land=True, ssim=SSIM)
    out = tr.step(hr_all[a:b].contiguous())
    torch.cuda.synchronize()
    q.put((rank, [float(out[k]) for k in ("loss", "pixel_loss", "ssim_loss")], tr.grads.cpu().numpy(),
           tr.params.cpu().numpy()))
    dist.destroy_process_group()


def test_ssim_dp_world2_matches_single_process():
    """test_spectral_dp_world2_matches_single_process's conventions and bars (gloo, both ranks
    on cuda:0; gradients 2e-4 rel-L2): the ranks' used counts differ; sums and counts go
    through one all-reduce."""
    import multiprocessing as mp
    hr_np = lt.land_batch(4, 2, 192, 25)
    used = used_positions(hr_np).sum(axis=1)
    assert used[:2].sum() == 98554 and used[2:].sum() == 64612
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
    tr = FusedTrainer(spec, 4, (48, 48), device=d, params=init_flat(spec, 5), micro=1, land=True, ssim=SSIM)
    out = tr.step(torch.tensor(hr_np, device=d))
    torch.cuda.synchronize()
    losses, g = [float(out[k]) for k in ("loss", "pixel_loss", "ssim_loss")], tr.grads.cpu().numpy()
    assert float(tr.ssim.ssim4[1]) == used.sum()
    for rank, l_r, g_r, p_r in res:
        assert l_r == losses, (rank, l_r, losses)
        assert np.linalg.norm(g_r - g) / np.linalg.norm(g) < 2e-4
    np.testing.assert_array_equal(res[0][3], res[1][3])  # replicas stay identical after Adam


# ------------------------------------------------------------------ T7. construction
@pytest.mark.parametrize("ssim,what", [
    (dict(weight=-0.5), "weight -0.5"), (dict(weight=float("nan")), "weight nan"),
    (dict(weight=float("inf")), "weight inf"), (dict(weight="1"), "weight '1'"),
    (dict(data_range=float("nan")), "data_range nan"), (dict(data_range=float("inf")), "data_range inf"),
    (dict(wieght=1.0), "wieght"), (dict(window=11), "window"), ([1.0], "a dict")])
def test_trainer_refuses_a_bad_ssim_config(ssim, what):
    with pytest.raises(ValueError, match=what):
        FusedTrainer(rcan_spec(1, 1), 2, (48, 48), device=dev(), ssim=ssim)
    # an HR tile below the window in either dimension, before anything is allocated
    with pytest.raises(ValueError, match="larger than the HR tile"):
        FusedTrainer(rcan_spec(1, 1, scale=2), 2, (4, 16), device=dev(), ssim=dict(weight=1.0))
    with pytest.raises(ValueError, match="larger than the HR tile"):
        FusedTrainer(rcan_spec(1, 1, scale=2), 2, (16, 4), device=dev(), ssim={})
