"""The spectral loss term on the HIP path: srmi_spectral_loss_* / srmi.spectra.SpectralLoss
and FusedTrainer(spectral=...) against the fp64 oracle (tests/spectral_loss_oracle.py).

Bars of the kernel tests.  The device transforms in fp32, so it is held to the error of the
SAME arithmetic done by a library: e32 is the error of the oracle run with complex64
transforms (scipy.fft) against the fp64 oracle on the very case under test -- for the parts
relative to the part, the largest over the planes, with the complex64 oracle's part rounded
to fp32 as the device's is (parts are fp32 by the ABI); for the gradient rel-L2 over the
batch.  The device may be 10 x e32 off, no floor.  S and L_spec are sums of the parts
(positive terms: the relative error of the sum is at most the largest of the terms') and
take the parts' bar.  Every test prints its figures before it asserts.  Measured on the
five cases and their coast forms: e32 of the parts 2.0e-8 .. 7.3e-8 with the device at 1.00 e32 (the same
fp32 value) on all but one case, 2.28 e32 there; e32 of the gradient 8.5e-8 .. 1.4e-7 with
the device at 1.13 .. 1.55 e32.

Case 1 holds a single job, so it cannot hold a used and a skipped one at once: the coast
test runs on cases 2 .. 5, and case 1 takes part in the all-jobs-skipped test.

Bars of the trainer tests: those of tests/test_gpu_land_train.py, named at each test."""
import functools
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import land_train_oracle as lt  # noqa: E402
import spectral_loss_oracle as slo  # noqa: E402
import test_gpu_model  # noqa: E402
from oracle import rcan_oracle as ro  # noqa: E402
from srmi import _lib  # noqa: E402
from srmi._lib import ptr, stream_handle  # noqa: E402
from srmi.engine import NetSpec, param_table  # noqa: E402
from srmi.spectra import SpectralLoss  # noqa: E402
from srmi.trainer import FusedTrainer, default_init_  # noqa: E402
from test_gpu_model import flat_from_model, rel_l2  # noqa: E402

# (planes, H, W, P, Q)
CASES = [(1, 16, 16, 16, 16), (3, 40, 56, 16, 12), (2, 48, 40, 32, 32), (4, 96, 80, 64, 32), (3, 192, 192, 64, 32)]
NWIN = {CASES[0]: 1, CASES[1]: 15, CASES[2]: 4, CASES[3]: 4, CASES[4]: 25}
IDS = ["x".join(map(str, c)) for c in CASES]
EPS = 1e-12
LOSS4 = (0.25, 1000.0, 0.5, 0.75)  # a finalised pixel loss: only [3] is read


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def bits(t):
    return t.contiguous().view(torch.int32)


def nbits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def shape_of(case):
    n, H, W = case[:3]
    return ((2, 2) if n == 4 else (n, 1)) + (H, W)


@functools.lru_cache(maxsize=None)
def white(case):
    """t = N(0, 1), p = t + 0.3 N(0, 1), fp32, a fixed seed per case."""
    rng = np.random.default_rng(300 + CASES.index(case))
    t = rng.standard_normal(shape_of(case)).astype(np.float32)
    p = (t + 0.3 * rng.standard_normal(shape_of(case))).astype(np.float32)
    return p, t


@functools.lru_cache(maxsize=None)
def coast(case):
    """white(case) with a coast through the target of every plane but the first
    (land_train_oracle.land_mask, cropped to the plane)."""
    p, t = white(case)
    N, C, H, W = t.shape
    t = t.copy().reshape(N * C, H, W)
    for k in range(1, N * C):
        t[k][lt.land_mask(max(H, W, 32), k)[:H, :W]] = np.nan
    return p, t.reshape(N, C, H, W)


def oracle_pair(p, t, P, Q):
    """(the fp64 oracle, e32 of the parts, e32 of the gradient)."""
    o64 = slo.loss_and_grad(p, t, P, Q, EPS)
    o32 = slo.loss_and_grad(p, t, P, Q, EPS, dtype="complex64")
    live = o64["counts"] > 0
    p32 = o32["parts"].astype(np.float32).astype(np.float64)
    e_parts = float((np.abs(p32 - o64["parts"])[live] / o64["parts"][live]).max())
    e_grad = float(np.linalg.norm(o32["grad"] - o64["grad"]) / np.linalg.norm(o64["grad"]))
    return o64, e_parts, e_grad


@functools.lru_cache(maxsize=None)
def white_oracle(case):
    return oracle_pair(*white(case), case[3], case[4])


@functools.lru_cache(maxsize=None)
def coast_oracle(case):
    return oracle_pair(*coast(case), case[3], case[4])


def run(p, t, P, Q, weight=1.0, dy0=None, eps=EPS, splits=None, loss4=LOSS4):
    """numpy p, t [N, C, H, W] -> dict of numpy results; dy0: what dy holds before add_dy
    (zeros when None); splits: tile ranges the batch goes through parts / add_dy in."""
    d = dev()
    N = p.shape[0]
    sl = SpectralLoss(p.shape, P, Q, eps, weight, device=d)
    sl.workspace.fill_(0xFF)  # need not be initialised: NaN patterns wherever it is read unwritten
    sl.gparts.fill_(-7.0)
    pd, td = torch.tensor(p, device=d), torch.tensor(t, device=d)
    dy = torch.zeros(p.shape, device=d) if dy0 is None else torch.tensor(dy0, device=d)
    l4 = torch.tensor(loss4, device=d)
    splits = splits or [(0, N)]
    for a, b in splits:
        sl.parts(pd[a:b], td[a:b], rows=a)
    sl.finalize(l4[3:4])
    for a, b in splits:
        sl.add_dy(dy[a:b], rows=slice(a, b))
    torch.cuda.synchronize()
    parts, cparts = sl.views()
    C = p.shape[1]
    return dict(parts=parts.cpu().numpy().reshape(N, C), cparts=cparts.cpu().numpy().reshape(N, C),
                spec4=sl.spec4.cpu().numpy(), total=sl.total.cpu().numpy(), dy=dy.cpu().numpy(),
                loss4=l4.cpu().numpy())


@functools.lru_cache(maxsize=None)
def white_run(case):
    return run(*white(case), case[3], case[4])


def check_against(res, o64, e_parts, e_grad, P, what):
    live = o64["counts"] > 0
    err = np.abs(res["parts"].astype(np.float64) - o64["parts"])[live] / o64["parts"][live]
    gerr = float(np.linalg.norm(res["dy"].astype(np.float64) - o64["grad"]) / np.linalg.norm(o64["grad"]))
    print(f"{what}: parts e32 {e_parts:.3e}, device {float(err.max()):.3e}, ratio {float(err.max()) / e_parts:.2f}; "
          f"gradient e32 {e_grad:.3e}, device {gerr:.3e}, ratio {gerr / e_grad:.2f}")
    assert np.array_equal(res["cparts"], o64["counts"].astype(np.float32))
    assert (res["parts"][~live] == 0).all()
    assert (err <= 10.0 * e_parts).all()
    assert gerr <= 10.0 * e_grad
    s4 = res["spec4"]
    s_err, l_err = abs(float(s4[0]) - o64["S"]) / o64["S"], abs(float(s4[3]) - o64["loss"]) / o64["loss"]
    print(f"{what}: S {s4[0]:.6f} oracle {o64['S']:.6f} rel {s_err:.3e}; L_spec {s4[3]:.8f} oracle "
          f"{o64['loss']:.8f} rel {l_err:.3e} (bar {10 * e_parts:.3e})")
    assert s4[1] == o64["nused"] and s4[2] == np.float32(1.0 / (o64["nused"] * P))
    assert s_err <= 10.0 * e_parts and l_err <= 10.0 * e_parts


# ------------------------------------------------------- 1.-3. against the oracle
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_parts_spec4_total_and_gradient_match_the_oracle(case):
    o64, e_parts, e_grad = white_oracle(case)
    res = white_run(case)
    assert o64["nused"] == case[0] * NWIN[case] and (o64["counts"] == NWIN[case]).all()
    check_against(res, o64, e_parts, e_grad, case[3], f"case {case}")
    # total = fma(weight, L_spec, loss4[3]): the exact product, one rounding
    l43, L64 = np.float64(np.float32(LOSS4[3])), res["spec4"].astype(np.float64)[3]
    assert nbits(res["total"])[0] == nbits(np.float32(l43 + L64))[0]
    assert np.array_equal(res["loss4"], np.array(LOSS4, np.float32))  # only read
    # the taper is 0 at its first point: no gradient on the first row and column
    assert (nbits(res["dy"][:, :, 0, :]) == 0).all() and (nbits(res["dy"][:, :, :, 0]) == 0).all()
    res2 = run(*white(case), case[3], case[4], weight=2.5)
    assert nbits(res2["total"])[0] == nbits(np.float32(l43 + 2.5 * res2["spec4"].astype(np.float64)[3]))[0]
    assert np.array_equal(nbits(res2["spec4"]), nbits(res["spec4"]))
    assert rel_l2(res2["dy"], 2.5 * res["dy"].astype(np.float64)) < 4 * 2.0 ** -24


# ----------------------------------------------------------- 4. into a random dy
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_add_dy_adds_to_what_dy_holds(case):
    rng = np.random.default_rng(7)
    dy0 = (1e-3 * rng.standard_normal(shape_of(case))).astype(np.float32)
    dy0.flat[::5] = -0.0
    res = run(*white(case), case[3], case[4], dy0=dy0)
    g = white_run(case)["dy"].astype(np.float64)  # 0 + the gradient: the gradient itself, rounded once
    want = dy0.astype(np.float64) + g
    # dy = fma(scale, sum, dy0): the rounding of g (not made here) and the rounding of the result
    U = 2.0 ** -24
    err = np.abs(res["dy"].astype(np.float64) - want)
    print(f"case {case}: largest error {float((err / (U * (np.abs(g) + np.abs(want)) + 1e-300)).max()):.3f} of the bar")
    assert (err <= U * (np.abs(g) + np.abs(want))).all()
    assert (nbits(res["dy"][:, :, 0, :]) == nbits(dy0[:, :, 0, :] + np.float32(0))).all()  # x + (+0)


# ------------------------------------------------------------------ 5. weight 0
@pytest.mark.parametrize("case", [CASES[1], CASES[3]], ids=[IDS[1], IDS[3]])
def test_weight_zero_leaves_dy_as_it_is(case):
    rng = np.random.default_rng(8)
    dy0 = rng.standard_normal(shape_of(case)).astype(np.float32)
    dy0.flat[::3] = -0.0
    dy0.flat[1::7] = np.nan
    res = run(*white(case), case[3], case[4], weight=0.0, dy0=dy0)
    assert np.array_equal(nbits(res["dy"]), nbits(dy0))
    assert np.array_equal(nbits(res["spec4"]), nbits(white_run(case)["spec4"]))
    assert nbits(res["total"])[0] == nbits(np.float32(LOSS4[3]))[0]


# ------------------------------------------------------------------- 6. p == t
@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[4]], ids=[IDS[0], IDS[1], IDS[4]])
def test_equal_planes_give_sqrt_eps_per_bin_and_a_zero_gradient(case):
    p, t = (v.copy() for v in white(case))
    k = p.shape[0] - 1
    p[k] = t[k]
    P = case[3]
    for eps in (EPS, 1e-6):
        res = run(p, t, P, case[4], eps=eps)
        want = np.float32(NWIN[case] * P * P * np.sqrt(np.float64(np.float32(eps))))  # eps as the ABI's float
        print(f"case {case} eps {eps}: part {res['parts'][k, 0]!r} expected {want!r}")
        assert res["parts"][k, 0] == want
        assert (nbits(res["dy"][k]) == 0).all()
    if k:
        assert np.array_equal(nbits(res["parts"][:k]), nbits(run(*white(case), P, case[4], eps=1e-6)["parts"][:k]))


# ---------------------------------------------------------------------- 7. NaN
@pytest.mark.parametrize("case", CASES[1:], ids=IDS[1:])
def test_a_coast_skips_its_jobs(case):
    p, t = coast(case)
    P, Q = case[3], case[4]
    o64, e_parts, e_grad = coast_oracle(case)
    used = slo.used_jobs(p, t, P, Q)
    print(f"case {case}: used jobs per plane {used.sum(axis=2).ravel()} of {NWIN[case]}")
    assert used.any() and not used.all()
    res = run(p, t, P, Q)
    check_against(res, o64, e_parts, e_grad, P, f"coast {case}")
    # +0.0f wherever no used window reaches
    cover = np.zeros(p.shape, bool)
    for n in range(p.shape[0]):
        for c in range(p.shape[1]):
            for w, (y0, x0) in enumerate(slo.windows(case[1], case[2], P, Q)):
                if used[n, c, w]:
                    cover[n, c, y0:y0 + P, x0:x0 + P] = True
    assert (~cover).any() and (nbits(res["dy"])[~cover] == 0).all() and not cover[~np.isfinite(t)].any()
    assert np.isfinite(res["dy"]).all()
    # uncovered pixels are not written at all
    dy0 = np.full(p.shape, -0.0, np.float32)
    assert (nbits(run(p, t, P, Q, dy0=dy0)["dy"])[~cover] == nbits(np.float32(-0.0))).all()
    # another NaN, and a non-finite prediction instead: the same bits
    t2 = nbits(t).copy()
    t2[np.isnan(t)] = -4194304 + 0x12345  # 0xffc12345: the sign bit and a payload
    t2 = t2.view(np.float32)
    assert np.isnan(t2).sum() == np.isnan(t).sum() and not np.array_equal(nbits(t2), nbits(t))
    res2 = run(p, t2, P, Q)
    for key in ("parts", "cparts", "spec4", "total", "dy"):
        assert np.array_equal(nbits(res2[key]), nbits(res[key])), key


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_job_skipped_is_zero_not_nan(case):
    p, t = (v.copy() for v in white(case))
    t[:, :, ::8, ::8] = np.nan
    rng = np.random.default_rng(9)
    dy0 = rng.standard_normal(shape_of(case)).astype(np.float32)
    res = run(p, t, case[3], case[4], dy0=dy0)
    assert (res["cparts"] == 0).all() and (nbits(res["parts"]) == 0).all()
    assert (nbits(res["spec4"]) == 0).all()
    assert nbits(res["total"])[0] == nbits(np.float32(LOSS4[3]))[0]
    assert np.array_equal(nbits(res["dy"]), nbits(dy0))


# ------------------------------------------------------------- 8. determinism
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bit_identical_runs_and_plane_ranges(case):
    for fields in (white, coast):
        p, t = fields(case)
        a, b = run(p, t, case[3], case[4]), run(p, t, case[3], case[4])
        for key in ("parts", "cparts", "spec4", "total", "dy"):
            assert np.array_equal(nbits(a[key]), nbits(b[key])), key
        N = p.shape[0]
        if N > 1:  # the batch in two calls over tile ranges, the later range first
            c = run(p, t, case[3], case[4], splits=[(1, N), (0, 1)])
            for key in ("parts", "cparts", "spec4", "total", "dy"):
                assert np.array_equal(nbits(a[key]), nbits(c[key])), key


# ------------------------------------------------------------------- capture
def test_the_three_launches_are_capturable_and_replay_on_new_inputs():
    d = dev()
    case = CASES[3]
    p, t = (torch.tensor(v, device=d) for v in coast(case))
    p2 = (p + 0.1).contiguous()
    sl = SpectralLoss(p.shape, case[3], case[4], device=d)
    pa, dy, l4 = p.clone(), torch.zeros_like(p), torch.tensor(LOSS4, device=d)

    def stage():
        sl.parts(pa, t)
        sl.finalize(l4[3:4])
        sl.add_dy(dy)
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
    sl.spec4.fill_(-7.0)
    g.replay()
    torch.cuda.synchronize()
    eager = run(p2.cpu().numpy(), t.cpu().numpy(), case[3], case[4])
    assert np.array_equal(nbits(sl.spec4.cpu().numpy()), nbits(eager["spec4"])) and eager["spec4"][1] == 4
    assert np.array_equal(nbits(dy.cpu().numpy()), nbits(eager["dy"]))
    assert np.array_equal(nbits(sl.total.cpu().numpy()), nbits(eager["total"]))
    assert not np.array_equal(eager["spec4"], run(*coast(case), case[3], case[4])["spec4"])  # the inputs do differ


# ----------------------------------------------------------- 9. refused arguments
def test_refused_arguments_launch_nothing():
    lib = _lib.load()
    d = dev()
    E = _lib.SRMI_ERR_ARG
    H = W = 64
    import ctypes as C
    n = C.c_size_t(0)
    wsz = lib.srmi_spectral_loss_workspace
    assert wsz(2, H, W, 32, 16, C.byref(n)) == 0 and n.value > 2 * 9 * 32 * 32 * 4
    nbytes = n.value
    for bad in ((2, H, W, 48, 16), (2, H, W, 8, 4), (2, H, W, 128, 64), (2, 48, W, 64, 32), (2, H, 48, 64, 32),
                (2, H, W, 32, 0), (2, H, W, 32, 33), (0, H, W, 32, 16)):
        assert wsz(*bad, C.byref(n)) == E, bad
    assert wsz(2, H, W, 32, 16, None) == E
    p = torch.randn(2, 1, H, W, device=d)
    t = torch.randn(2, 1, H, W, device=d)
    ws = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=d)
    parts, cparts = torch.full((2,), -7.0, device=d), torch.full((2,), -7.0, device=d)
    l4 = torch.tensor(LOSS4, device=d)
    s4, tot = torch.full((4,), -7.0, device=d), torch.full((1,), -7.0, device=d)
    dy = torch.full((2, 1, H, W), -7.0, device=d)
    st = stream_handle()
    f = lib.srmi_spectral_loss_parts
    ok = dict(pred=ptr(p), target=ptr(t), nplanes=2, H=H, W=W, P=32, Q=16, eps=1e-12, parts=ptr(parts),
              cparts=ptr(cparts), ws=ptr(ws), nbytes=nbytes)
    for change in (dict(P=48), dict(P=128), dict(P=8), dict(H=16), dict(W=16), dict(Q=0), dict(Q=33),
                   dict(nplanes=0), dict(eps=0.0), dict(eps=-1.0), dict(eps=float("nan")), dict(pred=None),
                   dict(target=None), dict(parts=None), dict(cparts=None), dict(ws=None), dict(nbytes=nbytes - 1)):
        a = dict(ok, **change)
        assert f(a["pred"], a["target"], a["nplanes"], a["H"], a["W"], a["P"], a["Q"], a["eps"], a["parts"],
                 a["cparts"], a["ws"], a["nbytes"], st) == E, change
    f = lib.srmi_spectral_loss_from_parts
    ok = dict(parts=ptr(parts), cparts=ptr(cparts), nplanes=2, P=32, weight=1.0, loss4=ptr(l4[3:4]), spec4=ptr(s4),
              total=ptr(tot))
    for change in (dict(P=48), dict(nplanes=0), dict(weight=-1.0), dict(weight=float("inf")), dict(parts=None),
                   dict(cparts=None), dict(loss4=None), dict(spec4=None), dict(total=None)):
        a = dict(ok, **change)
        assert f(a["parts"], a["cparts"], a["nplanes"], a["P"], a["weight"], a["loss4"], a["spec4"], a["total"],
                 st) == E, change
    f = lib.srmi_spectral_loss_dy
    ok = dict(ws=ptr(ws), nbytes=nbytes, nplanes=2, H=H, W=W, P=32, Q=16, weight=1.0, spec4=ptr(s4), dy=ptr(dy))
    for change in (dict(P=48), dict(H=16), dict(Q=0), dict(Q=33), dict(nplanes=0), dict(weight=-1.0),
                   dict(weight=float("nan")), dict(ws=None), dict(spec4=None), dict(dy=None), dict(nbytes=nbytes - 1)):
        a = dict(ok, **change)
        assert f(a["ws"], a["nbytes"], a["nplanes"], a["H"], a["W"], a["P"], a["Q"], a["weight"], a["spec4"],
                 a["dy"], st) == E, change
    torch.cuda.synchronize()
    # nothing was launched: every output still holds what it was filled with
    assert (parts == -7.0).all() and (cparts == -7.0).all() and (s4 == -7.0).all() and (tot == -7.0).all()
    assert (dy == -7.0).all() and (ws == 0x5A).all()
    # the Python layer says which value it refuses
    for kw, what in ((dict(window=48), "window 48"), (dict(stride=0), "stride 0"), (dict(stride=65), "stride 65"),
                     (dict(eps=0.0), "eps 0.0"), (dict(weight=-1.0), "weight -1.0")):
        with pytest.raises(ValueError, match=what):
            SpectralLoss((2, 1, H, W), device=d, **kw)
    with pytest.raises(ValueError, match="does not fit"):
        SpectralLoss((2, 1, 48, 48), device=d)


# ===================================================================== the trainer
def rcan_spec(nl, nb, scale=4, dtype="bf16"):
    return NetSpec(arch="rcan", nchannels_in=2, nchannels_out=2, nfeatures=64, nlayers=nl, nblocks=nb, cbottleneck=2,
                   scale=scale, dtype=dtype)


def init_flat(spec, seed):
    table = param_table(spec)
    flat = torch.empty(sum(t[2] for t in table), device=dev())
    default_init_(flat, table, seed=seed)
    return flat


SPECTRAL = dict(weight=1.0, window=64, stride=32)


# ------------------------------------------------- T1. weight 0 is the plain trainer
@pytest.mark.parametrize("loss_fn", ["l2", "charbonnier"])
@pytest.mark.parametrize("B,micro", [(2, 1), (4, 2)])
def test_weight_zero_trainer_is_the_plain_trainer(B, micro, loss_fn):
    """The parts and the finalise run, add_dy launches nothing, total = loss4[3] + 0 * L_spec,
    and the backward takes the pixel loss's dy as it is instead of forming it in the tail
    kernels: every bit of two steps is the plain trainer's."""
    spec = rcan_spec(1, 2)
    flat = init_flat(spec, 5)
    hr = torch.tensor(ro.synthetic_hr(B, 2, 192, 19), device=dev())
    res = []
    for spectral in (None, dict(SPECTRAL, weight=0.0)):
        tr = FusedTrainer(spec, B, (48, 48), device=dev(), params=flat, micro=micro, loss_fn=loss_fn, spectral=spectral)
        assert tr.micro == micro
        rows = []
        for _ in range(2):
            out = tr.step(hr)
            torch.cuda.synchronize()
            assert set(out) == ({"loss", "interp_loss"} if spectral is None else
                                {"loss", "interp_loss", "pixel_loss", "spectral_loss"})
            rows.append((out["loss"].clone(), out["interp_loss"].clone(), tr.sr.clone(), tr.grads.clone(),
                         tr.params.clone()))
        if spectral is not None:
            assert torch.equal(bits(out["pixel_loss"]), bits(out["loss"])) and float(out["spectral_loss"]) > 0
        res.append(rows)
        del tr
    for k, (a, b) in enumerate(zip(*res)):
        for x, y, what in zip(a, b, ("loss", "interp_loss", "sr", "grads", "params")):
            assert torch.equal(bits(x), bits(y)), (k, what, float((x - y).abs().max()))
    assert np.isfinite(float(res[0][1][0]))


# --------------------------------------------------------- T2. / T4. against fp64
def spectral_drift_bounds(monkeypatch, model, hr, scale, loss_fn, g_ref):
    """test_gpu_model.drift_bounds itself (3 x the drift of the same fp64 step with
    bf16-rounded conv operands, + 1e-3) with the oracle step it runs the emulation through
    replaced by the one with the term, as test_gpu_land_train.masked_drift_bounds does."""
    monkeypatch.setattr(test_gpu_model, "oracle_grads",
                        lambda m, h, s: slo.train_step(m, h, s, loss_fn, SPECTRAL)[:3])
    return test_gpu_model.drift_bounds(model, hr, scale, g_ref)


def step_vs_oracle(monkeypatch, hr, loss_fn, land):
    d = dev()
    model = ro.RCANOracle(nchannels_in=2, nchannels_out=2, nlayers=2, nblocks=2, nfeatures=64, cbottleneck=2)
    ro.init_params_numpy(model, 22)
    spec = rcan_spec(2, 2)
    table = param_table(spec)
    flat = flat_from_model(model, table).to(d)
    model = model.double()
    l_ref, _, g_ref, parts = slo.train_step(model, hr, 4, loss_fn, SPECTRAL)
    bound = spectral_drift_bounds(monkeypatch, model, hr, 4, loss_fn, g_ref)
    tr = FusedTrainer(spec, 3, (48, 48), device=d, params=flat, loss_fn=loss_fn, land=land, spectral=SPECTRAL)
    hr_d = torch.tensor(hr, device=d)
    out = tr.step(hr_d)
    torch.cuda.synchronize()
    for key, ref in (("loss", l_ref), ("pixel_loss", parts["pixel_loss"]), ("spectral_loss", parts["spectral_loss"])):
        got = float(out[key])
        print(f"{loss_fn} land={land}: {key} {got:.6f} oracle {ref:.6f} rel {abs(got - ref) / ref:.2e} (bar 2e-3)")
        assert abs(got - ref) / ref < 2e-3, key
    assert float(tr.spectral.spec4[1]) == parts["nused"] == slo.used_jobs(np.zeros_like(hr), hr, 64, 32).sum()
    assert parts["spectral_loss"] > 0.1 * parts["pixel_loss"]  # the term is a real share of the loss
    g = tr.grads.cpu()
    for name, off, n, shape in table:
        r = rel_l2(g[off:off + n].view(shape), g_ref[name])
        assert r <= bound[name], (name, r, bound[name])
    dy = tr.dy.cpu().numpy().copy()
    out = tr.step(hr_d)
    torch.cuda.synchronize()
    assert torch.isfinite(tr.params).all() and np.isfinite(float(out["loss"]))
    return tr, dy, parts


@pytest.mark.parametrize("loss_fn", ["l2", "charbonnier"])
def test_spectral_trainer_step_vs_oracle(loss_fn, monkeypatch):
    """test_land_trainer_step_vs_masked_oracle's bars: the losses 2e-3 relative, every
    gradient tensor within test_gpu_model.drift_bounds."""
    tr, _, parts = step_vs_oracle(monkeypatch, ro.synthetic_hr(3, 2, 192, 21), loss_fn, False)
    assert parts["nused"] == 3 * 2 * 25


@pytest.mark.parametrize("loss_fn", ["l2", "charbonnier"])
def test_spectral_land_trainer_step_vs_oracle(loss_fn, monkeypatch):
    hr = lt.land_batch(3, 2, 192, 21)
    lt.check_conditions(hr, 4)
    tr, dy, parts = step_vs_oracle(monkeypatch, hr, loss_fn, True)
    assert 2 * 25 < parts["nused"] < 3 * 2 * 25
    assert (dy[~np.isfinite(hr)].view(np.int32) == 0).all()  # +0.0f on land


# ------------------------------------------------------------- T3. the fp32 engine
def test_spectral_trainer_fp32_step_vs_oracle():
    """test_land_trainer_fp32_step_vs_masked_oracle's bars: the loss and the output 1e-5
    relative, every gradient tensor 1e-3 rel-L2."""
    d = dev()
    model = ro.RCANOracle(nchannels_in=2, nchannels_out=2, nlayers=2, nblocks=2, nfeatures=64, cbottleneck=2)
    ro.init_params_numpy(model, 23)
    spec = rcan_spec(2, 2, dtype="fp32")
    table = param_table(spec)
    hr = ro.synthetic_hr(3, 2, 192, 21)
    tr = FusedTrainer(spec, 3, (48, 48), device=d, params=flat_from_model(model, table).to(d), spectral=SPECTRAL)
    l_ref, out_ref, g_ref, parts = slo.train_step(model.double(), hr, 4, "l2", SPECTRAL)
    out = tr.step(torch.tensor(hr, device=d))
    torch.cuda.synchronize()
    for key, ref in (("loss", l_ref), ("pixel_loss", parts["pixel_loss"]), ("spectral_loss", parts["spectral_loss"])):
        print(f"fp32: {key} {float(out[key]):.8f} oracle {ref:.8f} rel {abs(float(out[key]) - ref) / ref:.2e}")
        assert abs(float(out[key]) - ref) / ref < 1e-5, key
    assert rel_l2(tr.sr, out_ref) < 1e-5
    g = tr.grads.cpu()
    worst = max(rel_l2(g[off:off + n].view(shape), g_ref[name]) for name, off, n, shape in table)
    print(f"fp32 engine with the spectral term: worst per-tensor grad rel-L2 {worst:.2e} (bar 1e-3)")
    assert worst < 1e-3


# -------------------------------------------------------- T5. micro-batch split
def test_spectral_micro_batch_split():
    """test_land_micro_batch_split's bars: the losses bit-identical (parts and counts in
    plane order), the gradients to 1e-5 rel-L2."""
    spec = rcan_spec(1, 2)
    flat = init_flat(spec, 5)
    hr = torch.tensor(lt.land_batch(4, 2, 192, 24), device=dev())
    res = []
    for micro in (1, 2):
        tr = FusedTrainer(spec, 4, (48, 48), device=dev(), params=flat, micro=micro, land=True, spectral=SPECTRAL)
        out = tr.step(hr)
        torch.cuda.synchronize()
        res.append(([float(out[k]) for k in ("loss", "pixel_loss", "spectral_loss")], tr.grads.clone()))
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
    tr = FusedTrainer(spec, b - a, (48, 48), device=d, params=flat, micro=2, info=info, land=True, spectral=SPECTRAL)
    out = tr.step(hr_all[a:b].contiguous())
    torch.cuda.synchronize()
    q.put((rank, [float(out[k]) for k in ("loss", "pixel_loss", "spectral_loss")], tr.grads.cpu().numpy(),
           tr.params.cpu().numpy()))
    dist.destroy_process_group()


def test_spectral_dp_world2_matches_single_process():
    """test_land_dp_world2_matches_single_process's conventions and bars (gloo, both ranks
    on cuda:0; gradients 2e-4 rel-L2): rank 0 holds the all-wet tile, so the ranks'
    used-job counts differ; parts and counts go through one all-reduce."""
    import multiprocessing as mp
    hr_np = lt.land_batch(4, 2, 192, 25)
    used = slo.used_jobs(np.zeros_like(hr_np), hr_np, 64, 32).sum(axis=(1, 2))
    assert used[0] == 50 and used[:2].sum() != used[2:].sum() and used[2:].sum() > 0
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
    tr = FusedTrainer(spec, 4, (48, 48), device=d, params=init_flat(spec, 5), micro=1, land=True, spectral=SPECTRAL)
    out = tr.step(torch.tensor(hr_np, device=d))
    torch.cuda.synchronize()
    losses, g = [float(out[k]) for k in ("loss", "pixel_loss", "spectral_loss")], tr.grads.cpu().numpy()
    assert float(tr.spectral.spec4[1]) == used.sum()
    for rank, l_r, g_r, p_r in res:
        assert l_r == losses, (rank, l_r, losses)
        assert np.linalg.norm(g_r - g) / np.linalg.norm(g) < 2e-4
    np.testing.assert_array_equal(res[0][3], res[1][3])  # replicas stay identical after Adam


# ------------------------------------------------------------------ T7. construction
@pytest.mark.parametrize("spectral,what", [
    (dict(window=48), "window 48"), (dict(window=128), "window 128"), (dict(stride=0), "stride 0"),
    (dict(window=32, stride=33), "stride 33"), (dict(weight=-0.5), "weight -0.5"),
    (dict(weight=float("nan")), "weight nan"), (dict(weight=float("inf")), "weight inf"), (dict(eps=0.0), "eps 0.0"),
    (dict(eps=-1e-12), "eps -1e-12"), (dict(windw=64), "windw")])
def test_trainer_refuses_a_bad_spectral_config(spectral, what):
    with pytest.raises(ValueError, match=what):
        FusedTrainer(rcan_spec(1, 1), 2, (48, 48), device=dev(), spectral=spectral)
    with pytest.raises(ValueError, match="larger than the HR tile"):
        FusedTrainer(rcan_spec(1, 1, scale=2), 2, (16, 16), device=dev(), spectral=dict(window=64))
