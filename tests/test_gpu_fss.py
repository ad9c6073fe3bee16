"""The fractions skill score on the HIP path: srmi_fss / srmi.fss.FractionsSkillScore and
RegionSuperResolver.score_fss against the oracle (tests/fss_oracle.py).

Bars.  Every sum is an integer, so the tables ('num', 'den', 'events_pred', 'events_truth',
'used') are held to the oracle EXACTLY (array_equal, int64).  The derived values are a handful
of fp64 roundings of exact integers on both sides (two int64 -> fp64 conversions, a quotient
and a difference, or the few products of afss): 1e-12 relative, test_gpu_distribution.py's bar
and its argument; the NaN positions must be equal.  Every test prints the number of differing
entries and the worst derived error before it asserts.

The shapes are the smallest at which the kernels can go wrong: one pixel; a ragged plane whose
second plane is off 16-byte alignment, whose W is no multiple of 64 (a partial ballot word) and
which the largest window covers from every position (fss == afss; that needs n >= 2 max(H, W) -
1 = 105, so the ladder ends 79, 105); one pixel more than the windows launch's 512 x 64 tile
both ways; many workgroups; a ladder that crosses every change in the number of words a window
reaches (h = 0, 1 .. 64, 65 .. 127); and the 256 x 256 case whose sums pass 2^32."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fss_oracle as fo  # noqa: E402
from srmi import _lib  # noqa: E402
from srmi._lib import ptr, stream_handle  # noqa: E402
from srmi.distribution import DistributionScore, contingency  # noqa: E402
from srmi.fss import FSS_DERIVED, FSS_TILE, FractionsSkillScore, fss_workspace  # noqa: E402
from test_gpu_distribution import field  # noqa: E402
from test_gpu_ssim_loss import dev, sid  # noqa: E402

TILE_H, TILE_W = FSS_TILE  # checked against the library by test_fss_oracle.py
TABLES = ("num", "den", "events_pred", "events_truth", "used")
DERIVED = ("fss",) + FSS_DERIVED
LADDER = (1, 3, 5, 9, 17, 33, 79, 105)
LADDER16 = (1, 3, 5, 7, 9, 17, 33, 63, 65, 67, 127, 129, 131, 191, 253, 255)
Q = (0.5, 0.9, 0.99)


def quantiles(truth, probs):
    """[C, T] fp32: a different threshold row per channel, from the channel's own values."""
    return np.stack([np.quantile(truth[c][np.isfinite(truth[c])], probs) for c in range(truth.shape[0])]).astype(np.float32)


def coast(pred, truth):
    """A coast in both fields, some +-Inf, and pixels masked in one field only."""
    p, t = pred.copy(), truth.copy()
    _, H, W = p.shape
    p[:, H // 3:H // 2, W // 4:W // 2] = np.nan
    t[:, H // 3:H // 2, W // 4:W // 2] = np.nan
    t[0, 0, 0] = np.inf
    p[-1, H - 1, W - 1] = -np.inf
    p[0, H // 5, ::7] = np.inf
    t[-1, ::5, W // 7] = np.nan
    return p, t


# name -> (shape, kind, probs of the thresholds, scales)
CASES = {
    "one pixel": ((1, 1, 1), "white", (0.5,), (1, 3)),
    "ragged white": ((2, 37, 53), "white", Q, LADDER),
    "ragged smooth": ((2, 37, 53), "smooth", Q, LADDER),
    "tile + 1": ((1, TILE_H + 1, TILE_W + 1), "white", (0.9,), (1, 3, 65, 255)),
    "tile": ((1, TILE_H, TILE_W), "smooth", (0.9,), (5, 129)),
    "many workgroups white": ((2, 300, 517), "white", (0.5, 0.99), (1, 5, 33, 129)),
    "many workgroups smooth": ((2, 300, 517), "smooth", (0.5, 0.99), (1, 5, 33, 129)),
    "T1 N1": ((2, 70, 150), "white", (0.9,), (7,)),
    "T8 N16": ((2, 70, 150), "white", (0.01, 0.1, 0.3, 0.5, 0.7, 0.9, 0.99, 0.999), LADDER16),
    "T8 N16 smooth": ((2, 70, 150), "smooth", (0.01, 0.1, 0.3, 0.5, 0.7, 0.9, 0.99, 0.999), LADDER16),
    "coast": ((2, 61, 130), "coast", Q, (1, 3, 9, 33, 131)),
}


@functools.lru_cache(maxsize=None)
def case(name):
    shape, kind, probs, scales = CASES[name]
    p, t = field("white" if kind == "coast" else kind, shape)
    if kind == "coast":
        p, t = coast(p, t)
    thr = quantiles(t, probs)
    for a in (p, t, thr):
        a.setflags(write=False)
    return p, t, thr, scales, fo.fss(p, t, thr, scales)


def measure(p, t, thr, scales, fill=0xFF):
    d = dev()
    fs = FractionsSkillScore(p.shape, thr, scales, device=d)
    fs.workspace.fill_(fill)
    res = fs.measure(torch.tensor(p, device=d), torch.tensor(t, device=d))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in res.items()}


def check_against(tag, m, o):
    """The bars of the module docstring; prints before it asserts."""
    wrong = {k: int((m[k] != o[k]).sum()) for k in TABLES}
    worst = 0.0
    nan_ok = True
    for k in DERIVED:
        got, want = m[k], o[k]
        nan_ok = nan_ok and np.array_equal(np.isnan(got), np.isnan(want))
        ok = np.isfinite(want) & np.isfinite(got)
        nan_ok = nan_ok and np.array_equal(got[~ok & ~np.isnan(want)], want[~ok & ~np.isnan(want)])  # +-Inf
        if ok.any():
            worst = max(worst, float((np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1e-300)).max()))
    print(f"{tag}: differing table entries {wrong}, worst derived rel error {worst:.2e}, NaN / Inf positions equal: {nan_ok}")
    for k in TABLES:
        assert m[k].dtype == np.int64 and m[k].shape == o[k].shape and np.array_equal(m[k], o[k]), k
    for k in DERIVED:
        assert m[k].dtype == np.float64 and m[k].shape == o[k].shape, k
    assert nan_ok and worst <= 1e-12


# ------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("name", list(CASES))
def test_matches_the_oracle(name):
    p, t, thr, scales, o = case(name)
    m = measure(p, t, thr, scales)
    check_against(name, m, o)
    if name.startswith("ragged"):  # the second plane starts off 16-byte alignment, and the window covers the plane
        assert (p[0].size * 4) % 16 != 0
        ok = np.isfinite(m["afss"])
        assert ok.any() and np.abs(m["fss"][..., -1][ok] - m["afss"][ok]).max() <= 1e-12
        assert np.array_equal(m["num"][..., -1], 37 * 53 * (m["events_pred"] - m["events_truth"]) ** 2)
    if name == "coast":
        assert (m["used"] < 61 * 130).all() and (m["events_truth"] > 0).all()


def test_sums_beyond_32_bits():
    """pred all 1, truth all 0, threshold 0.5, n = 255 on 256 x 256: Sp is the clipped window's
    area, St 0, so num = den = (sum_y min(y + 127, 255) - max(y - 127, 0) + 1)^2 summed as
    squares = 94 820 853 760 000; a 32-bit accumulator anywhere fails it."""
    p, t = np.ones((1, 256, 256), np.float32), np.zeros((1, 256, 256), np.float32)
    m = measure(p, t, [0.5], (255,))
    ext = np.minimum(np.arange(256) + 127, 255) - np.maximum(np.arange(256) - 127, 0) + 1
    want = int((ext.astype(np.int64) ** 2).sum()) ** 2
    print(f"n = 255 on 256^2: num {int(m['num'][0, 0, 0])}, den {int(m['den'][0, 0, 0])}, expected {want}")
    assert want == 94820853760000
    assert m["num"][0, 0, 0] == want and m["den"][0, 0, 0] == want
    assert m["fss"][0, 0, 0] == 0 and m["events_pred"][0, 0] == 65536 and m["events_truth"][0, 0] == 0
    assert np.isnan(m["skilful_scale"][0, 0]) and m["afss"][0, 0] == 0 and np.isinf(m["bias"][0, 0])


def test_equal_fields_a_nan_threshold_and_an_empty_channel():
    p, t, _, _, _ = case("ragged white")
    t2 = t.copy()
    t2[1] = np.nan  # channel 1 has no used pixel
    thr = np.array([[289.0, np.nan, 1e9], [290.0, 291.0, np.nan]], dtype=np.float32)
    m = measure(t2.copy(), t2, thr, LADDER)
    check_against("equal fields", m, fo.fss(t2, t2, thr, LADDER))
    assert (m["fss"][0, 0] == 1).all() and m["skilful_scale"][0, 0] == 1
    assert np.isnan(m["fss"][0, 1:]).all() and (m["den"][0, 1:] == 0).all()  # a NaN threshold, and one above everything
    assert m["used"][1] == 0 and (m["num"][1] == 0).all() and (m["den"][1] == 0).all()
    for k in DERIVED:
        assert np.isnan(m[k][1]).all(), k
    m = measure(p, t2, thr, LADDER)
    check_against("empty channel", m, fo.fss(p, t2, thr, LADDER))


# ------------------------------------------------- 2. determinism, device thresholds, capture
def test_bit_identical_runs_whatever_the_workspace_held():
    for name in ("coast", "tile + 1"):
        p, t, thr, scales, _ = case(name)
        a = measure(p, t, thr, scales)
        for other in (measure(p, t, thr, scales), measure(p, t, thr, scales, fill=0x00), measure(p, t, thr, scales, fill=0x5A)):
            for k in TABLES + DERIVED:
                assert np.array_equal(other[k].view(np.int64), a[k].view(np.int64)), (name, k)


def test_thresholds_refilled_on_the_device_between_two_measures():
    d = dev()
    p, t, thr, scales, o = case("ragged white")
    thr_d = torch.tensor(thr, device=d)
    fs = FractionsSkillScore(p.shape, thr_d, scales, device=d)
    assert fs.thresholds is thr_d
    pd, td = torch.tensor(p, device=d), torch.tensor(t, device=d)
    m = {k: v.cpu().numpy().copy() for k, v in fs.measure(pd, td).items()}
    check_against("device thresholds", m, o)
    thr2 = (thr + np.float32(0.75)).astype(np.float32)
    thr_d.copy_(torch.tensor(thr, device=d) + 0.75)  # on the device: no host read in between
    m2 = {k: v.cpu().numpy().copy() for k, v in fs.measure(pd, td).items()}
    check_against("device thresholds refilled", m2, fo.fss(p, t, thr2, scales))
    assert not np.array_equal(m["num"], m2["num"])


def raw_call(p, t, thr_np, ladder, canary=8, **change):
    """srmi_fss on buffers that carry `canary` words after each output and after the workspace
    -> (rc, the buffers, the workspace, its bytes)."""
    d = dev()
    lib = _lib.load()
    Cn, H, W = p.shape
    T, N = thr_np.shape[1], len(ladder)
    nbytes = fss_workspace(Cn, H, W, T, N)
    ws = torch.full((nbytes + 8 * canary,), 0x5A, dtype=torch.uint8, device=d)
    sizes = {"num": Cn * T * N, "den": Cn * T * N, "events": Cn * T * 2, "used": Cn, "derived": Cn * T * (N + 6)}
    bufs = {k: torch.full((sizes[k] + canary,), -7, dtype=torch.float64 if k == "derived" else torch.int64, device=d)
            for k in sizes}
    keep = [torch.tensor(p, device=d), torch.tensor(t, device=d), torch.tensor(thr_np, device=d)]
    a = dict(pred=ptr(keep[0]), truth=ptr(keep[1]), C=Cn, H=H, W=W, thr=ptr(keep[2]), T=T,
             scales=(C.c_int * 16)(*ladder), N=N, ws=ptr(ws), nbytes=nbytes, num=ptr(bufs["num"]), den=ptr(bufs["den"]),
             events=ptr(bufs["events"]), used=ptr(bufs["used"]), derived=ptr(bufs["derived"]))
    a.update(change)
    rc = lib.srmi_fss(a["pred"], a["truth"], a["C"], a["H"], a["W"], a["thr"], a["T"], a["scales"], a["N"], a["ws"],
                      a["nbytes"], a["num"], a["den"], a["events"], a["used"], a["derived"], a.get("launches", 0),
                      stream_handle())
    torch.cuda.synchronize()
    return rc, bufs, ws, nbytes, sizes


def test_canaries_behind_every_output_and_the_workspace():
    for name in ("ragged white", "tile + 1", "T8 N16"):
        p, t, thr, scales, o = case(name)
        rc, bufs, ws, nbytes, sizes = raw_call(p, t, thr, scales)
        assert rc == 0
        for k, b in bufs.items():
            assert (b[sizes[k]:] == -7).all(), (name, k)
        assert (ws[nbytes:] == 0x5A).all(), name
        Cn, T, N = p.shape[0], thr.shape[1], len(scales)
        assert np.array_equal(bufs["num"][:sizes["num"]].cpu().numpy().reshape(Cn, T, N), o["num"])
        assert np.array_equal(bufs["events"][:sizes["events"]].cpu().numpy().reshape(Cn, T, 2)[..., 1], o["events_truth"])


def test_the_launches_are_capturable_and_replay_on_new_inputs():
    d = dev()
    p, t, thr, scales, o = case("coast")
    pd, td = torch.tensor(p, device=d), torch.tensor(t, device=d)
    fs = FractionsSkillScore(p.shape, thr, scales, device=d)
    pa = pd.clone()
    fs.measure(pa, td)  # warm-up outside capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(device=d)
    s.wait_stream(torch.cuda.current_stream(d))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            res = fs.measure(pa, td)
    torch.cuda.current_stream(d).wait_stream(s)
    p2 = np.roll(p, 3, axis=-1)
    pa.copy_(torch.tensor(p2, device=d))
    fs.derived.fill_(-7.0)
    fs.num.fill_(-7)
    g.replay()
    torch.cuda.synchronize()
    m = {k: v.cpu().numpy().copy() for k, v in res.items()}
    o2 = fo.fss(p2, t, thr, scales)
    check_against("replay on new inputs", m, o2)
    assert not np.array_equal(o2["num"], o["num"])  # the inputs do differ


# ----------------------------------------------------------- 3. refused arguments
def test_refused_arguments_launch_nothing():
    E = _lib.SRMI_ERR_ARG
    p, t, thr, scales, _ = case("ragged white")
    nbytes = fss_workspace(2, 37, 53, 3, len(scales))

    def sc(*v):
        return (C.c_int * 16)(*v)
    changes = [dict(pred=None), dict(truth=None), dict(thr=None), dict(scales=None), dict(ws=None), dict(num=None),
               dict(den=None), dict(events=None), dict(used=None), dict(derived=None), dict(T=0), dict(T=9), dict(N=0),
               dict(N=17), dict(C=0), dict(H=0), dict(W=0), dict(H=-1), dict(H=1 << 16, W=1 << 15),
               dict(nbytes=nbytes - 1), dict(launches=8), dict(launches=-1), dict(scales=sc(1, 3, 5, 9, 17, 33, 79, 104)),
               dict(scales=sc(1, 3, 5, 9, 17, 33, 79, 257)), dict(scales=sc(0, 3, 5, 9, 17, 33, 79, 105)),
               dict(scales=sc(1, 3, 3, 9, 17, 33, 79, 105)), dict(scales=sc(1, 5, 3, 9, 17, 33, 79, 105)),
               dict(scales=sc(-1, 3, 5, 9, 17, 33, 79, 105)), dict(H=46340, W=46340, scales=sc(255), N=1)]
    for change in changes:
        rc, bufs, ws, _, _ = raw_call(p, t, thr, scales, **change)
        assert rc == E, change
        for k, b in bufs.items():
            assert (b == -7).all(), (change, k)
        assert (ws == 0x5A).all(), change
    rc, bufs, ws, nb, _ = raw_call(p, t, thr, scales)
    rc2, _, _, _, _ = raw_call(p, t, thr, scales, ws=ptr(ws) + 8, nbytes=nb)  # a misaligned workspace
    assert rc == 0 and rc2 == E
    # the Python layer refuses before anything is allocated
    d = dev()
    for kw in (dict(scales=(1, 2)), dict(scales=(3, 1)), dict(scales=()), dict(scales=(257,))):
        with pytest.raises(ValueError, match="scales"):
            FractionsSkillScore((2, 37, 53), [0.0], device=d, **kw)
    with pytest.raises(ValueError, match="thresholds"):
        FractionsSkillScore((2, 37, 53), [0.0] * 9, device=d)
    with pytest.raises(ValueError, match="thresholds"):
        FractionsSkillScore((2, 37, 53), torch.zeros((3, 2), device=d), device=d)
    with pytest.raises(ValueError, match="thresholds"):
        FractionsSkillScore((2, 37, 53), torch.zeros((2, 2), dtype=torch.float64, device=d), device=d)
    fs = FractionsSkillScore((2, 37, 53), [0.0], device=d)
    with pytest.raises(ValueError, match="pred"):
        fs.measure(torch.zeros((2, 37, 52), device=d), torch.zeros((2, 37, 53), device=d))


# --------------------------------------------- 4. n = 1 is the distribution score's table
def test_n1_equals_the_contingency_of_a_joint_table_with_an_edge_at_the_threshold():
    """Values on multiples of 1 / 8 inside (-4, 4), a joint table of 8 bins on [-4, 4]: the bin of
    a value is computed without rounding and bin 4 starts at the threshold 0."""
    d = dev()
    rng = np.random.default_rng(77)
    shape = (2, 45, 83)
    t = (rng.integers(-30, 31, shape) / 8.0).astype(np.float32)
    p = (t + rng.integers(-6, 7, shape) / 8.0).clip(-3.75, 3.75).astype(np.float32)
    p[0, 3, 3] = np.nan
    t[1, 7, 9] = np.nan
    pd, td = torch.tensor(p, device=d), torch.tensor(t, device=d)
    ds = DistributionScore(shape, 16, 8, (), value_range=(-4.0, 4.0), device=d)
    table = contingency(ds.measure(pd, td)["joint"], 4)
    fs = FractionsSkillScore(shape, [0.0], (1,), device=d)
    m = {k: v.cpu().numpy() for k, v in fs.measure(pd, td).items()}
    hits, misses, fa = table["hits"], table["misses"], table["false_alarms"]
    print(f"n = 1: num {m['num'][:, 0, 0]} = misses {misses} + false alarms {fa}; den {m['den'][:, 0, 0]}, hits {hits}")
    assert (hits > 0).all() and (misses > 0).all() and (fa > 0).all()
    assert np.array_equal(m["num"][:, 0, 0], misses + fa)
    assert np.array_equal(m["den"][:, 0, 0], 2 * hits + misses + fa)
    assert np.array_equal(m["events_pred"][:, 0], hits + fa) and np.array_equal(m["events_truth"][:, 0], hits + misses)
    np.testing.assert_allclose(m["bias"][:, 0], table["bias"], rtol=1e-15)


# ------------------------------------------------------- 5. RegionSuperResolver
@functools.lru_cache(maxsize=None)
def region(land):
    from srmi.superres import RegionSuperResolver
    from test_gpu_inference import _small_rcan
    d = dev()
    spec, _, flat = _small_rcan()
    rng = np.random.RandomState(64)
    f0 = rng.randn(1, 160, 224)
    hr = ((f0 + np.roll(f0, 1, 1) + np.roll(f0, 1, 2)) * 2 + 5).astype(np.float32)
    if land:
        hr[0, 40:72, 100:140] = np.nan  # land on whole LR pixels
    hr_d = torch.tensor(hr, device=d)
    rs = RegionSuperResolver(spec, flat.to(d), (1, 40, 56), tile_lr=(16, 32), overlap=(4, 4), land=land, device=d)
    images, losses = rs.score(hr_d)
    torch.cuda.synchronize()
    base = {k: v.clone() for k, v in images.items()}, {k: v.clone() for k, v in losses.items()}
    return rs, hr_d, base


@pytest.mark.parametrize("on", ["value", "gradient"])
@pytest.mark.parametrize("land", [False, True], ids=["sea", "land"])
def test_score_fss_is_score_plus_the_measure_of_its_images(land, on):
    from srmi.gradient import GradientScore
    from test_gpu_ssim_loss import bits
    d = dev()
    rs, hr_d, (images0, losses0) = region(land)
    probs, scales = (0.9, 0.99), (1, 3, 9, 33)
    images, losses, got = rs.score_fss(hr_d, probs=probs, scales=scales, on=on)
    torch.cuda.synchronize()
    assert set(images) == set(images0) and set(losses) == set(losses0) and set(got) == {"model", "interpolated"}
    for k in images0:
        assert torch.equal(bits(images[k]), bits(images0[k])), k
    for k in losses0:
        assert torch.equal(bits(losses[k]), bits(losses0[k])), k
    shape = tuple(hr_d.shape)
    for name in got:
        a, b = images[name], hr_d
        if on == "gradient":
            g = GradientScore(shape, (1.0, 1.0), True, device=d).measure(a, b)
            a, b = g["gmag_pred"], g["gmag_truth"]
        thr = DistributionScore(shape, 1024, 0, probs, device=d).measure(a, b)["q_truth"].float()
        assert torch.equal(got[name]["thresholds"], thr) and thr.dtype == torch.float32
        by_hand = FractionsSkillScore(shape, thr, scales, device=d).measure(a, b)
        torch.cuda.synchronize()
        m = {k: got[name][k].cpu().numpy() for k in TABLES + DERIVED}
        for k in TABLES + DERIVED:
            assert np.array_equal(m[k], by_hand[k].cpu().numpy(), equal_nan=True), (name, k)
        check_against(f"score_fss {name} land={land} on={on}", m,
                      fo.fss(a.cpu().numpy(), b.cpu().numpy(), thr.cpu().numpy(), scales))
        full = shape[1] * shape[2]
        assert (m["used"] < full).all() if (land or on == "gradient") else (m["used"] == full).all()
        print(f"score_fss {name} land={land} on={on}: fss {m['fss'][0]}, skilful {m['skilful_scale'][0]}")
    # the scorers are cached per argument key; explicit thresholds need no quantile
    n = len(rs._fss)
    rs.score_fss(hr_d, probs=probs, scales=scales, on=on)
    assert len(rs._fss) == n
    _, _, fixed = rs.score_fss(hr_d, thresholds=[5.0, 7.0], scales=scales, on=on)
    torch.cuda.synchronize()
    assert len(rs._fss) == n + 1 and fixed["model"]["thresholds"].cpu().numpy().tolist() == [[5.0, 7.0]]
    with pytest.raises(ValueError, match="scales"):
        rs.score_fss(hr_d, scales=(2,))
    with pytest.raises(ValueError, match="on "):
        rs.score_fss(hr_d, on="anomaly")
