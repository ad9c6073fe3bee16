"""The distribution score on the HIP path: srmi_distribution /
srmi.distribution.DistributionScore against the numpy oracle (tests/distribution_oracle.py),
and RegionSuperResolver.score_distribution end to end.

Bars.  The histograms, the joint histogram, the count and the range are held to the oracle
EXACTLY (array_equal): every device operation on them is an integer operation or one of the
three fp32 operations of the definition, which numpy reproduces bit for bit.  The derived
values are fp64 on both sides, each at most about ten roundings of exact integers (1e-15):
they are held to 1e-12 relative, with 1e-12 (hi - lo) absolute for values near 0 -- still
five orders below anything an fp32 intermediate would leave (6e-8).  Every test prints the
number of table entries that differ and the derived values' worst error in units of the bar
before it asserts.  Measured on an MI355X: 0 entries and 0 of the bar on every case.

The shapes are the smallest at which the kernel can go wrong: one pixel; a ragged one whose
second plane leaves a and b off 16-byte alignment; SPAN_H x SPAN_W = 8192 pixels is what one
workgroup covers in one step (kDistSpan of csrc/distribution.hip), and the third shape
exceeds it by one pixel on each axis; the last has many workgroups, so the merge of the
partial tables is exercised.  The smooth field puts rows of 64 and more neighbouring pixels
into one bin: the contended path."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import distribution_oracle as do  # noqa: E402
from srmi import _lib  # noqa: E402
from srmi._lib import ptr  # noqa: E402
from srmi.distribution import (COPY_BY_WAVE, MERGE_RUNS, ONE_COPY, DistributionScore,  # noqa: E402
                               distribution_workspace)
from srmi.superres import RegionSuperResolver  # noqa: E402
from test_gpu_inference import _small_rcan  # noqa: E402

SPAN_H, SPAN_W = 64, 128  # kDistSpan = 8192 pixels of a workgroup per step
SHAPES = [(1, 1, 1), (2, 37, 53), (1, SPAN_H + 1, SPAN_W + 1), (2, 300, 517)]
PARAMS = [(2, 0), (16, 2), (256, 32), (4096, 64), (2, 64), (4096, 0)]  # (B, J): every B and every J of the issue
TILE = (16, 32)  # the smallest 16-row tile the inference engine takes
TABLES = ("hist_pred", "hist_truth", "joint", "count")
DERIVED = ("pss", "w1", "under", "over", "q_pred", "q_truth", "q_bias")


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


@functools.lru_cache(maxsize=None)
def field(kind, shape):
    """white: truth = 290 + 1.5 N(0, 1), pred = truth + 0.3 N(0, 1).  smooth: a few long
    sinusoids, almost constant along a row, the prediction pulled to the mean."""
    Cn, H, W = shape
    if kind == "white":
        rng = np.random.default_rng(200)
        truth = (290.0 + 1.5 * rng.standard_normal(shape)).astype(np.float32)
        pred = (truth + 0.3 * rng.standard_normal(shape)).astype(np.float32)
    else:
        c, y, x = np.meshgrid(np.arange(Cn), np.arange(H), np.arange(W), indexing="ij")
        t = (np.sin(2 * np.pi * (y / (1.7 * H) + x / (1000.0 * W) + 0.1 * c)) + 0.5 * np.sin(
            2 * np.pi * (y / (0.9 * H) - x / (1500.0 * W)) + 1.0) + 0.25 * np.cos(2 * np.pi * y / (0.6 * H) + c))
        truth = (290.0 + 1.5 * t).astype(np.float32)
        pred = (290.0 + 1.2 * t + 0.05 * np.sin(2 * np.pi * y / (0.5 * H))).astype(np.float32)
    truth.setflags(write=False)
    pred.setflags(write=False)
    return pred, truth


@functools.lru_cache(maxsize=None)
def oracle(kind, shape, B, J):
    return do.distribution(*field(kind, shape), bins=B, joint=J)


def measure(pred, truth, **kw):
    """numpy fields -> (the measure dict as numpy arrays, the DistributionScore)."""
    d = dev()
    sc = DistributionScore(pred.shape, device=d, **kw)
    m = sc.measure(torch.tensor(pred, device=d), torch.tensor(truth, device=d))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in m.items()}, sc


def check_against(tag, m, o):
    """The bars of the module docstring; prints before it asserts."""
    wrong = {k: int((m[k] != o[k]).sum()) for k in TABLES}
    span = np.where(np.isfinite(o["hi"]), o["hi"].astype(np.float64) - o["lo"].astype(np.float64), 0.0)
    worst = 0.0
    for k in DERIVED:
        got, want = m[k].astype(np.float64), o[k]
        assert np.array_equal(np.isnan(got), np.isnan(want)), (tag, k)
        bar = 1e-12 * np.maximum(np.abs(want), span.reshape((-1,) + (1,) * (want.ndim - 1)))
        fin = np.isfinite(want)
        if fin.any():
            worst = max(worst, float((np.abs(got - want)[fin] / np.where(bar[fin] > 0, bar[fin], 1.0)).max()))
    print(f"{tag}: entries that differ {wrong}, derived worst {worst:.3g} of the bar, N {o['count'].tolist()}")
    for k in TABLES:
        assert m[k].dtype == np.int64 and np.array_equal(m[k], o[k]), (tag, k)
    for k in ("lo", "hi"):
        assert m[k].dtype == np.float32 and np.array_equal(m[k].view(np.int32), o[k].view(np.int32)), (tag, k)
    assert worst <= 1.0, tag


# ---------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("BJ", PARAMS, ids=lambda p: f"B{p[0]}-J{p[1]}")
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", ["white", "smooth"])
def test_fields_match_the_oracle(kind, shape, BJ):
    B, J = BJ
    pred, truth = field(kind, shape)
    o = oracle(kind, shape, B, J)
    m, sc = measure(pred, truth, bins=B, joint=J)
    check_against(f"{kind} {shape} B {B} J {J}", m, o)
    assert (m["count"] == shape[1] * shape[2]).all()
    assert (m["hist_truth"][:, 0] == 0).all() and (m["hist_truth"][:, B + 1] == 0).all()
    assert m["joint"].shape == (shape[0], J, J) and m["q_pred"].shape == (shape[0], len(do.DEFAULT_PROBS))


def test_the_smooth_field_is_the_contended_case():
    """At B = 256 most segments of 64 neighbouring pixels of a row share one bin."""
    shape = SHAPES[3]
    _, truth = field("smooth", shape)
    o = oracle("smooth", shape, 256, 32)
    n = one = 0
    for c in range(shape[0]):
        k = do.bin_index(truth[c], o["lo"][c], o["hi"][c], 256)[:, :512].reshape(shape[1], 8, 64)
        one += int((k.max(2) == k.min(2)).sum())
        n += k.shape[0] * 8
    print(f"smooth: {one} of {n} 64-pixel segments lie in one bin")
    assert one >= 0.6 * n


@pytest.mark.parametrize("kind", ["white", "smooth"])
def test_every_variant_of_the_kernel_gives_the_same_tables(kind):
    shape = SHAPES[3]
    pred, truth = field(kind, shape)
    o = oracle(kind, shape, 256, 32)
    for flags in (MERGE_RUNS, ONE_COPY, COPY_BY_WAVE, MERGE_RUNS | ONE_COPY, MERGE_RUNS | COPY_BY_WAVE):
        m, _ = measure(pred, truth, flags=flags)
        check_against(f"{kind} flags {flags}", m, o)


# ------------------------------------------------------------------ 2. mask and range
def test_a_coast_in_both_fields():
    shape = SHAPES[3]
    pred, truth = (v.copy() for v in field("white", shape))
    rng = np.random.default_rng(5)
    truth[0, 100:180, 200:420] = np.nan  # a block
    truth[rng.random(shape) < 0.01] = np.nan  # scattered
    pred[rng.random(shape) < 0.01] = np.nan  # elsewhere
    pred[1, 17, 33] = np.inf
    truth[1, 250, 3] = -np.inf
    o = do.distribution(pred, truth)
    assert (o["count"] < shape[1] * shape[2] - 2000).all() and o["count"][0] < o["count"][1]
    m, _ = measure(pred, truth)
    check_against("coast", m, o)


def test_a_channel_without_a_used_pixel():
    shape = SHAPES[1]
    pred, truth = (v.copy() for v in field("white", shape))
    pred[0] = np.nan
    o = do.distribution(pred, truth, bins=16, joint=4)
    m, _ = measure(pred, truth, bins=16, joint=4)
    check_against("empty channel", m, o)
    assert m["count"][0] == 0 and np.isnan(m["pss"][0]) and np.isnan(m["q_bias"][0]).all() and np.isnan(m["lo"][0])
    assert (m["hist_pred"][0] == 0).all() and (m["joint"][0] == 0).all() and np.isfinite(m["pss"][1])


def test_a_constant_truth_splits_the_prediction_exactly():
    truth = np.full((1, 40, 70), 290.25, dtype=np.float32)
    pred = truth.copy()
    pred[0, :7] = 290.0
    pred[0, 7:10, :35] = 291.0
    o = do.distribution(pred, truth, bins=16, joint=4)
    m, _ = measure(pred, truth, bins=16, joint=4)
    check_against("constant truth", m, o)
    want = np.zeros(18, dtype=np.int64)
    want[0], want[16], want[17] = 7 * 70, 40 * 70 - 7 * 70 - 105, 105
    assert np.array_equal(m["hist_pred"][0], want) and m["hist_truth"][0][16] == 2800
    assert m["lo"][0] == m["hi"][0] == np.float32(290.25) and m["w1"][0] == 0.0


def test_a_caller_range_narrower_than_the_truth():
    shape = SHAPES[1]
    pred, truth = field("white", shape)
    rng_ = (289.5, 290.75)
    o = do.distribution(pred, truth, bins=16, joint=32, value_range=rng_)
    assert (o["hist_truth"][:, 0] > 100).all() and (o["hist_truth"][:, 17] > 100).all()
    m, _ = measure(pred, truth, bins=16, joint=32, value_range=rng_)
    check_against("caller range", m, o)
    assert (m["lo"] == np.float32(289.5)).all() and (m["hi"] == np.float32(290.75)).all()


# ----------------------------------------------------- 3. the index clamp, through the C ABI
def raw_call(pred, truth, B, J, probs=do.DEFAULT_PROBS, lo_hi=None, canary=8):
    """srmi_distribution on buffers that carry `canary` words after each output and after the
    workspace -> (rc, outputs as numpy, the canaries' state)."""
    d = dev()
    lib = _lib.load()
    Cn, H, W = pred.shape
    P = len(probs)
    nbytes = distribution_workspace(Cn, H, W, B, J)
    ws = torch.full((nbytes + 8 * canary,), 0x5A, dtype=torch.uint8, device=d)
    sizes = {"hist": Cn * 2 * (B + 2), "joint": Cn * J * J, "range": Cn * 2, "count": Cn, "derived": Cn * (4 + 2 * P)}
    dtypes = {"hist": torch.int64, "joint": torch.int64, "range": torch.float32, "count": torch.int64,
              "derived": torch.float64}
    bufs = {k: torch.full((sizes[k] + canary,), -7, dtype=dtypes[k], device=d) for k in sizes}
    a, b = torch.tensor(pred, device=d), torch.tensor(truth, device=d)
    rc = lib.srmi_distribution(ptr(a), ptr(b), Cn, H, W, B, J, None if lo_hi is None else (C.c_float * 2)(*lo_hi),
                               (C.c_double * max(P, 1))(*probs), P, ptr(ws), nbytes, ptr(bufs["hist"]),
                               ptr(bufs["joint"]), ptr(bufs["range"]), ptr(bufs["count"]), ptr(bufs["derived"]), 0,
                               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    intact = all(bool((bufs[k][sizes[k]:] == -7).all()) for k in sizes) and bool((ws[nbytes:] == 0x5A).all())
    out = {k: bufs[k][:sizes[k]].cpu().numpy() for k in sizes}
    return rc, out, intact


def test_huge_values_go_to_under_and_over_and_touch_nothing_else():
    shape = SHAPES[1]
    pred, truth = (v.copy() for v in field("white", shape))
    flat = pred.reshape(-1)
    flat[0::7] = 3e38
    flat[1::7] = -3e38
    flat[2::7] = 1e6
    flat[3::7] = -1e6
    flat[4::11] = 3.4028235e38
    for B, J, lo_hi in ((256, 32, None), (4096, 64, None), (2, 2, (289.0, 291.0))):
        o = do.distribution(pred, truth, bins=B, joint=J, value_range=lo_hi)
        rc, out, intact = raw_call(pred, truth, B, J, lo_hi=lo_hi)
        assert rc == 0 and intact
        Cn = shape[0]
        hist = out["hist"].reshape(Cn, 2, B + 2)
        assert np.array_equal(hist[:, 0], o["hist_pred"]) and np.array_equal(hist[:, 1], o["hist_truth"])
        assert np.array_equal(out["joint"].reshape(Cn, J, J), o["joint"]) and np.array_equal(out["count"], o["count"])
        assert np.array_equal(out["range"].reshape(Cn, 2)[:, 0].view(np.int32), o["lo"].view(np.int32))
        assert np.allclose(out["derived"].reshape(Cn, -1), o["derived"], rtol=1e-12, atol=0)
        assert (hist[:, 0, 0] > 400).all() and (hist[:, 0, B + 1] > 400).all()


# ---------------------------------------------------------- 4. reproducible, capturable
def test_bit_identical_runs_and_no_dependence_on_the_workspace():
    d = dev()
    shape = SHAPES[3]
    pred, truth = (torch.tensor(v, device=d) for v in field("smooth", shape))
    sc = DistributionScore(shape, device=d)
    outs = ("hist", "joint_hist", "range", "count", "derived", "q_bias")
    sc.measure(pred, truth)
    first = {k: getattr(sc, k).clone() for k in outs}
    sc.measure(pred, truth)
    for k in outs:
        assert torch.equal(bits(getattr(sc, k)), bits(first[k])), k
    sc.workspace.fill_(0xFF)
    for k in outs:
        getattr(sc, k).fill_(-7)
    sc.measure(pred, truth)
    for k in outs:
        assert torch.equal(bits(getattr(sc, k)), bits(first[k])), k


def test_measure_is_capturable_on_one_stream():
    d = dev()
    shape = SHAPES[2]
    pred, truth = (torch.tensor(v, device=d) for v in field("white", shape))
    eager = DistributionScore(shape, device=d)
    me = {k: v.clone() for k, v in eager.measure(pred, truth).items()}
    sc = DistributionScore(shape, device=d)
    sc.measure(pred, truth)  # warm-up outside capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(device=d)
    s.wait_stream(torch.cuda.current_stream(d))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            m = sc.measure(pred, truth)
    torch.cuda.current_stream(d).wait_stream(s)
    for _ in range(2):
        for k in ("hist", "joint_hist", "range", "count", "derived", "q_bias"):
            getattr(sc, k).fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        for k in me:
            assert torch.equal(bits(m[k]), bits(me[k])), k


# --------------------------------------------------------------------- 5. refusals
REFUSALS = ["null-a", "null-b", "null-workspace", "null-hist", "null-joint", "null-range", "null-count", "null-derived",
            "null-probs", "short-workspace", "B1", "B4097", "J-1", "J65", "nprobs17", "nprobs-1", "prob0", "prob1",
            "prob-nan", "range-equal", "range-reversed", "range-nan", "range-inf", "C0", "H0", "W0", "HW-2^31",
            "flags8"]


@pytest.mark.parametrize("case", REFUSALS)
def test_refusals_leave_the_outputs_untouched(case):
    d = dev()
    lib = _lib.load()
    Cn, H, W, B, J = 1, 16, 16, 16, 4
    a = torch.zeros((1, 16, 16), device=d)
    nbytes = distribution_workspace(Cn, H, W, B, J)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=d)
    hist = torch.full((1, 2, 18), -3, dtype=torch.int64, device=d)
    joint = torch.full((1, 4, 4), -3, dtype=torch.int64, device=d)
    rng_ = torch.full((1, 2), -7.0, device=d)
    count = torch.full((1,), -3, dtype=torch.int64, device=d)
    probs, nprobs, lo_hi, flags = [0.5, 0.9], 2, None, 0
    derived = torch.full((1, 8), -7.0, dtype=torch.float64, device=d)
    Cn = 0 if case == "C0" else Cn
    H = 0 if case == "H0" else 65536 if case == "HW-2^31" else H
    W = 0 if case == "W0" else 32768 if case == "HW-2^31" else W
    B = {"B1": 1, "B4097": 4097}.get(case, B)
    J = {"J-1": -1, "J65": 65}.get(case, J)
    nprobs = {"nprobs17": 17, "nprobs-1": -1}.get(case, nprobs)
    probs = {"prob0": [0.5, 0.0], "prob1": [1.0, 0.5], "prob-nan": [float("nan"), 0.5]}.get(case, probs)
    lo_hi = {"range-equal": (1.0, 1.0), "range-reversed": (2.0, 1.0), "range-nan": (float("nan"), 1.0),
             "range-inf": (0.0, float("inf"))}.get(case)
    flags = 8 if case == "flags8" else 0

    def arg(name, t):
        return None if case == "null-" + name else ptr(t)

    cprobs = None if case == "null-probs" else (C.c_double * 17)(*(probs + [0.5] * (17 - len(probs))))
    rc = lib.srmi_distribution(arg("a", a), arg("b", a), Cn, H, W, B, J,
                               None if lo_hi is None else (C.c_float * 2)(*lo_hi), cprobs, nprobs, arg("workspace", ws), nbytes - (case == "short-workspace"), arg("hist", hist),
                               arg("joint", joint), arg("range", rng_), arg("count", count), arg("derived", derived),
                               flags, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == _lib.SRMI_ERR_ARG
    assert (hist == -3).all() and (joint == -3).all() and (rng_ == -7.0).all() and (count == -3).all()
    assert (derived == -7.0).all() and (ws == 0).all()
    if case in ("B1", "B4097", "J-1", "J65", "C0", "H0", "W0", "HW-2^31"):
        n = C.c_size_t(5)
        assert lib.srmi_distribution_workspace(Cn, H, W, B, J, C.byref(n)) == _lib.SRMI_ERR_ARG and n.value == 5
        with pytest.raises(ValueError):
            DistributionScore((Cn, H, W), bins=B, joint=J, device=d)
    if case.startswith("prob"):
        with pytest.raises(ValueError):
            DistributionScore((1, 16, 16), probs=probs, device=d)
    if case == "nprobs17":
        with pytest.raises(ValueError):
            DistributionScore((1, 16, 16), probs=[0.5] * 17, device=d)
    if case.startswith("range"):
        with pytest.raises(ValueError):
            DistributionScore((1, 16, 16), value_range=lo_hi, device=d)
    if case == "flags8":
        with pytest.raises(ValueError):
            DistributionScore((1, 16, 16), flags=8, device=d)


def test_measure_refuses_wrong_inputs():
    d = dev()
    sc = DistributionScore((1, 16, 20), device=d)
    ok = torch.zeros((1, 16, 20), device=d)
    for bad in (torch.zeros((1, 20, 16), device=d), ok.double(), ok.cpu(), torch.zeros((1, 20, 16), device=d).mT):
        with pytest.raises(ValueError):
            sc.measure(bad, ok)
        with pytest.raises(ValueError):
            sc.measure(ok, bad)


# -------------------------------------------------------------------- 6. end to end
def _field(rng, C_, h, w):
    base = rng.randn(C_, h, w)
    return (base + np.roll(base, 1, 1) + np.roll(base, 1, 2)).astype(np.float32)


@pytest.mark.parametrize("land", [False, True], ids=["sea", "land"])
def test_score_distribution_is_score_plus_the_measure_of_its_images(land):
    d = dev()
    spec, model, flat = _small_rcan()
    rng = np.random.RandomState(71)
    hr = _field(rng, 1, 160, 224) * 2 + 5
    if land:
        hr[0, 40:72, 100:140] = np.nan  # land on whole LR pixels
    kw = dict(tile_lr=TILE, overlap=(4, 4), land=land, device=d)
    rs = RegionSuperResolver(spec, flat.to(d), (1, 40, 56), **kw)
    plain = RegionSuperResolver(spec, flat.to(d), (1, 40, 56), **kw)
    hrd = torch.tensor(hr, device=d)
    images, losses, dist = rs.score_distribution(hrd)
    images0, losses0 = plain.score(hrd)
    assert set(dist) == {"model", "interpolated"}
    for k in ("input", "interpolated", "model"):
        assert torch.equal(bits(images[k]), bits(images0[k]))
    for k in ("model", "interpolated"):
        assert torch.equal(bits(losses[k]), bits(losses0[k]))
        m = DistributionScore((1, 160, 224), device=d).measure(images[k], hrd)
        assert set(m) == set(dist[k])
        for q in m:
            assert torch.equal(bits(m[q]), bits(dist[k][q])), (k, q)
        o = do.distribution(images[k].cpu().numpy(), hr)
        check_against(f"score_distribution {k} land={land}", {q: v.cpu().numpy() for q, v in dist[k].items()}, o)
        n = int(dist[k]["count"].item())
        assert (0 < n < 160 * 224) if land else n == 160 * 224
    # a second call reuses the buffers and gives the same bits; other arguments get their own
    keep = {k: dist[k]["hist_pred"].clone() for k in dist}
    scorers = dict(rs._distribution)
    _, _, again = rs.score_distribution(hrd)
    assert rs._distribution == scorers and len(scorers) == 1
    for k in keep:
        assert again[k]["hist_pred"].data_ptr() == dist[k]["hist_pred"].data_ptr()
        assert torch.equal(again[k]["hist_pred"], keep[k])
    _, _, other = rs.score_distribution(hrd, bins=16, joint=0, probs=(0.5,), value_range=(0.0, 10.0))
    assert len(rs._distribution) == 2 and other["model"]["hist_pred"].shape == (1, 18)
    assert other["model"]["q_bias"].shape == (1, 1) and float(other["model"]["hi"]) == 10.0
