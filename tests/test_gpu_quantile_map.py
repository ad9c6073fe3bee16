"""Quantile mapping on the HIP path: srmi_quantile_map_accumulate / _fit / _apply and
srmi.quantile_map.QuantileMap against the numpy oracle (tests/quantile_map_oracle.py), and
RegionSuperResolver(quantile_map=...) end to end.

Bars.  The accumulated tables and the count are held to the oracle EXACTLY (array_equal):
every device operation on them is an integer operation or one of the fp32 operations of the
definition, which numpy reproduces bit for bit.  The knots are fp64 on both sides, an integer
search and then at most four roundings of exact integers and of the range: they are held to
1e-12 (hi - lo), the bar tests/test_gpu_distribution.py uses for fp64 derived values (its
docstring has the reason: five orders below anything an fp32 intermediate would leave).  The
fp32 table and meta must be the rounding of the DEVICE's own knots, bit for bit, and the mapped
field, computed by the oracle from the device's table and meta, must be the device's bit for
bit (int32 view): every operation of the apply is an fp32 one rounded on its own.  Every test
prints the number of entries or elements that differ before it asserts.  Measured on an
MI355X: 0 entries, 0 elements and 0 of the knots' bar on every case.

The shapes are the smallest at which the kernels can go wrong: one pixel; a ragged one whose
second plane is off 16-byte alignment (also with a base offset by one element, so that base
alone is unaligned); SPAN_H x SPAN_W = 8192 pixels is what one histogram workgroup covers in
one step (kQmSpan of csrc/quantile_map.hip) and ASPAN_H x ASPAN_W = 2048 what one apply
workgroup does (kQmApplySpan), and a shape exceeds each by one pixel on each axis; the last
has many workgroups, so the merge of the partial tables is exercised."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import quantile_map_oracle as qo  # noqa: E402
from srmi import _lib  # noqa: E402
from srmi._lib import ptr  # noqa: E402
from srmi.quantile_map import QuantileMap, accumulate_workspace  # noqa: E402
from srmi.superres import RegionSuperResolver  # noqa: E402
from test_gpu_distribution import _field, field  # noqa: E402
from test_gpu_inference import _small_rcan  # noqa: E402

SPAN_H, SPAN_W = 64, 128  # kQmSpan = 8192 pixels of a histogram workgroup per step
ASPAN_H, ASPAN_W = 32, 64  # kQmApplySpan = 2048 pixels of an apply workgroup per step
SHAPES = [(1, 1, 1), (2, 37, 53), (1, ASPAN_H + 1, ASPAN_W + 1), (1, SPAN_H + 1, SPAN_W + 1), (2, 300, 517)]
BINS = [2, 16, 256, 4096]
TILE = (16, 32)  # the smallest 16-row tile the inference engine takes
IDS = dict(ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s))


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


def stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def base_of(shape):
    """the detail base: a large-scale gradient around 290, so that src - base is the detail"""
    Cn, H, W = shape
    c, y, x = np.meshgrid(np.arange(Cn), np.arange(H), np.arange(W), indexing="ij")
    b = (290.0 + 0.8 * np.sin(2 * np.pi * (y / (2.3 * H) + x / (3.1 * W)) + c)).astype(np.float32)
    b.setflags(write=False)
    return b


def ranges(Cn, detail):
    """one pair per channel, the second narrower: both fields leave it on both sides"""
    r = [(-3.5, 3.75), (-2.0, 2.5)] if detail else [(286.5, 293.75), (288.0, 292.5)]
    return np.asarray(r[:Cn], dtype=np.float32)


def inputs(kind, shape, detail):
    src, truth = field(kind, shape)
    return src, truth, (base_of(shape) if detail else None), ranges(shape[0], detail)


@functools.lru_cache(maxsize=None)
def oracle_tables(kind, shape, B, detail):
    src, truth, base, rg = inputs(kind, shape, detail)
    return qo.accumulate(src, truth, base, B, rg)


def crange(rg):
    return (C.c_float * rg.size)(*rg.reshape(-1).tolist())


def T(a):
    return None if a is None else torch.tensor(a, device=dev())


def dev_accumulate(src, truth, base, B, rg, first=1, hist=None, count=None, ws=None):
    """srmi_quantile_map_accumulate on device tensors -> (hist, count) device tensors"""
    d = dev()
    Cn, H, W = src.shape
    if ws is None:
        ws = torch.empty(accumulate_workspace(Cn, H, W, B), dtype=torch.uint8, device=d)
    if hist is None:
        hist = torch.full((Cn, 2, B + 2), -7, dtype=torch.int64, device=d)
        count = torch.full((Cn,), -7, dtype=torch.int64, device=d)
    rc = _lib.load().srmi_quantile_map_accumulate(ptr(src), ptr(truth), ptr(base), Cn, H, W, B, crange(rg), first,
                                                  ptr(ws), ws.numel(), ptr(hist), ptr(count), stream())
    assert rc == 0
    return hist, count


def dev_fit(hist, count, B, rg, tail):
    d = dev()
    Cn = hist.shape[0]
    knots = torch.full((Cn, B + 3), -7.0, dtype=torch.float64, device=d)
    table = torch.full((Cn, B + 3), -7.0, dtype=torch.float32, device=d)
    meta = torch.full((Cn, 4), -7.0, dtype=torch.float32, device=d)
    rc = _lib.load().srmi_quantile_map_fit(ptr(hist), ptr(count), Cn, B, crange(rg), tail, ptr(knots), ptr(table),
                                           ptr(meta), stream())
    assert rc == 0
    return knots, table, meta


def dev_apply(x, base, B, table, meta, strength, out):
    Cn, H, W = x.shape
    rc = _lib.load().srmi_quantile_map_apply(ptr(x), ptr(base), Cn, H, W, B, ptr(table), ptr(meta), strength, ptr(out),
                                             stream())
    assert rc == 0
    return out


def check_fit(tag, knots, table, meta, hist, B, rg, tail):
    """the fit bars of the module docstring; prints before it asserts.  -> the oracle's knots"""
    want, _, _ = qo.fit(hist, B, rg, tail)
    got = knots.cpu().numpy()
    span = (rg[:, 1].astype(np.float64) - rg[:, 0].astype(np.float64))[:, None]
    worst = float((np.abs(got - want) / (1e-12 * span)).max())
    t_wrong = int((bits(table) != bits(knots.float())).sum())
    m_want = qo.meta_of(got, rg, B)
    m_wrong = int((meta.cpu().numpy().view(np.int32) != m_want.view(np.int32)).sum())
    print(f"{tag}: knots worst {worst:.3g} of the bar, table entries that differ {t_wrong}, meta {m_wrong}")
    assert worst <= 1.0 and t_wrong == 0 and m_wrong == 0, tag
    assert (np.diff(got, axis=1) >= 0).all(), tag
    return want


# ------------------------------------------------------------------- 1. accumulate
@pytest.mark.parametrize("B", BINS)
@pytest.mark.parametrize("shape", SHAPES, **IDS)
@pytest.mark.parametrize("detail", [False, True], ids=["value", "detail"])
@pytest.mark.parametrize("kind", ["white", "smooth"])
def test_tables_equal_the_oracle(kind, detail, shape, B):
    src, truth, base, rg = inputs(kind, shape, detail)
    want_h, want_n = oracle_tables(kind, shape, B, detail)
    hist, count = dev_accumulate(T(src), T(truth), T(base), B, rg)
    torch.cuda.synchronize()
    wrong = int((hist.cpu().numpy() != want_h).sum())
    print(f"{kind} {shape} B {B} detail {detail}: table entries that differ {wrong}, N {want_n.tolist()}")
    assert wrong == 0 and np.array_equal(count.cpu().numpy(), want_n)
    assert (want_n == shape[1] * shape[2]).all()
    if shape[1] * shape[2] > 1000 and kind == "white":
        assert (want_h[:, :, 0] > 0).all() and (want_h[:, :, B + 1] > 0).all()  # both outer entries in use


def test_a_base_pointer_off_16_byte_alignment():
    """src and truth aligned, base one element into its buffer: the run loads of the base alone
    take the scalar path."""
    shape, B = SHAPES[1], 16
    src, truth, base, rg = inputs("white", shape, True)
    want_h, want_n = oracle_tables("white", shape, B, True)
    buf = torch.zeros(base.size + 1, device=dev())
    buf[1:] = T(base).reshape(-1)
    off = buf[1:].view(shape)
    assert off.data_ptr() % 16 == 4
    hist, count = dev_accumulate(T(src), T(truth), off, B, rg)
    assert np.array_equal(hist.cpu().numpy(), want_h) and np.array_equal(count.cpu().numpy(), want_n)
    # and the apply, with x and out aligned
    knots, table, meta = dev_fit(hist, count, B, rg, 4)
    out = dev_apply(T(src), off, B, table, meta, 1.0, torch.empty(shape, device=dev()))
    want = qo.apply(src, base, table.cpu().numpy(), meta.cpu().numpy(), B)
    assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))


def awkward(shape, detail):
    """NaN scattered differently in src, truth and base, +-Inf, values exactly at lo and hi,
    huge values"""
    src, truth, base, rg = inputs("white", shape, detail)
    src, truth = src.copy(), truth.copy()
    base = None if base is None else base.copy()
    rng = np.random.default_rng(17)
    src[rng.random(shape) < 0.02] = np.nan
    truth[rng.random(shape) < 0.02] = np.nan
    truth[0, 10:20, 5:30] = np.nan
    if base is not None:
        base[rng.random(shape) < 0.02] = np.nan
    fs, ft = src.reshape(-1), truth.reshape(-1)
    fs[0::41], fs[1::41], fs[2::41], fs[3::41] = 3e38, -3e38, 1e6, -1e6
    ft[4::43], ft[5::43] = 3.4028235e38, -3.4028235e38
    fs[6::47], ft[7::47] = np.inf, -np.inf
    lo, hi = rg[0]
    if base is None:
        fs[8::53], fs[9::53], ft[10::53], ft[11::53] = lo, hi, hi, lo
    else:  # base is 290.0 there, so the detail is exactly lo and hi (290 + lo and 290 + hi are fp32 numbers)
        fb = base.reshape(-1)
        for k in (8, 9, 10, 11):
            fb[k::53] = 290.0
        fs[8::53], fs[9::53], ft[10::53], ft[11::53] = 290.0 + lo, 290.0 + hi, 290.0 + hi, 290.0 + lo
    return src, truth, base, rg


@pytest.mark.parametrize("detail", [False, True], ids=["value", "detail"])
def test_nan_infinities_edges_and_huge_values(detail):
    shape = SHAPES[4]
    src, truth, base, rg = awkward(shape, detail)
    for B in (2, 256, 4096):
        want_h, want_n = qo.accumulate(src, truth, base, B, rg)
        assert (want_n < shape[1] * shape[2] - 4000).all() and (want_h[0, :, B] > 0).all()
        hist, count = dev_accumulate(T(src), T(truth), T(base), B, rg)
        wrong = int((hist.cpu().numpy() != want_h).sum())
        print(f"awkward B {B} detail {detail}: table entries that differ {wrong}, N {want_n.tolist()}")
        assert wrong == 0 and np.array_equal(count.cpu().numpy(), want_n)


def test_two_accumulations_add_first_overwrites_and_the_workspace_does_not_matter():
    shape, B = SHAPES[4], 256
    s1, t1, base, rg = inputs("white", shape, True)
    s2, t2, _, _ = inputs("smooth", shape, True)
    h1, n1 = oracle_tables("white", shape, B, True)
    h2, n2 = oracle_tables("smooth", shape, B, True)
    d = dev()
    ws = torch.full((accumulate_workspace(*shape, B),), 0xFF, dtype=torch.uint8, device=d)
    hist, count = dev_accumulate(T(s1), T(t1), T(base), B, rg, ws=ws)
    assert np.array_equal(hist.cpu().numpy(), h1)
    dev_accumulate(T(s2), T(t2), T(base), B, rg, first=0, hist=hist, count=count, ws=ws)
    assert np.array_equal(hist.cpu().numpy(), h1 + h2) and np.array_equal(count.cpu().numpy(), n1 + n2)
    ws.fill_(0x5A)
    dev_accumulate(T(s2), T(t2), T(base), B, rg, first=1, hist=hist, count=count, ws=ws)
    assert np.array_equal(hist.cpu().numpy(), h2) and np.array_equal(count.cpu().numpy(), n2)
    # the object: first call overwrites, later calls add, reset starts over
    qm = QuantileMap(shape[0], rg, bins=B, on="detail", device=d)
    qm.hist.fill_(-9)
    qm.accumulate(T(s1), T(t1), T(base))
    qm.accumulate(T(s2), T(t2), T(base))
    assert np.array_equal(qm.hist.cpu().numpy(), h1 + h2)
    qm.reset()
    qm.accumulate(T(s2), T(t2), T(base))
    assert np.array_equal(qm.hist.cpu().numpy(), h2) and np.array_equal(qm.state_dict()["count"], n2)


# -------------------------------------------------------------------------- 2. fit
@pytest.mark.parametrize("B", BINS)
@pytest.mark.parametrize("tail", [0, 16])
@pytest.mark.parametrize("detail", [False, True], ids=["value", "detail"])
@pytest.mark.parametrize("kind", ["white", "smooth"])
def test_knots_table_and_meta(kind, detail, tail, B):
    shape = SHAPES[4]
    _, _, _, rg = inputs(kind, shape, detail)
    want_h, want_n = oracle_tables(kind, shape, B, detail)
    knots, table, meta = dev_fit(T(want_h), T(want_n), B, rg, tail)
    check_fit(f"{kind} B {B} detail {detail} tail {tail}", knots, table, meta, want_h, B, rg, tail)


@pytest.mark.parametrize("B", BINS)
def test_fit_on_awkward_tables(B):
    """equal tables (the identity, exactly), an all-NaN channel (N == 0: the identity), a
    one-pixel field, tables with long empty stretches, and a tail_count no knot meets"""
    rg = ranges(2, False)
    e = np.stack([qo.edges(*r, B) for r in rg])
    rng = np.random.default_rng(B)
    same = rng.integers(0, 40, (2, 1, B + 2)) * (rng.random((2, 1, B + 2)) < 0.5)
    same = np.repeat(same, 2, axis=1).astype(np.int64)
    knots, table, meta = dev_fit(T(same), T(same[:, 0].sum(1)), B, rg, 0)
    assert np.array_equal(knots.cpu().numpy(), e) and (meta[:, 2:] == 0).all()
    check_fit(f"equal tables B {B}", knots, table, meta, same, B, rg, 0)

    src, truth = (v.copy() for v in field("white", SHAPES[1]))
    src[0] = np.nan
    hist, count = dev_accumulate(T(src), T(truth), None, B, rg)
    knots, table, meta = dev_fit(hist, count, B, rg, 4)
    assert count[0] == 0 and np.array_equal(knots[0].cpu().numpy(), e[0]) and not np.array_equal(
        knots[1].cpu().numpy(), e[1])
    check_fit(f"all-NaN channel B {B}", knots, table, meta, hist.cpu().numpy(), B, rg, 4)

    one = np.zeros((1, 2, B + 2), dtype=np.int64)
    one[0, 0, 1], one[0, 1, B] = 1, 1
    knots, table, meta = dev_fit(T(one), T(np.ones(1, dtype=np.int64)), B, rg[:1], 0)
    check_fit(f"one pixel B {B}", knots, table, meta, one, B, rg[:1], 0)

    gaps = np.zeros((2, 2, B + 2), dtype=np.int64)
    gaps[:, 0, ::max(1, B // 7)] = 1000
    gaps[:, 1, B // 2:B // 2 + 2] = gaps[:, 0].sum(1)[:, None] // 2
    gaps[:, 1, 0] += gaps[:, 0].sum(1) - gaps[:, 1].sum(1)
    for tail in (0, 16, 10 ** 9):
        knots, table, meta = dev_fit(T(gaps), T(gaps[:, 0].sum(1)), B, rg, tail)
        check_fit(f"gaps B {B} tail {tail}", knots, table, meta, gaps, B, rg, tail)
    assert np.array_equal(knots.cpu().numpy(), e)  # tail 10^9: no trusted knot


# ------------------------------------------------------------------------ 3. apply
@functools.lru_cache(maxsize=None)
def fitted(kind, shape, B, detail):
    """the device's table and meta for a field (made once), as device tensors"""
    _, _, _, rg = inputs(kind, shape, detail)
    want_h, want_n = oracle_tables(kind, shape, B, detail)
    _, table, meta = dev_fit(T(want_h), T(want_n), B, rg, 16 if shape[1] * shape[2] > 4096 else 0)
    torch.cuda.synchronize()
    return table, meta


def check_apply(tag, x, base, B, table, meta, strength, inplace):
    want = qo.apply(x, base, table.cpu().numpy(), meta.cpu().numpy(), B, strength)
    xd = T(x)
    out = xd if inplace else torch.full(x.shape, -7.0, device=dev())
    dev_apply(xd, T(base), B, table, meta, strength, out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    wrong = int((got.view(np.int32) != want.view(np.int32)).sum())
    print(f"{tag}: elements that differ {wrong} of {want.size}")
    assert wrong == 0, tag
    if not inplace:
        assert np.array_equal(xd.cpu().numpy().view(np.int32), x.view(np.int32)), tag
    return got


@pytest.mark.parametrize("B", BINS)
@pytest.mark.parametrize("shape", SHAPES, **IDS)
@pytest.mark.parametrize("detail", [False, True], ids=["value", "detail"])
@pytest.mark.parametrize("kind", ["white", "smooth"])
def test_the_mapped_field_is_the_oracles_bit_for_bit(kind, detail, shape, B):
    src, truth, base, rg = inputs(kind, shape, detail)
    table, meta = fitted(kind, shape, B, detail)
    tag = f"{kind} {shape} B {B} detail {detail}"
    a = check_apply(tag + " s 1 out of place", src, base, B, table, meta, 1.0, False)
    b = check_apply(tag + " s 1 in place", src, base, B, table, meta, 1.0, True)
    assert np.array_equal(a.view(np.int32), b.view(np.int32))
    check_apply(tag + " s 0.5 in place", src, base, B, table, meta, 0.5, True)
    check_apply(tag + " s 0.5 out of place", src, base, B, table, meta, 0.5, False)
    if shape[1] * shape[2] > 1000:
        assert np.abs(a - src).max() > 1e-3  # the map moves the field


@pytest.mark.parametrize("detail", [False, True], ids=["value", "detail"])
def test_apply_on_nan_infinities_and_values_beyond_both_ends(detail):
    shape, B = SHAPES[4], 256
    src, _, base, rg = awkward(shape, detail)
    fs = src.reshape(-1)
    nan_bits = np.array([0x7fc00000, 0xffc00001, 0x7f800001, 0x7fffffff], dtype=np.uint32).view(np.float32)
    fs[100:104] = nan_bits
    table, meta = fitted("white", shape, B, detail)
    for strength in (1.0, 0.5):
        for inplace in (False, True):
            got = check_apply(f"awkward detail {detail} s {strength} in place {inplace}", src, base, B, table, meta,
                              strength, inplace)
            g = got.reshape(-1)
            with np.errstate(invalid="ignore"):
                v = fs - base.reshape(-1) if detail else fs
            nanv = np.isnan(v)
            assert nanv.sum() > 4000 and np.array_equal(g.view(np.int32)[nanv], fs.view(np.int32)[nanv])
            if detail:
                only_base = np.isnan(base.reshape(-1)) & ~np.isnan(fs)
                assert only_base.sum() > 1000 and np.array_equal(g[only_base], fs[only_base])
            assert (fs == np.inf).sum() > 1000 and (g[fs == np.inf] == np.inf).all()
            assert np.array_equal(np.isnan(g), np.isnan(fs))


# ---------------------------------------------------------------------- 4. refusals
def _refusal_setup(B=16, Cn=1, H=16, W=16):
    d = dev()
    a = torch.zeros((Cn, H, W), device=d)
    ws = torch.zeros(accumulate_workspace(Cn, H, W, B) + 16, dtype=torch.uint8, device=d)
    out = dict(hist=torch.full((Cn, 2, B + 2), -3, dtype=torch.int64, device=d),
               count=torch.full((Cn,), -3, dtype=torch.int64, device=d),
               knots=torch.full((Cn, B + 3), -7.0, dtype=torch.float64, device=d),
               table=torch.full((Cn, B + 3), -7.0, device=d), meta=torch.full((Cn, 4), -7.0, device=d),
               out=torch.full((Cn, H, W), -7.0, device=d))
    return d, a, ws, out


def _untouched(out, ws):
    torch.cuda.synchronize()
    assert (out["hist"] == -3).all() and (out["count"] == -3).all() and (out["knots"] == -7.0).all()
    assert (out["table"] == -7.0).all() and (out["meta"] == -7.0).all() and (out["out"] == -7.0).all()
    assert (ws == 0).all()


BAD_RANGES = {"range-equal": (1.0, 1.0), "range-reversed": (2.0, 1.0), "range-nan": (float("nan"), 1.0),
              "range-inf": (0.0, float("inf")), "range-overflow": (-3e38, 3e38), "range-null": None}
ACC_REFUSALS = ["null-src", "null-truth", "null-workspace", "null-hist", "null-count", "short-workspace",
                "misaligned-workspace", "B1", "B4097", "C0", "C17", "H0", "W0", "HW-2^31"] + list(BAD_RANGES)


@pytest.mark.parametrize("case", ACC_REFUSALS)
def test_accumulate_refusals_leave_the_outputs_untouched(case):
    d, a, ws, out = _refusal_setup()
    lib = _lib.load()
    Cn, H, W, B = 1, 16, 16, 16
    nbytes = ws.numel() - 16
    Cn = {"C0": 0, "C17": 17}.get(case, Cn)
    H = 0 if case == "H0" else 65536 if case == "HW-2^31" else H
    W = 0 if case == "W0" else 32768 if case == "HW-2^31" else W
    B = {"B1": 1, "B4097": 4097}.get(case, B)
    rg = BAD_RANGES.get(case, (0.0, 1.0))
    crg = None if rg is None else (C.c_float * 34)(*(list(rg) * 17))

    def arg(name, t):
        return None if case == "null-" + name else ptr(t)

    wsp = ptr(ws) + (4 if case == "misaligned-workspace" else 0)
    rc = lib.srmi_quantile_map_accumulate(arg("src", a), arg("truth", a), None, Cn, H, W, B, crg, 1,
                                          None if case == "null-workspace" else wsp,
                                          nbytes - (case == "short-workspace"), arg("hist", out["hist"]),
                                          arg("count", out["count"]), stream())
    assert rc == _lib.SRMI_ERR_ARG
    _untouched(out, ws)
    if case in ("B1", "B4097", "C0", "C17", "H0", "W0", "HW-2^31"):
        n = C.c_size_t(5)
        assert lib.srmi_quantile_map_accumulate_workspace(Cn, H, W, B, C.byref(n)) == _lib.SRMI_ERR_ARG and n.value == 5
    if case in ("B1", "B4097", "C0", "C17") or case.startswith("range"):
        with pytest.raises(ValueError):
            QuantileMap(Cn, rg, bins=B, device=d)
    assert lib.srmi_quantile_map_accumulate_workspace(1, 16, 16, 16, None) == _lib.SRMI_ERR_ARG


FIT_REFUSALS = ["null-hist", "null-count", "null-knots", "null-table", "null-meta", "B1", "B4097", "C0", "C17",
                "tail-1"] + list(BAD_RANGES)


@pytest.mark.parametrize("case", FIT_REFUSALS)
def test_fit_refusals_leave_the_outputs_untouched(case):
    d, a, ws, out = _refusal_setup()
    Cn, B = {"C0": 0, "C17": 17}.get(case, 1), {"B1": 1, "B4097": 4097}.get(case, 16)
    rg = BAD_RANGES.get(case, (0.0, 1.0))
    crg = None if rg is None else (C.c_float * 34)(*(list(rg) * 17))

    def arg(name):
        return None if case == "null-" + name else ptr(out[name])

    rc = _lib.load().srmi_quantile_map_fit(arg("hist"), arg("count"), Cn, B, crg, -1 if case == "tail-1" else 4,
                                           arg("knots"), arg("table"), arg("meta"), stream())
    assert rc == _lib.SRMI_ERR_ARG
    _untouched(out, ws)


APPLY_REFUSALS = ["null-x", "null-table", "null-meta", "null-out", "out-is-base", "out-overlaps-base",
                  "out-overlaps-x", "B1", "B4097", "C0", "C17", "H0", "W0", "HW-2^31", "strength-0.1", "strength1.5",
                  "strength-nan", "strength-inf"]


@pytest.mark.parametrize("case", APPLY_REFUSALS)
def test_apply_refusals_leave_the_outputs_untouched(case):
    d, a, ws, out = _refusal_setup()
    Cn, H, W, B = 1, 16, 16, 16
    Cn = {"C0": 0, "C17": 17}.get(case, Cn)
    H = 0 if case == "H0" else 65536 if case == "HW-2^31" else H
    W = 0 if case == "W0" else 32768 if case == "HW-2^31" else W
    B = {"B1": 1, "B4097": 4097}.get(case, B)
    strength = {"strength-0.1": -0.1, "strength1.5": 1.5, "strength-nan": float("nan"),
                "strength-inf": float("inf")}.get(case, 1.0)
    big = torch.full((2 * 256,), -7.0, device=d)  # a buffer in which x / base and out can overlap by half
    x, base, o = ptr(a), None, ptr(out["out"])
    if case == "out-is-base":
        base = o
    elif case == "out-overlaps-base":
        base, o = ptr(big), ptr(big) + 4 * 128
    elif case == "out-overlaps-x":
        x, o = ptr(big), ptr(big) + 4 * 128
    x = None if case == "null-x" else x
    o = None if case == "null-out" else o
    rc = _lib.load().srmi_quantile_map_apply(x, base, Cn, H, W, B, None if case == "null-table" else ptr(out["table"]),
                                             None if case == "null-meta" else ptr(out["meta"]), strength, o, stream())
    assert rc == _lib.SRMI_ERR_ARG
    _untouched(out, ws)
    assert (big == -7.0).all()


def test_the_object_refuses_wrong_inputs():
    d = dev()
    qm = QuantileMap(1, (0.0, 1.0), bins=16, on="detail", device=d)
    ok = torch.zeros((1, 16, 20), device=d)
    with pytest.raises(RuntimeError):
        qm.apply(ok, ok)  # no table yet
    for bad in (torch.zeros((2, 16, 20), device=d), ok.double(), ok.cpu(), torch.zeros((1, 20, 16), device=d).mT):
        with pytest.raises(ValueError):
            qm.accumulate(bad, ok, ok)
    with pytest.raises(ValueError):
        qm.accumulate(ok, torch.zeros((1, 16, 24), device=d), ok)
    with pytest.raises(ValueError):
        qm.accumulate(ok, ok)  # a detail map needs its base
    qm.fit()
    assert (qm.meta[:, 2:] == 0).all()  # nothing accumulated: the identity
    for s in (-0.5, 1.5, float("nan")):
        with pytest.raises(ValueError):
            qm.apply(ok, ok, strength=s)
    with pytest.raises(ValueError):
        qm.apply(ok)
    with pytest.raises(ValueError):
        QuantileMap(1, (0.0, 1.0), on="value", device=d).accumulate(ok, ok, ok)  # a value map refuses one
    with pytest.raises(_lib.SrmiError):
        qm.apply(ok, ok, out=ok)  # out is base
    # strength 0 launches nothing: x itself, or a copy in out
    x = torch.rand((1, 16, 20), device=d)
    assert qm.apply(x, ok, strength=0.0) is x
    other = torch.zeros_like(x)
    assert qm.apply(x, ok, strength=0.0, out=other) is other and torch.equal(other, x)


# ------------------------------------------------------- 5. reproducible, capturable
def test_the_object_end_to_end_twice_and_from_a_loaded_state():
    d = dev()
    shape, B = SHAPES[4], 256
    src, truth, base, rg = inputs("white", shape, True)
    runs = []
    for _ in range(2):
        qm = QuantileMap(shape[0], rg, bins=B, on="detail", tail_count=16, device=d)
        qm.accumulate(T(src), T(truth), T(base))
        qm.fit()
        out = qm.apply(T(src), T(base))
        assert out is qm.out and qm.apply(T(src), T(base)).data_ptr() == out.data_ptr()  # nothing new is allocated
        runs.append((qm, {k: getattr(qm, k).clone() for k in ("hist", "count", "knots", "table", "meta", "out")}))
    for k, v in runs[0][1].items():
        assert torch.equal(bits(v), bits(runs[1][1][k])), k
    check_fit("object", qm.knots, qm.table, qm.meta, oracle_tables("white", shape, B, True)[0], B, rg, 16)
    want = qo.apply(src, base, qm.table.cpu().numpy(), qm.meta.cpu().numpy(), B)
    assert np.array_equal(runs[0][1]["out"].cpu().numpy().view(np.int32), want.view(np.int32))
    # the mapped detail has the truth's quantiles: the oracle's calibration, seen on the device's output
    got = runs[0][1]["out"].cpu().numpy()
    w_before = qo.w1_samples(src - base, truth - base)
    w_after = qo.w1_samples(got - base, truth - base)
    print(f"detail W1 {w_before:.4f} -> {w_after:.5f}")
    assert w_after < w_before
    other = QuantileMap(shape[0], (0.0, 1.0), bins=B, on="value", device=d)
    other.load_state_dict(qm.state_dict())
    assert other.fitted and other.on == "detail"
    for k in ("hist", "count", "knots", "table", "meta"):
        assert torch.equal(bits(getattr(other, k)), bits(getattr(qm, k))), k
    # from_histograms of a fixed-range distribution score is the value map of the same fields
    from srmi.distribution import DistributionScore
    sc = DistributionScore((1,) + shape[1:], bins=B, joint=0, value_range=(286.5, 293.75), device=d)
    m = sc.measure(T(src[:1]), T(truth[:1]))
    fh = QuantileMap.from_histograms(m["hist_pred"], m["hist_truth"], (286.5, 293.75), device=d)
    direct = QuantileMap(1, (286.5, 293.75), bins=B, on="value", device=d)
    direct.accumulate(T(src[:1]), T(truth[:1]))
    direct.fit()
    assert fh.fitted and torch.equal(fh.hist, direct.hist) and torch.equal(bits(fh.table), bits(direct.table))


def test_accumulate_fit_apply_is_capturable_on_one_stream():
    d = dev()
    shape, B = SHAPES[3], 256
    src, truth, base, rg = inputs("white", shape, True)
    s_, t_, b_ = T(src), T(truth), T(base)
    eager = QuantileMap(shape[0], rg, bins=B, device=d)
    eager.accumulate(s_, t_, b_)
    eager.fit()
    want = eager.apply(s_, b_).clone()
    qm = QuantileMap(shape[0], rg, bins=B, device=d)
    qm.accumulate(s_, t_, b_)  # warm-up outside capture: the buffers exist
    qm.fit()
    qm.apply(s_, b_)
    qm.reset()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(device=d)
    s.wait_stream(torch.cuda.current_stream(d))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            qm.accumulate(s_, t_, b_)
            qm.fit()
            out = qm.apply(s_, b_)
    torch.cuda.current_stream(d).wait_stream(s)
    for _ in range(2):
        for k in ("hist", "count", "knots", "table", "meta", "out"):
            getattr(qm, k).fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        for k in ("hist", "count", "knots", "table", "meta"):
            assert torch.equal(bits(getattr(qm, k)), bits(getattr(eager, k))), k
        assert torch.equal(bits(out), bits(want))


# -------------------------------------------------------------------- 6. end to end
LR_SHAPE, HR_SHAPE = (1, 40, 56), (1, 160, 224)


@functools.lru_cache(maxsize=None)
def regions(land):
    """three HR regions (numpy): two to fit on, one to map"""
    rng = np.random.RandomState(91)
    out = []
    for _ in range(3):
        hr = _field(rng, 1, 160, 224) * 2 + 5
        if land:
            hr[0, 40:72, 100:140] = np.nan  # land on whole LR pixels
        hr.setflags(write=False)
        out.append(hr)
    return tuple(out)


def make(land=False, **kw):
    d = dev()
    spec, _, flat = _small_rcan()
    return RegionSuperResolver(spec, flat.to(d), LR_SHAPE, tile_lr=TILE, overlap=(4, 4), land=land, device=d, **kw)


@pytest.mark.parametrize("on,land,ensemble", [("detail", False, 1), ("value", False, 1), ("detail", True, 1),
                                              ("value", True, 1), ("detail", False, 4)],
                         ids=["detail", "value", "detail-land", "value-land", "detail-ensemble4"])
def test_the_resolvers_model_is_the_map_of_the_plain_resolvers(on, land, ensemble):
    hrs = [T(h) for h in regions(land)]
    plain = make(land, ensemble=ensemble)
    qm = plain.fit_quantile_map(hrs[:2], bins=64, on=on)
    assert qm.on == on and qm.fitted and int(qm.count[0]) > 2 * 160 * 224 * (0.9 if land else 1) - 1
    rs = make(land, ensemble=ensemble, quantile_map=qm)
    im0 = {k: v.clone() for k, v in plain.score(hrs[2])[0].items()}
    im = rs.score(hrs[2])[0]
    want = qm.apply(im0["model"], im0["interpolated"] if on == "detail" else None)
    wrong = int((bits(im["model"]) != bits(want)).sum())
    print(f"{on} land {land} ensemble {ensemble}: elements that differ {wrong}; moved "
          f"{float((want - im0['model']).abs().nan_to_num().max()):.3g}")
    assert wrong == 0 and not torch.equal(bits(want), bits(im0["model"]))
    for k in im0:
        if k != "model":
            assert torch.equal(bits(im[k]), bits(im0[k])), k
    assert torch.equal(torch.isnan(im["model"]), torch.isnan(im0["model"]))
    assert bool(torch.isnan(im["model"]).any()) == land
    # half strength is the oracle's half correction of the same fields, bit for bit
    half = make(land, ensemble=ensemble, quantile_map=qm, qm_strength=0.5).score(hrs[2])[0]["model"]
    o = qo.apply(im0["model"].cpu().numpy(), im0["interpolated"].cpu().numpy() if on == "detail" else None,
                 qm.table.cpu().numpy(), qm.meta.cpu().numpy(), 64, 0.5)
    assert np.array_equal(half.cpu().numpy().view(np.int32), o.view(np.int32))


def test_the_replayed_graph_is_the_eager_run_and_reads_a_refitted_map():
    hrs = [T(h) for h in regions(False)]
    plain = make()
    qm = plain.fit_quantile_map(hrs[:1], bins=64)
    eager = make(quantile_map=qm)
    rg = make(quantile_map=qm, graph=True)
    lr = plain.score(hrs[2])[0]["input"].clone()
    want = eager.super_resolve(lr)["model"].clone()
    for _ in range(2):
        assert torch.equal(bits(rg.super_resolve(lr)["model"]), bits(want))
    # refit the SAME object on another region: the next replay maps through the new table
    im = plain.score(hrs[1])[0]
    qm.reset()
    qm.accumulate(im["model"], hrs[1], im["interpolated"])
    qm.fit()
    want2 = eager.super_resolve(lr)["model"].clone()
    assert not torch.equal(bits(want2), bits(want))
    assert torch.equal(bits(rg.super_resolve(lr)["model"]), bits(want2))


def test_consistency_runs_after_the_map():
    """'residual_left' with the map is no larger than 10 x that of the same resolver without:
    the correction runs after the map (were it before, the map's displacement, orders above
    E^K r0, would be left in it).  The factor only guards the order of the two steps."""
    hrs = [T(h) for h in regions(False)]
    plain = make(consistent=3)
    qm = plain.fit_quantile_map(hrs[:2], bins=64)
    off = float(plain.score(hrs[2])[0]["residual_left"].abs().max())
    im = make(consistent=3, quantile_map=qm).score(hrs[2])[0]
    on_ = float(im["residual_left"].abs().max())
    # what the coarse scale would be left with were the map applied last
    last = make(quantile_map=qm).score(hrs[2])[0]
    from srmi.engine import downsample
    moved = float((last["input"] - downsample(last["model"][None], 4, mode=plain.dmode)[0]).abs().max())
    print(f"residual_left max: map off {off:.3g}, map on {on_:.3g} (x {on_ / off:.2f}); mapped and uncorrected {moved:.3g}")
    assert on_ <= 10 * off
    # the map was fitted on the blended field before the correction: the same tables as consistent=0
    qm0 = make().fit_quantile_map(hrs[:2], bins=64)
    assert torch.equal(qm0.hist, qm.hist) and torch.equal(bits(qm0.table), bits(qm.table))


def test_no_map_is_the_object_as_it_was():
    hr = T(regions(False)[2])
    a = make(quantile_map=None, qm_strength=0.3).score(hr)
    b = make().score(hr)
    assert sorted(a[0]) == sorted(b[0]) == ["input", "interpolated", "model"]
    for k in b[0]:
        assert torch.equal(bits(a[0][k]), bits(b[0][k])), k
    for k in b[1]:
        assert torch.equal(bits(a[1][k]), bits(b[1][k])), k


@pytest.mark.parametrize("on", ["detail", "value"])
def test_fit_quantile_map_is_a_manual_accumulate_over_the_same_images(on):
    hrs = [T(h) for h in regions(False)]
    plain = make()
    qm = plain.fit_quantile_map(hrs[:2], bins=32, on=on, tail_count=8)
    manual = QuantileMap(1, qm.range, bins=32, on=on, tail_count=8, device=dev())
    for hr in hrs[:2]:
        im = plain.score(hr)[0]
        manual.accumulate(im["model"], hr, im["interpolated"] if on == "detail" else None)
    manual.fit()
    for k in ("hist", "count", "knots", "table", "meta"):
        assert torch.equal(bits(getattr(qm, k)), bits(getattr(manual, k))), k
    # the default range: the first region's truth (or truth detail), min and max
    im = plain.score(hrs[0])[0]
    t = hrs[0] - im["interpolated"] if on == "detail" else hrs[0]
    assert qm.range[0, 0] == float(t.min()) and qm.range[0, 1] == float(t.max())
    given = plain.fit_quantile_map(hrs[:1], bins=32, on=on, value_range=(-50.0, 50.0))
    assert given.range.tolist() == [[-50.0, 50.0]] and int(given.hist[0, :, 0].sum()) == 0


def test_the_resolver_refuses_a_map_that_does_not_fit():
    d = dev()
    fit1 = QuantileMap(1, (0.0, 1.0), bins=16, device=d)
    with pytest.raises(ValueError):
        make(quantile_map=fit1)  # no table yet
    fit1.fit()
    make(quantile_map=fit1)
    two = QuantileMap(2, (0.0, 1.0), bins=16, device=d)
    two.fit()
    with pytest.raises(ValueError):
        make(quantile_map=two)  # channels
    cpu = QuantileMap(1, (0.0, 1.0), bins=16, device="cpu")
    cpu.fitted = True
    with pytest.raises(ValueError):
        make(quantile_map=cpu)  # device
    for s in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError):
            make(quantile_map=fit1, qm_strength=s)
    # a state of the other mode loaded into a map a resolver already holds: the eager run refuses
    rs = make(quantile_map=fit1)
    sd = fit1.state_dict()
    sd["on"] = "value"
    fit1.load_state_dict(sd)
    with pytest.raises(ValueError):
        rs.super_resolve(torch.zeros(LR_SHAPE, device=d))
    with pytest.raises(ValueError):
        make().fit_quantile_map([])
    with pytest.raises(ValueError):
        make().fit_quantile_map([torch.zeros(HR_SHAPE, device=d)], on="both")
