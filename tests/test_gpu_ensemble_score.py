"""The ensemble score on the HIP path (srmi_ensemble_score, srmi.ensemble_score.EnsembleScore)
against its numpy oracle (tests/ensemble_score_oracle.py).

Bars, derived, not measured.  The integer tables and the CRPS map (NaN positions included) are
exact: the per-pixel arithmetic is fp64 with every operation rounded once in a stated order,
which numpy's float64 elementwise operations reproduce.  A device sum adds T non-negative
terms, the oracle's bits, in some fixed order: it is within T * 2^-53 of their correctly rounded
sum (math.fsum), relative to the sum of the terms -- the a-priori bound of any summation
order.  The derived values equal ``derive`` applied to the device's own sums and tables, bit for
bit.

Shapes: one pixel; 37 x 53 (an odd plane: every plane but the first starts off a 16-byte
boundary, the one-by-one form, with a ragged last quad) at an odd K and at K = 8; 37 x 54 (the
planes of channel 0 are aligned, those of channel 1 are not: the 16-byte form with a ragged last
quad beside the other form); one pixel and one quad more than a workgroup's span; 300 x 517
(aligned, 38 workgroups a plane)."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ensemble_score_oracle as eo  # noqa: E402
from srmi import _lib  # noqa: E402
from srmi._lib import ptr, stream_handle  # noqa: E402
from srmi.ensemble_score import ENS_SPAN, FINISH, MAIN, EnsembleScore, ensemble_workspace  # noqa: E402
from test_gpu_ssim_loss import dev  # noqa: E402

U = 2.0 ** -53
NAN_BITS = 0x7fc00000
TABLES = ("used", "rank_hist", "tied", "bin_count")
DERIVED = eo.DERIVED + ("bin_spread", "bin_rmse")


def smooth(rng, shape):
    """A field a few pixels smooth: a box sum of white noise along both axes."""
    x = rng.standard_normal(shape)
    for ax in (-1, -2):
        if shape[ax] > 1:
            x = x + np.roll(x, 1, ax) + np.roll(x, -1, ax) + np.roll(x, 2, ax)
    return x


def fields(content, K, Cn, H, W, seed):
    rng = np.random.default_rng(seed)
    shape = (Cn, H, W)
    if content == "white":
        y = rng.standard_normal(shape)
        m = 0.6 * y[None] + 0.8 * rng.standard_normal((K,) + shape)
    elif content == "smooth":
        y = smooth(rng, shape)
        m = y[None] + 0.3 * np.stack([smooth(rng, shape) for _ in range(K)])
    elif content == "warm":  # 290 +- 1.5: the spacing of fp32 there is 3e-5
        y = 290.0 + 1.5 * rng.standard_normal(shape)
        m = y[None] + 0.4 * rng.standard_normal((K,) + shape)
    elif content == "quantised":  # halves: ties with the truth and equal members occur
        y = np.round(2 * rng.standard_normal(shape)) / 2
        m = np.round(2 * (y[None] + 0.7 * rng.standard_normal((K,) + shape))) / 2
    elif content == "identical":
        y = rng.standard_normal(shape)
        m = np.repeat((y + rng.standard_normal(shape))[None], K, 0)
    else:
        raise ValueError(content)
    return m.astype(np.float32), y.astype(np.float32)


def poke(m, y, rng, empty_channel=False):
    """NaN / +-Inf in the truth only, in one member only, and in both; the last channel all NaN."""
    n = y.size
    flat_y, flat_m = y.reshape(-1), m.reshape(m.shape[0], -1)
    bad = (np.nan, np.inf, -np.inf)
    for i, at in enumerate(rng.choice(n, size=min(n, 9), replace=False)):
        if i % 3 == 0:
            flat_y[at] = bad[i // 3]
        elif i % 3 == 1:
            flat_m[rng.integers(m.shape[0]), at] = bad[i // 3]
        else:
            flat_y[at] = bad[i // 3]
            flat_m[rng.integers(m.shape[0]), at] = bad[(i // 3 + 1) % 3]
    if empty_channel:
        y[-1] = np.nan


def spread_edges(m, B, Cn, nan_row=False):
    """B - 1 ascending edges per channel across the members' spread; nan_row: a row holding NaN."""
    if B == 1:
        return np.zeros((Cn, 0), dtype=np.float32)
    with np.errstate(invalid="ignore"):
        s = m.astype(np.float64).std(0).reshape(Cn, -1)
    s = np.where(np.isfinite(s), s, 0.0)
    ed = np.stack([np.quantile(s[c], np.linspace(0, 1, B + 1)[1:-1]) for c in range(Cn)]).astype(np.float32)
    if nan_row:
        ed[-1, ::2] = np.nan
    return ed


# name -> (K, C, H, W), content, B, poke?, empty channel?, NaN edge row?
CASES = {
    "one pixel": ((2, 1, 1, 1), "white", 1, False, False, False),
    "odd K, ragged": ((3, 2, 37, 53), "white", 16, True, False, False),
    "K8, ragged, quantised": ((8, 2, 37, 53), "quantised", 4, True, False, False),
    "K8, ragged, warm, NaN edges": ((8, 2, 37, 53), "warm", 16, False, False, True),
    "identical members": ((4, 2, 37, 53), "identical", 3, False, False, False),
    "half aligned": ((4, 2, 37, 54), "smooth", 2, True, False, False),
    "K5": ((5, 3, 16, 16), "white", 1, False, False, False),
    "K6": ((6, 2, 40, 52), "quantised", 5, True, False, False),
    "K7": ((7, 1, 33, 20), "warm", 2, False, False, False),
    "span + 1 wide": ((4, 2, 1, ENS_SPAN + 1), "smooth", 3, True, False, False),
    "span + 1 high": ((4, 1, ENS_SPAN + 1, 1), "white", 2, False, False, False),
    "span + 4": ((4, 2, 2, ENS_SPAN // 2 + 2), "white", 2, True, False, False),
    "K4, many workgroups": ((4, 2, 300, 517), "smooth", 10, True, True, False),
    "K8, many workgroups": ((8, 2, 300, 517), "white", 3, True, False, False),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(members, truth, edges, the oracle's terms / tables / term columns): made once, never changed."""
    (K, Cn, H, W), content, B, pk, empty, nan_row = CASES[name]
    seed = sorted(CASES).index(name)
    m, y = fields(content, K, Cn, H, W, seed)
    if pk:
        poke(m, y, np.random.default_rng(100 + seed), empty)
    ed = spread_edges(m, B, Cn, nan_row)
    terms = eo.pixel_terms(m, y, ed)
    for a in (m, y, ed):
        a.setflags(write=False)
    return m, y, ed, dict(terms=terms, tables=eo.tables(terms, K, B), columns=eo.sum_terms(terms, B),
                          crps_map=eo.crps_map(terms))


def measure(m, y, ed, crps_map=True, fill=None, launches=0):
    d = dev()
    es = EnsembleScore(m.shape, ed, crps_map, device=d)
    if fill is not None:
        es.workspace.fill_(fill)
    res = es.measure(torch.tensor(m, device=d), torch.tensor(y, device=d), launches)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in res.items()}


def check_against(what, got, K, o):
    """The bars of the module docstring; prints the worst sum error before it asserts."""
    for k in TABLES:
        assert got[k].dtype == np.int64 and np.array_equal(got[k], o["tables"][k]), (what, k)
    if "crps_map" in got:
        ref = o["crps_map"]
        gb, nan = got["crps_map"].view(np.int32), np.isnan(ref)
        assert np.array_equal(np.isnan(got["crps_map"]), nan), what
        assert (gb[nan] == NAN_BITS).all() and np.array_equal(gb[~nan], ref.view(np.int32)[~nan]), what
    worst = 0.0
    bad = []
    for c, cols in enumerate(o["columns"]):
        for i, col in enumerate(cols):
            dv = float(got["sums"][c, i])
            if col.size == 0:
                if dv != 0.0:
                    bad.append((c, i, dv, 0.0))
                continue
            exact, mag = math.fsum(col.tolist()), math.fsum(np.abs(col).tolist())
            err, bar = abs(dv - exact), col.size * U * mag
            if mag > 0:
                worst = max(worst, err / (U * mag))
            if not err <= bar:
                bad.append((c, i, dv, exact))
    print(f"{what}: worst sum error {worst:.2f} x 2^-53 of the sum of the terms (bar: the number of terms, up to "
          f"{int(o['tables']['used'].max())})")
    assert not bad, (what, bad)
    tabs = {k: got[k] for k in TABLES}
    ref = eo.derive(got["sums"], tabs, K)
    for k in DERIVED:
        assert got[k].dtype == np.float64 and np.array_equal(got[k], ref[k], equal_nan=True), (what, k, got[k], ref[k])
        fin = np.isfinite(ref[k])
        assert np.array_equal(got[k][fin].view(np.int64), ref[k][fin].view(np.int64)), (what, k)


# ------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("name", sorted(CASES))
def test_matches_the_oracle(name):
    m, y, ed, o = case(name)
    got = measure(m, y, ed)
    check_against(name, got, m.shape[0], o)
    assert np.array_equal(got["edges"], ed, equal_nan=True) and got["bin_count"].shape == (m.shape[1], ed.shape[1] + 1)
    (K, Cn, H, W), content, B, pk, empty, nan_row = CASES[name]
    used = o["tables"]["used"]
    if pk:
        assert (used[:Cn - 1 if empty else Cn] > 0).all() and used.sum() < Cn * H * W
    if empty:
        assert used[-1] == 0 and np.isnan(got["crps"][-1]) and not got["sums"][-1].any()
        assert np.isnan(got["crps_map"][-1]).all()
    if content == "quantised":
        assert (o["tables"]["tied"][:1] > 0).all()
    if content == "identical":
        assert not got["sums"][:, 3].any() and not got["rank_hist"][:, 1:K].any()
        assert not got["sums"][:, 4].any()  # K = 4 equal members: the tree gives the member, the variance is 0
    if nan_row:
        assert np.isnan(ed[-1]).sum() == 8 and not got["bin_count"][-1][8:].any()  # at most 7 edges can count


def test_exchangeable_draws_on_the_device():
    """The CPU test's statistics from the device's own tables and sums (seed 0)."""
    rng = np.random.default_rng(0)
    m = rng.standard_normal((8, 1, 300, 517)).astype(np.float32)
    y = rng.standard_normal((1, 300, 517)).astype(np.float32)
    got = measure(m, y, np.zeros((1, 0), dtype=np.float32), crps_map=False)
    n = got["used"][0]
    h = got["rank_hist"][0].astype(np.float64)
    chi2 = float(((h - n / 9) ** 2 / (n / 9)).sum())
    print(f"chi2 {chi2:.2f} crps_fair {got['crps_fair'][0]:.5f} ssr {got['ssr'][0]:.4f}")
    assert n == 300 * 517 and chi2 < 26.12 and abs(got["crps_fair"][0] - 1 / math.sqrt(math.pi)) < 5e-3
    assert abs(got["ssr"][0] - 1.0) < 0.01 and got["crps"][0] > got["crps_fair"][0]


# ------------------------------------------------- 2. determinism, device edges, capture, launches
def same_bits(a, b, what):
    for k in TABLES + DERIVED + ("sums",) + (("crps_map",) if "crps_map" in a and "crps_map" in b else ()):
        assert np.array_equal(a[k].view(np.int64 if a[k].dtype.itemsize == 8 else np.int32),
                              b[k].view(np.int64 if b[k].dtype.itemsize == 8 else np.int32)), (what, k)


def test_bit_identical_runs_whatever_the_workspace_held_and_without_the_map():
    for name in ("K8, ragged, quantised", "K4, many workgroups"):
        m, y, ed, _ = case(name)
        a = measure(m, y, ed)
        same_bits(a, measure(m, y, ed), name)
        same_bits(a, measure(m, y, ed, fill=0x00), name)
        same_bits(a, measure(m, y, ed, fill=0x5A), name)
        same_bits(a, measure(m, y, ed, crps_map=False), name)


def test_edges_filled_on_the_device_after_construction():
    d = dev()
    m, y, ed, o = case("K6")
    ed_d = torch.zeros(ed.shape, dtype=torch.float32, device=d)
    es = EnsembleScore(m.shape, ed_d, True, device=d)
    assert es.edges is ed_d
    md, yd = torch.tensor(m, device=d), torch.tensor(y, device=d)
    ed_d.copy_(torch.tensor(ed, device=d))  # after construction, on the device
    got = {k: v.cpu().numpy().copy() for k, v in es.measure(md, yd).items()}
    check_against("device edges", got, m.shape[0], o)
    ed2 = (ed * np.float32(1.25)).astype(np.float32)
    ed_d.mul_(1.25)  # no host read in between
    got2 = {k: v.cpu().numpy().copy() for k, v in es.measure(md, yd).items()}
    t2 = eo.pixel_terms(m, y, ed2)
    B = ed.shape[1] + 1
    check_against("device edges refilled", got2, m.shape[0],
                  dict(terms=t2, tables=eo.tables(t2, m.shape[0], B), columns=eo.sum_terms(t2, B),
                       crps_map=eo.crps_map(t2)))
    assert not np.array_equal(got["bin_count"], got2["bin_count"])


def test_the_launches_are_capturable_and_replay_on_new_inputs():
    d = dev()
    m, y, ed, o = case("half aligned")
    md, yd = torch.tensor(m, device=d), torch.tensor(y, device=d)
    es = EnsembleScore(m.shape, ed, True, device=d)
    eager = {k: v.cpu().numpy().copy() for k, v in es.measure(md, yd).items()}  # also the warm-up outside capture
    ya = yd.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(device=d)
    s.wait_stream(torch.cuda.current_stream(d))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            res = es.measure(md, ya)
    torch.cuda.current_stream(d).wait_stream(s)
    for buf in (es.counts, es.sums, es.derived, es.crps_map):
        buf.fill_(-7)
    g.replay()
    torch.cuda.synchronize()
    same_bits(eager, {k: v.cpu().numpy().copy() for k, v in res.items()}, "replay")
    y2 = np.roll(y, 3, axis=-1)
    ya.copy_(torch.tensor(y2, device=d))
    g.replay()
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy().copy() for k, v in res.items()}
    t2 = eo.pixel_terms(m, y2, ed)
    K, B = m.shape[0], ed.shape[1] + 1
    check_against("replay on a new truth", got, K,
                  dict(terms=t2, tables=eo.tables(t2, K, B), columns=eo.sum_terms(t2, B), crps_map=eo.crps_map(t2)))
    assert not np.array_equal(got["rank_hist"], o["tables"]["rank_hist"])


def test_launch_subsets_compose_to_the_full_call():
    d = dev()
    m, y, ed, _ = case("K8, many workgroups")
    full = measure(m, y, ed)
    es = EnsembleScore(m.shape, ed, True, device=d)
    md, yd = torch.tensor(m, device=d), torch.tensor(y, device=d)
    for buf in (es.counts, es.sums, es.derived, es.crps_map):
        buf.fill_(-7)
    es.measure(md, yd, MAIN)
    torch.cuda.synchronize()
    assert (es.counts == -7).all() and (es.derived == -7).all()  # the main launch writes partials and the map only
    assert np.array_equal(es.crps_map.cpu().numpy().view(np.int32), full["crps_map"].view(np.int32))
    es.crps_map.fill_(-7)
    res = es.measure(md, yd, FINISH)
    torch.cuda.synchronize()
    assert (es.crps_map == -7).all()
    got = {k: v.cpu().numpy().copy() for k, v in res.items()}
    del got["crps_map"]
    same_bits(full, got, "main, then finish")
    same_bits(full, measure(m, y, ed, launches=MAIN | FINISH), "both bits")


# ------------------------------------------------------------- 3. canaries and refusals
def test_canaries_behind_every_output_and_the_workspace_and_refusals_launch_nothing():
    d = dev()
    lib = _lib.load()
    canary = 8
    for name in ("odd K, ragged", "span + 1 wide", "K4, many workgroups"):
        m, y, ed, o = case(name)
        K, Cn, H, W = m.shape
        B = ed.shape[1] + 1
        nbytes = ensemble_workspace(K, Cn, H, W, B)
        ws = torch.full((nbytes + 8 * canary,), 0x5A, dtype=torch.uint8, device=d)
        sizes = {"counts": Cn * (K + 3 + B), "sums": Cn * (9 + 2 * B), "derived": Cn * (9 + 2 * B), "map": Cn * H * W}
        dt = {"counts": torch.int64, "sums": torch.float64, "derived": torch.float64, "map": torch.float32}
        bufs = {k: torch.full((sizes[k] + canary,), -7, dtype=dt[k], device=d) for k in sizes}
        md, yd, ed_d = torch.tensor(m, device=d), torch.tensor(y, device=d), torch.tensor(ed, device=d)

        def run(**change):
            a = dict(members=ptr(md), truth=ptr(yd), K=K, C=Cn, H=H, W=W, edges=ptr(ed_d), B=B, ws=ptr(ws), nbytes=nbytes,
                     counts=ptr(bufs["counts"]), sums=ptr(bufs["sums"]), derived=ptr(bufs["derived"]),
                     map=ptr(bufs["map"]), launches=0)
            a.update(change)
            rc = lib.srmi_ensemble_score(*a.values(), stream_handle())
            torch.cuda.synchronize()
            return rc
        for kw in (dict(members=None), dict(truth=None), dict(edges=None), dict(ws=None), dict(counts=None),
                   dict(sums=None), dict(derived=None), dict(K=1), dict(K=9), dict(B=0), dict(B=17), dict(C=0), dict(H=0),
                   dict(W=-1), dict(nbytes=nbytes - 1), dict(ws=ptr(ws) + 8), dict(launches=4)):
            assert run(**kw) == _lib.SRMI_ERR_ARG, (name, kw)
        assert run(H=1 << 16, W=1 << 15) == _lib.SRMI_ERR_SHAPE
        for k, b in bufs.items():
            assert (b == -7).all(), (name, k)  # nothing was written
        assert (ws == 0x5A).all()
        assert run() == 0
        for k, b in bufs.items():
            assert (b[sizes[k]:] == -7).all(), (name, k)
        assert (ws[nbytes:] == 0x5A).all(), name
        counts = bufs["counts"][:sizes["counts"]].cpu().numpy().reshape(Cn, -1)
        assert np.array_equal(counts[:, 0], o["tables"]["used"]) and np.array_equal(counts[:, K + 3:], o["tables"]["bin_count"])
        got_map = bufs["map"][:sizes["map"]].cpu().numpy().reshape(Cn, H, W)
        assert np.array_equal(got_map, o["crps_map"], equal_nan=True)
    with pytest.raises(ValueError, match="members"):
        EnsembleScore((4, 2, 8, 8), [], device=d).measure(torch.zeros((3, 2, 8, 8), device=d), torch.zeros((2, 8, 8), device=d))
    with pytest.raises(ValueError, match="truth"):
        EnsembleScore((4, 2, 8, 8), [], device=d).measure(torch.zeros((4, 2, 8, 8), device=d),
                                                          torch.zeros((2, 8, 8), device=d, dtype=torch.float64))
