"""The fractions skill score's oracle (tests/fss_oracle.py) against the identities of its
definition (include/srmi.h, "the fractions skill score"), scipy's uniform filter and fields
whose displacement is known; the argument checks, the netCDF round trip and the bindings; no
GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import fss_oracle as fo
from test_gradient_oracle import smooth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("srmi_fss_workspace", "srmi_fss")
LADDER = (1, 3, 5, 9, 17, 33, 79)


def white(shape, seed):
    rng = np.random.default_rng(seed)
    t = rng.standard_normal(shape).astype(np.float32)
    p = (t + 0.7 * rng.standard_normal(shape)).astype(np.float32)
    return p, t


def test_n1_is_the_contingency_table_of_the_same_event():
    p, t = white((2, 23, 31), 1)
    thr = np.array([[0.0, 1.0, 2.5], [-0.5, 0.3, 9.0]], dtype=np.float32)
    r = fo.fss(p, t, thr, (1, 5))
    hits, misses, fa = fo.contingency(p, t, thr)
    assert (hits + misses > 0)[:, :2].all() and (fa > 0)[:, :2].all()
    assert np.array_equal(r["num"][:, :, 0], misses + fa)
    assert np.array_equal(r["den"][:, :, 0], 2 * hits + misses + fa)
    assert np.array_equal(r["events_pred"], hits + fa) and np.array_equal(r["events_truth"], hits + misses)
    assert r["num"].dtype == np.int64 and r["den"].dtype == np.int64
    # no event in either field: den == 0 and fss is NaN, the frequencies are 0
    assert r["den"][1, 2, 0] == 0 and np.isnan(r["fss"][1, 2]).all() and r["f_truth"][1, 2] == 0
    assert np.isnan(r["skilful_scale"][1, 2]) and np.isnan(r["afss"][1, 2])


def test_a_window_that_covers_the_plane_gives_afss():
    p, t = white((2, 9, 14), 2)
    thr = np.array([0.2, 1.0], dtype=np.float32)
    r = fo.fss(p, t, thr, (3, 27, 29))  # 27 = 2 max(H, W) - 1
    H, W = 9, 14
    ep, et = r["events_pred"], r["events_truth"]
    for k in (1, 2):
        assert np.array_equal(r["num"][:, :, k], H * W * (ep - et) ** 2)
        assert np.array_equal(r["den"][:, :, k], H * W * (ep ** 2 + et ** 2))
        np.testing.assert_allclose(r["fss"][:, :, k], r["afss"], rtol=1e-13)
    assert not np.array_equal(r["num"][:, :, 0], r["num"][:, :, 1])


def test_equal_fields_score_one_at_every_scale_with_an_event():
    _, t = white((1, 17, 20), 3)
    r = fo.fss(t.copy(), t, [0.5, 100.0], LADDER)
    assert (r["num"] == 0).all() and (r["fss"][0, 0] == 1).all() and np.isnan(r["fss"][0, 1]).all()
    assert r["skilful_scale"][0, 0] == 1 and r["bias"][0, 0] == 1 and r["afss"][0, 0] == 1


def test_window_counts_are_scipys_uniform_filter():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(4)
    ind = rng.random((21, 34)) < 0.3
    for n in (1, 3, 9, 33, 41, 67, 255):
        ref = ndi.uniform_filter(ind.astype(np.float64), n, mode="constant") * n * n
        got = fo.window_counts(ind, n)
        assert got.dtype == np.int64
        assert np.abs(got - ref).max() <= 1e-14 * n * n * 21 * 34, n
    p, t = white((1, 21, 34), 5)
    r = fo.fss(p, t, [0.4], (5, 9))
    _, ip, it = fo.events(p, t, [0.4])
    for k, n in enumerate((5, 9)):  # the textbook form, with the fractions
        fp = ndi.uniform_filter(ip[0, 0].astype(np.float64), n, mode="constant")
        ft = ndi.uniform_filter(it[0, 0].astype(np.float64), n, mode="constant")
        ref = 1.0 - ((fp - ft) ** 2).sum() / ((fp ** 2).sum() + (ft ** 2).sum())
        assert abs(r["fss"][0, 0, k] - ref) <= 1e-12


@pytest.mark.parametrize("d,skilful", [(0, 1), (2, 3), (5, 9)])
def test_a_displaced_field_is_skilful_from_the_displacement_on(d, skilful):
    """A field rolled by d columns: the point-wise table pays twice, FSS rises with n and the
    skilful scale follows the displacement."""
    _, t = smooth((1, 40, 37), 3, noise=0)
    p = np.roll(t, d, axis=-1)
    thr = np.array([[np.quantile(t, 0.9)]], dtype=np.float32)
    r = fo.fss(p, t, thr, LADDER)
    f = r["fss"][0, 0]
    print(f"d = {d}: fss {f}, target {r['target'][0, 0]:.4f}, skilful {r['skilful_scale'][0, 0]}")
    if d == 0:
        assert (f == 1).all()
    else:
        assert (np.diff(f) > 0).all() and f[0] < r["target"][0, 0]
    assert r["skilful_scale"][0, 0] == skilful


def test_nan_and_inf_are_the_mask_in_both_fields():
    p, t = white((2, 12, 15), 6)
    p[0, 3, 4] = np.nan
    t[0, 7, 7] = np.inf      # above every threshold, and yet no event
    t[1, 0, 0] = -np.inf
    p[1, 11, 14] = np.inf
    thr = [0.0, 0.8]
    r = fo.fss(p, t, thr, (1, 3, 7))
    assert np.array_equal(r["used"], [12 * 15 - 2, 12 * 15 - 2])
    # the same as fields in which the pixels that are not used are below every threshold in both
    bad = ~(np.isfinite(p) & np.isfinite(t))
    p2, t2 = p.copy(), t.copy()
    p2[bad] = -1e30
    t2[bad] = -1e30
    r2 = fo.fss(p2, t2, thr, (1, 3, 7))
    for k in ("num", "den", "events_pred", "events_truth"):
        assert np.array_equal(r[k], r2[k]), k
    assert not np.array_equal(r["f_truth"], r2["f_truth"])  # the frequencies are over the used pixels
    # a NaN threshold: no event
    r3 = fo.fss(p, t, [np.nan], (1, 3))
    assert (r3["den"] == 0).all() and (r3["events_truth"] == 0).all() and np.isnan(r3["fss"]).all()


def test_a_channel_without_a_used_pixel_is_nan_with_zero_tables():
    p, t = white((2, 8, 9), 7)
    t[1] = np.nan
    r = fo.fss(p, t, [0.0, 1.0], (1, 3, 5))
    assert r["used"][1] == 0 and (r["num"][1] == 0).all() and (r["den"][1] == 0).all()
    assert (r["events_pred"][1] == 0).all()
    for k in ("fss",) + fo.DERIVED:
        assert np.isnan(r[k][1]).all() and np.isfinite(r[k][0]).all(), k


def test_argument_checks():
    from srmi.fss import FractionsSkillScore, check_scales
    assert check_scales((1, 3, 255)) == (1, 3, 255) and check_scales([5]) == (5,)
    for s in ((), (2,), (1, 4), (3, 3), (5, 3), (0,), (-1,), (257,), (1.0, 3), (True, 3), tuple(range(1, 35, 2)), 3,
              ("3",)):
        with pytest.raises(ValueError, match="scales"):
            check_scales(s)
    # the constructor refuses before it touches a device
    for shape, thr, sc in (((2, 8, 8), [0.0] * 9, (1, 3)), ((2, 8, 8), [], (1, 3)), ((2, 8, 8), np.zeros((3, 2)), (1,)),
                           ((2, 8, 8), "x", (1,)), ((0, 8, 8), [0.0], (1,)), ((1, 0, 8), [0.0], (1,)),
                           ((1, 8, -1), [0.0], (1,)), ((1, 1 << 16, 1 << 15), [0.0], (1,)), ((1, 8, 8), [0.0], (1, 2)),
                           ((1, 46340, 46340), [0.0], (1, 255))):  # H W n^4 > 2^62
        with pytest.raises(ValueError):
            FractionsSkillScore(shape, thr, sc, device="cuda:0")
    lib = __import__("srmi._lib", fromlist=["load"]).load()
    n = C.c_size_t(0)
    E = -10001
    for bad in ((1, 8, 8, 0, 1), (1, 8, 8, 9, 1), (1, 8, 8, 1, 0), (1, 8, 8, 1, 17), (0, 8, 8, 1, 1), (1, 0, 8, 1, 1),
                (1, 8, 0, 1, 1), (1, 1 << 16, 1 << 15, 1, 1)):
        assert lib.srmi_fss_workspace(*bad, C.byref(n)) == E, bad
    assert lib.srmi_fss_workspace(1, 8, 8, 1, 1, None) == E
    assert lib.srmi_fss_workspace(2, 4096, 4096, 8, 16, C.byref(n)) == 0 and n.value > 0


def test_save_and_load_fss_round_trip(tmp_path):
    from srmi.results import load_fss, save_fss
    p, t = white((2, 12, 15), 8)
    t[1] = np.nan  # an empty channel: NaN survives
    thr = np.array([[0.0, 1.0, np.nan], [0.5, 0.6, 0.7]], dtype=np.float32)
    r = fo.fss(p, t, thr, (1, 3, 7))
    r["num"][0, 0, 2] = 94820853760000 * 40000 + 12345  # above 2^53: the tables are kept as integers
    path = save_fss(str(tmp_path / "f.nc"), r, ["SST", "SSS"], thr, (1, 3, 7))
    back, names, thr2, scales = load_fss(path)
    assert names == ["SST", "SSS"] and scales == (1, 3, 7)
    assert thr2.dtype == np.float32 and np.array_equal(thr2, thr, equal_nan=True)
    for k in ("num", "den", "events_pred", "events_truth", "used"):
        assert back[k].dtype == np.int64 and np.array_equal(back[k], r[k]), k
    for k in ("fss",) + fo.DERIVED:
        assert back[k].dtype == np.float64 and np.array_equal(back[k], r[k], equal_nan=True), k
    with pytest.raises(ValueError, match="lacks"):
        save_fss(str(tmp_path / "bad.nc"), {"num": r["num"]}, ["SST", "SSS"], thr, (1, 3, 7))
    with pytest.raises(ValueError, match="fss"):
        save_fss(str(tmp_path / "bad.nc"), dict(r, fss=r["fss"][:, :, :2]), ["SST", "SSS"], thr, (1, 3, 7))


def test_the_tile_size_python_states_is_the_librarys():
    """FSS_TILE places the GPU tests' seam cases: the workspace holds 16 bytes per (channel,
    threshold, scale) and rectangle a workgroup of the windows launch owns, so what one more
    scale costs says where one more row or column opens a new rectangle."""
    from srmi import _lib
    from srmi.fss import FSS_TILE
    lib = _lib.load()
    th, tw = FSS_TILE

    def tiles(H, W, Cn=1, T=1):
        a, b = C.c_size_t(0), C.c_size_t(0)
        assert lib.srmi_fss_workspace(Cn, H, W, T, 1, C.byref(a)) == 0
        assert lib.srmi_fss_workspace(Cn, H, W, T, 2, C.byref(b)) == 0
        assert a.value % 16 == 0 and (b.value - a.value) % (16 * Cn * T) == 0
        return (b.value - a.value) // (16 * Cn * T)
    assert tiles(1, 1) == 1 and tiles(th, tw) == 1 and tiles(th + 1, tw) == 2 and tiles(th, tw + 1) == 2
    assert tiles(2 * th, 3 * tw) == 6 and tiles(2 * th + 1, 3 * tw + 1, Cn=2, T=3) == 12


def test_symbols_are_declared_and_bound():
    from srmi import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "srmi.h")).read()
    for name in SYMBOLS:
        assert name in _lib.EXPORTED and hasattr(lib, name) and f"int {name}(" in header
    import srmi.fss as sf
    for name in ("FractionsSkillScore", "check_scales", "FSS_TILE"):
        assert hasattr(sf, name)
    from srmi import results
    from srmi.superres import RegionSuperResolver
    assert hasattr(RegionSuperResolver, "score_fss") and hasattr(results, "save_fss") and hasattr(results, "load_fss")
