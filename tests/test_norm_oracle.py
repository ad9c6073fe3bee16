"""Host-side checks of the task.norm layer (srmi.norm): the numpy restatement of the
reference's statistics and six norm branches (tests/norm_oracle.py) on cases that
can be worked out by hand, the mode names, the argument checks that must come
before any device work, the statistics file round trip, and the C ABI bindings."""
import os
import re

import numpy as np
import pytest
import torch

import norm_oracle as no
from conftest import GOLDEN, ROOT

NEW_SYMBOLS = ("srmi_tile_stats", "srmi_tile_stats_finalize", "srmi_batch_prep_norm", "srmi_region_to_tiles_norm")


def _slices():
    # 2 time slices of 2 tiles x 1 variable, 2 x 2 pixels
    a = np.array([[[[1.0, 3.0], [5.0, 7.0]]], [[[-4.0, -2.0], [-2.0, -4.0]]]])
    b = np.array([[[[2.0, 2.0], [2.0, 2.0]]], [[[-1.0, -3.0], [-5.0, -7.0]]]])
    return [a, b]


def test_oracle_tile_and_global_statistics_by_hand():
    t = no.compute_normalization(_slices())
    assert t.shape == (2, 1, 4)
    # tile 0: means 4, 2 -> 3; variances 5, 0 -> 2.5; max 7; min 1
    np.testing.assert_array_equal(t[0, 0], [3.0, 2.5, 7.0, 1.0])
    # tile 1 is negative throughout: means -3, -4; variances 1, 5; max -1 (not 0); min -7
    np.testing.assert_array_equal(t[1, 0], [-3.5, 3.0, -1.0, -7.0])
    g = no.globalize_norm(t)
    np.testing.assert_array_equal(g, [[-0.25, 2.75, 7.0, -7.0]])


def test_oracle_statistics_match_reference_golden():
    """tests/golden/norm.npz holds what the reference's own NormData and globalize_norm
    made of three fp32 time slices (make_golden_norm.py).  The restatement does the same
    numpy operations on the same dtype, so it reproduces them exactly; in fp64 it
    agrees to fp32 accuracy."""
    g = np.load(os.path.join(GOLDEN, "norm.npz"))
    assert list(g["stats"]) == no.STATS
    slices = [g[f"slice{i}"] for i in range(3)]
    t32 = no.compute_normalization(slices)
    np.testing.assert_array_equal(t32, g["tstats"])
    np.testing.assert_array_equal(no.globalize_norm(g["tstats"]), g["gstats"])
    t64 = no.compute_normalization([s.astype(np.float64) for s in slices])
    np.testing.assert_allclose(t64, g["tstats"], rtol=2e-6, atol=2e-6)
    assert g["tstats"][1, 0, 1] == 0.0 and g["tstats"][2, 1, 2] < 0.0  # constant plane; negative max


def test_oracle_norm_branches_by_hand():
    sl = _slices()
    t = no.compute_normalization(sl)
    x = sl[0]
    out, at = no.norm(x, "lnorm")
    np.testing.assert_allclose(out[0, 0], (x[0, 0] - 4.0) / np.sqrt(5.0))
    assert sorted(at) == ["mean", "std"] and at["mean"].shape == (2, 1, 1, 1)
    out, at = no.norm(x, "lscale")
    np.testing.assert_array_equal(out[0, 0], [[0.0, 1 / 3], [2 / 3, 1.0]])
    np.testing.assert_array_equal(at["max"][:, 0, 0, 0], [7.0, -2.0])
    np.testing.assert_array_equal(at["min"][:, 0, 0, 0], [1.0, -4.0])
    out, at = no.norm(x, "gnorm", tstats=t)
    np.testing.assert_allclose(out, (x + 0.25) / np.sqrt(2.75))
    assert at == {}
    out, at = no.norm(x, "gscale", tstats=t)
    np.testing.assert_allclose(out, (x + 7.0) / 14.0)
    assert at == {}
    # the batch is tile 1 alone: its statistics are row 1, selected by tile_range
    out, at = no.norm(x[1:], "tnorm", (1, 2), t)
    np.testing.assert_allclose(out[0, 0], (x[1, 0] + 3.5) / np.sqrt(3.0))
    np.testing.assert_array_equal(at["mean"].ravel(), [-3.5])
    out, at = no.norm(x[1:], "tscale", (1, 2), t)
    np.testing.assert_allclose(out[0, 0], (x[1, 0] + 7.0) / 6.0)
    np.testing.assert_array_equal([at["max"].ravel(), at["min"].ravel()], [[-1.0], [-7.0]])
    with pytest.raises(Exception, match="Unknown norm: znorm"):
        no.norm(x, "znorm")
    # denorm undoes both kinds
    for m in ("lnorm", "lscale"):
        out, at = no.norm(x, m)
        np.testing.assert_allclose(no.denorm(out, at), x, rtol=1e-15, atol=1e-15)


def test_norm_type_names():
    from srmi.config import Section
    from srmi.norm import ATTR_KEYS, NORM_TYPES, norm_type
    assert NORM_TYPES == ("lnorm", "lscale", "gnorm", "gscale", "tnorm", "tscale")
    for n in NORM_TYPES:
        assert norm_type(Section(norm=n)) == n
    assert norm_type(None) == "lnorm" and norm_type(Section()) == "lnorm"
    with pytest.raises(Exception, match="Unknown norm: znorm"):
        norm_type(Section(norm="znorm"))
    assert {k: set(v) for k, v in ATTR_KEYS.items()} == {
        "lnorm": {"mean", "std"}, "tnorm": {"mean", "std"}, "lscale": {"max", "min"}, "tscale": {"max", "min"},
        "gnorm": set(), "gscale": set()}


def test_tnorm_task_file():
    from srmi.config import load_group
    from srmi.norm import norm_type
    assert norm_type(load_group("task", "swot-tnorm")) == "tnorm"


def test_dataset_norm_without_stats_raises_before_device_work():
    from srmi.batch import prep_batch
    from srmi.norm import normalize_tiles
    raw = torch.zeros(2, 1, 8, 8)  # a host tensor: nothing may be launched on it
    for m in ("gnorm", "gscale", "tnorm", "tscale"):
        with pytest.raises(ValueError, match="stats"):
            prep_batch(raw, norm=m)
        with pytest.raises(ValueError, match="stats"):
            normalize_tiles(raw, m)
    with pytest.raises(Exception, match="Unknown norm: znorm"):
        prep_batch(raw, norm="znorm")


def test_normstats_save_load_round_trip(tmp_path):
    from srmi.norm import STATS, NormStats
    assert list(STATS) == no.STATS
    rng = np.random.RandomState(0)
    st = NormStats()
    st.tiles = torch.tensor(rng.randn(7, 2, 4).astype(np.float32))
    p = st.save(str(tmp_path / "norms.nc"), ["SST", "SSS"])
    back = NormStats.load(p)
    assert torch.equal(back.tiles, st.tiles)
    swapped = NormStats.load(p, varnames=["SSS", "SST"])
    assert torch.equal(swapped.tiles, st.tiles[:, [1, 0]])
    np.testing.assert_allclose(back.globals.numpy(), no.globalize_norm(st.tiles.double().numpy()), rtol=1e-7)
    from scipy.io import netcdf_file
    with netcdf_file(p, "r", mmap=False) as f:
        assert f.variables["SST"].dimensions == ("tiles", "stat")
        assert [b"".join(r.tolist()).decode().rstrip("\0") for r in f.variables["stat"][:]] == no.STATS
    # the offsets of the dataset modes, from the stored rows
    t = st.tiles.abs()  # variances must be >= 0 for the sqrt
    st2 = NormStats()
    st2.tiles, st2.globals = t, torch.tensor(no.globalize_norm(t.double().numpy()).astype(np.float32))
    off, div = st2.offsets("tnorm", (2, 5))
    assert torch.equal(off, t[2:5, :, 0]) and torch.equal(div, torch.sqrt(t[2:5, :, 1]))
    off, div = st2.offsets("tscale", (2, 5))
    assert torch.equal(off, t[2:5, :, 3]) and torch.equal(div, t[2:5, :, 2] - t[2:5, :, 3])
    off, div = st2.offsets("gscale", (0, 3))
    assert off.shape == (3, 2) and torch.equal(off[1], st2.globals[:, 3])
    g = st2.for_grid(np.array([2, -1, 0]))
    assert torch.equal(g.tiles[0], t[2]) and torch.equal(g.tiles[2], t[0]) and bool(torch.isnan(g.tiles[1]).all())


def test_new_header_symbols_are_bound():
    from srmi import _lib
    hdr = open(os.path.join(ROOT, "include", "srmi.h")).read()
    protos = set(re.findall(r"\b(srmi_[a-z0-9_]+)\s*\(", hdr))
    for n in NEW_SYMBOLS:
        assert n in protos, f"{n} not declared in srmi.h"
        assert n in _lib.EXPORTED, f"{n} not bound in _lib"
    defs = dict((k, int(v)) for k, v in re.findall(r"#define (SRMI_NORM_[A-Z]+) (\d+)", hdr))
    assert defs == {"SRMI_NORM_LNORM": 0, "SRMI_NORM_LSCALE": 1, "SRMI_NORM_AFFINE": 2}
    for k, v in defs.items():
        assert getattr(_lib, k) == v
