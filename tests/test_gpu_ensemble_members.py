"""RegionSuperResolver(members=True) and score_ensemble on the HIP path: the member fields are
the ensemble blend's K = 1 case bit for bit, their pairwise fp32 mean and spread are 'model' and
'spread' bit for bit, members=False is the resolver as it was, and score_ensemble is ``score``
plus EnsembleScore.measure of 'members'.  The small end-to-end fixture is
tests/test_gpu_ensemble.py's."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ensemble_score_oracle as eo  # noqa: E402
from srmi.distribution import DistributionScore  # noqa: E402
from srmi.ensemble_score import EnsembleScore  # noqa: E402
from test_gpu_ensemble import e2e, ensemble_dev, make  # noqa: E402
from test_gpu_overlap import bits, dev  # noqa: E402

TABLES = ("used", "rank_hist", "tied", "bin_count")
DERIVED = eo.DERIVED + ("bin_spread", "bin_rmse")


def mean_and_spread(members):
    """srmi_tiles_blend_ensemble's mean and spread as srmi.h states them, in numpy's fp32 with
    every operation rounded once: the pairwise sums in ascending j, one division by (float)K
    each, one square root."""
    m = members.cpu().numpy()
    K = np.float32(m.shape[0])
    with np.errstate(invalid="ignore"):
        mean = eo.tree(list(m)) / K
        d = [x - mean for x in m]
        return mean, np.sqrt(eo.tree([x * x for x in d]) / K)


def land_region(e):
    lr = e["lr"].clone()
    lr[0, 30:38, 40:48] = float("nan")
    lr[0, :, 80] = float("nan")
    return lr


@pytest.mark.parametrize("kw", [dict(ensemble=4), dict(ensemble=8), dict(ensemble=(0, 3, 5)),
                                dict(ensemble=8, land=True, min_wet=0.25)],
                         ids=["K4", "K8", "chosen", "land"])
def test_members_are_the_single_slab_blends_and_close_on_model_and_spread(kw):
    e = e2e()
    lr = land_region(e) if kw.get("land") else e["lr"]
    rs = make(e, members=True, **kw)
    im = {k: v.clone() for k, v in rs.super_resolve(lr).items()}
    K = rs.K
    assert tuple(im["members"].shape) == (K, 1, 288, 352) and im["members"].dtype == torch.float32
    s = rs.s
    for j, f in enumerate(rs.variants):
        one, _ = ensemble_dev(rs.sr[j], 1 << f, rs.off, rs.div, rs.bad, 1, rs.ty * s, rs.tx * s, rs.sy * s, rs.sx * s,
                              288, 352, rs.region if rs.land else None, s)
        assert torch.equal(bits(im["members"][j]), bits(one)), (kw, j)
    nan = torch.isnan(im["model"])
    assert bool(nan.any()) == bool(kw.get("land"))
    ok = ~nan
    okn = ok.cpu().numpy()
    mean, spread = mean_and_spread(im["members"])
    assert np.array_equal(np.isnan(mean), ~okn) and np.array_equal(np.isnan(spread), ~okn)
    assert np.array_equal(mean.view(np.int32)[okn], bits(im["model"]).cpu().numpy()[okn]), kw
    assert np.array_equal(spread.view(np.int32)[okn], bits(im["spread"]).cpu().numpy()[okn]), kw
    # the members disagree (the network is not equivariant), and member 0 is the plain resolver's field
    assert float(im["spread"][ok].max()) > 0
    plain = make(e, **{k: v for k, v in kw.items() if k != "ensemble"}).super_resolve(lr)["model"]
    assert torch.equal(bits(plain), bits(im["members"][0]))
    # the same bits without members, and from a captured graph
    off = make(e, **kw).super_resolve(lr)
    assert "members" not in off
    for k in off:
        assert torch.equal(bits(off[k]), bits(im[k])), (kw, k)
    rg = make(e, members=True, graph=True, **kw)
    for _ in range(2):  # the capture's warm-up, then a replay
        g = rg.super_resolve(lr)
        assert sorted(g) == sorted(im)
        for k in im:
            assert torch.equal(bits(g[k]), bits(im[k])), (kw, k)


def test_members_false_is_the_object_as_it_was_and_one_variant_has_no_members():
    e = e2e()
    a = make(e, ensemble=8, members=False)
    im = a.super_resolve(e["lr"])
    assert sorted(im) == sorted(e["images"]) == ["input", "interpolated", "model", "spread"]
    for k in im:
        assert torch.equal(bits(im[k]), bits(e["images"][k])), k
    assert "members" not in a.images and not a.members
    for kw in (dict(), dict(ensemble=1), dict(ensemble=(0,))):
        with pytest.raises(ValueError, match="members"):
            make(e, members=True, **kw)
    with pytest.raises(ValueError, match="members=True"):
        a.score_ensemble(torch.zeros((1, 288, 352), device=dev()))


def test_members_come_before_the_consistency_correction():
    e = e2e()
    rs = make(e, ensemble=4, members=True, consistent=2)
    im = rs.super_resolve(e["lr"])
    raw = make(e, ensemble=4, members=True).super_resolve(e["lr"])
    assert torch.equal(bits(im["members"]), bits(raw["members"])) and torch.equal(bits(im["spread"]), bits(raw["spread"]))
    assert not torch.equal(bits(im["model"]), bits(raw["model"]))


@pytest.mark.parametrize("land", [False, True], ids=["sea", "land"])
def test_score_ensemble_is_score_plus_the_measure_of_members(land, tmp_path):
    from srmi.results import load_ensemble_score, save_ensemble_score
    e = e2e()
    d = dev()
    rng = np.random.RandomState(77)
    f0 = rng.randn(1, 288, 352)
    hr = ((f0 + np.roll(f0, 1, 1) + np.roll(f0, 1, 2)) * 2 + 5).astype(np.float32)
    if land:
        hr[0, 40:72, 100:140] = np.nan  # land on whole LR pixels
    hr_d = torch.tensor(hr, device=d)
    kw = dict(land=True, min_wet=0.25) if land else {}
    rs = make(e, ensemble=4, members=True, **kw)
    images0, losses0 = rs.score(hr_d)
    torch.cuda.synchronize()
    images0, losses0 = {k: v.clone() for k, v in images0.items()}, {k: v.clone() for k, v in losses0.items()}
    probs = (0.25, 0.5, 0.75)
    images, losses, got = rs.score_ensemble(hr_d, probs=probs, crps_map=True)
    torch.cuda.synchronize()
    assert set(images) == set(images0) and set(losses) == set(losses0)
    for k in images0:
        assert torch.equal(bits(images[k]), bits(images0[k])), k
    for k in losses0:
        assert torch.equal(bits(losses[k]), bits(losses0[k])), k
    shape = (1, 288, 352)
    edges = DistributionScore(shape, 1024, 0, probs, device=d).measure(images["spread"], images["spread"])["q_truth"].float()
    assert torch.equal(got["edges"], edges) and edges.dtype == torch.float32 and tuple(edges.shape) == (1, 3)
    by_hand = EnsembleScore((4,) + shape, edges, True, device=d).measure(images["members"], hr_d)
    torch.cuda.synchronize()
    m = {k: got[k].cpu().numpy() for k in TABLES + DERIVED + ("sums", "crps_map", "edges")}
    for k in m:
        assert np.array_equal(m[k], by_hand[k].cpu().numpy(), equal_nan=True), k
    # and the oracle on what the device scored
    mem, ed = images["members"].cpu().numpy(), edges.cpu().numpy()
    terms = eo.pixel_terms(mem, hr, ed)
    tabs = eo.tables(terms, 4, 4)
    for k in TABLES:
        assert np.array_equal(m[k], tabs[k]), k
    assert np.array_equal(m["crps_map"], eo.crps_map(terms), equal_nan=True)
    ref = eo.derive(m["sums"], tabs, 4)
    for k in DERIVED:
        assert np.array_equal(m[k], ref[k], equal_nan=True), k
    full = 288 * 352
    assert (m["used"] < full).all() if land else (m["used"] == full).all()
    assert m["bin_count"].sum() == m["used"].sum() and (m["bin_count"] > 0).all()
    print(f"score_ensemble land={land}: crps {m['crps'][0]:.4f} fair {m['crps_fair'][0]:.4f} rmse {m['rmse_mean'][0]:.4f} "
          f"ssr {m['ssr'][0]:.4f} corr {m['spread_error_corr'][0]:.4f} rank_hist {m['rank_hist'][0].tolist()}")
    # the scorers are cached per argument key; explicit edges need no quantile
    n = len(rs._ens)
    rs.score_ensemble(hr_d, probs=probs, crps_map=True)
    assert len(rs._ens) == n
    _, _, fixed = rs.score_ensemble(hr_d, edges=[0.01, 0.02])
    torch.cuda.synchronize()
    assert len(rs._ens) == n + 1 and fixed["edges"].cpu().numpy().tolist() == [[np.float32(0.01), np.float32(0.02)]]
    assert "crps_map" not in fixed and np.array_equal(fixed["rank_hist"].cpu().numpy(), m["rank_hist"])
    with pytest.raises(ValueError, match="probs"):
        rs.score_ensemble(hr_d, probs=())
    with pytest.raises(ValueError):
        rs.score_ensemble(hr_d, edges=[0.0] * 16)
    # the file round trip of a device result
    path = save_ensemble_score(str(tmp_path / "ens.nc"), got, ["SST"])
    back, names = load_ensemble_score(path)
    assert names == ["SST"]
    for k in m:
        assert np.array_equal(back[k], m[k], equal_nan=True) and back[k].dtype == m[k].dtype, k
