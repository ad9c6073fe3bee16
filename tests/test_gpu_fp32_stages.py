"""The exact-fp32 engine (SRMI_DTYPE_F32) one level below the whole step: per image and per
stage, the maps its forward saves and its backward stages leave behind (read in place
through srmi_engine_buffer) against the fp64 oracle's intermediates, the filter gradients
against an fp64 recomputation from the engine's own operands, and a batch of two against
the same two images run alone.

Driven with a fixed upstream dy (no loss), so an image's backward does not depend on the
batch.  Bars: 5e-5 rel-L2 per image and map -- the level every healthy fp32 gradient tensor
of this model holds -- or ten times the drift of fp32 torch on the CPU from
fp64 for that map where that is larger (measured in the same test: at most 6e-7 for these
cases, so 5e-5 holds everywhere); 1e-5 for the filter-gradient closure (test_wgrad's bar
for the same kernel); bit identity for the batch split's maps and 1e-6 for its parameter
gradients (fp32 summation order, as test_fp32_micro_batch_step_matches_single_engine).

What they found: the gradient offset of group 0's first RCAB, once
taken for a composition defect, is a single ReLU decision at a pre-activation of +3.9e-8.
A backward map below such an element cannot match fp64 in ANY fp32 arithmetic that rounds
it the other way, so the backward maps are compared twice: against the plain fp64 oracle
(test_backward_maps_vs_oracle; fails at 48 x 48 for that reason and is kept as a strict
expected failure that names the element) and against the fp64 oracle run with the
engine's own ReLU masks (test_backward_maps_vs_mask_aligned_oracle), after
test_relu_masks_differ_from_fp64_only_inside_fp32_rounding has held those masks to fp64's
wherever an fp32 sum can tell the sign."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import fp32_stages as fs  # noqa: E402
from fp32_stages import rel_l2  # noqa: E402

TILES = [(48, 48), (8, 32)]  # the flagship tile (3 x 4 row chunks, TW 48) and the smallest the engine takes (TW 32)
DEPTHS = [(1, 1), (1, 3), (2, 3), (3, 1)]
CASES = [pytest.param(hw, cb, nl, nb, id=f"{hw[0]}x{hw[1]}-cb{cb}-{nl}x{nb}")
         for hw in TILES for cb in (2, 16) for nl, nb in DEPTHS]
SPLIT_CASES = CASES + [pytest.param(hw, cb, 2, 8, id=f"{hw[0]}x{hw[1]}-cb{cb}-2x8") for hw in TILES for cb in (2, 16)]
BAR = 5e-5


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _case(hw, cb, nl, nb):
    return fs.make_case(nl, nb, cb, hw)


@functools.lru_cache(maxsize=None)
def _oracle(hw, cb, nl, nb):
    return fs.oracle_pair(_case(hw, cb, nl, nb))


@functools.lru_cache(maxsize=None)
def _engine(hw, cb, nl, nb):
    return fs.engine_stages(_case(hw, cb, nl, nb), dev())


def _check_maps(keys, eng, ref, drift, what):
    bad = []
    worst = (0.0, None)
    for key in keys:
        for n in range(ref[key].shape[0]):
            err = rel_l2(eng[key][n], ref[key][n])
            bar = max(BAR, 10 * drift[key][n])
            worst = max(worst, (err, (key, n)))
            if not err < bar:
                bad.append((key, f"image {n}", f"engine {err:.2e}", f"fp32 CPU {drift[key][n]:.2e}", f"bar {bar:.1e}"))
    print(f"\n{what}: worst engine {worst[0]:.2e} at {worst[1]}; worst fp32 CPU drift "
          f"{max(max(drift[k]) for k in keys):.2e}")
    assert not bad, bad


@pytest.mark.parametrize("hw,cb,nl,nb", CASES)
def test_forward_maps_vs_oracle(hw, cb, nl, nb):
    """(a) hb(0, 0), every t, u and hb(g, b), per image."""
    ref, drift = _oracle(hw, cb, nl, nb)
    keys = [k for k in ref if k != "grads" and k[0] in ("hb", "t", "u")]
    assert len(keys) == nl * (3 * nb + 1) + 1
    _check_maps(keys, _engine(hw, cb, nl, nb), ref, drift, "forward maps")


@pytest.mark.parametrize("hw,cb,nl,nb", CASES)
def test_saved_state_survives_backward(hw, cb, nl, nb):
    """(b) The first slot of each saved array (hb(0, 0), t, u and the CA record of group 0's
    first RCAB) is bit-identical to its post-forward snapshot after every backward stage,
    the head's included."""
    assert _engine(hw, cb, nl, nb)["clobbered"] == []


FLIP = ("DZ after the stage of group 0, image 1: conv1 of group 0's first RCAB has the pre-activation z[c 52, y 21, "
        "x 23] = +3.9e-8 in fp64 (+3.0e-8 in fp32 torch), inside the fp32 rounding error of zero; the engine's fp32 sum "
        "lands on the other side, so its ReLU mask drops that one element of dz (|dt| / ||dz|| = 2.0e-3 .. 2.4e-3 "
        "there, exactly the measured error) and everything below it follows: no defect "
        "(test_backward_maps_vs_mask_aligned_oracle)")
CASES_C = [pytest.param(*p.values, id=p.id,
                        marks=[pytest.mark.xfail(strict=True, reason=FLIP)] if p.values[0] == (48, 48) else [])
           for p in CASES]


@pytest.mark.parametrize("hw,cb,nl,nb", CASES_C)
def test_backward_maps_vs_oracle(hw, cb, nl, nb):
    """(c) dRES after stage 0; after the stage of group g its first RCAB's dz and du (what
    the stage leaves in DZ / DU) and the gradient w.r.t. the group's input, per image,
    against the plain fp64 oracle at 5e-5.

    Fails at 48 x 48 (measured, cb 16, 2 x 3: dz(0, 1) image 1 2.03e-3, gin(0) image 1
    7.2e-5, every other map 1.2e-6 .. 1.4e-6; 1 x 1 cb 2: 2.29e-3 / 7.2e-5; 3 x 1: also
    dz(1, 1) image 0 9.85e-3, where z = +2.2e-7, and the maps below it 3.7e-4 .. 5.7e-4):
    one ReLU decision per affected map differs from fp64's at a pre-activation inside the
    fp32 rounding error of zero (FLIP).  Passes at 8 x 32, whose tiles hold no such element."""
    ref, drift = _oracle(hw, cb, nl, nb)
    keys = [("dres",)] + [k for g in range(nl) for k in (("dz", g, 1), ("du", g, 1), ("gin", g))]
    _check_maps(keys, _engine(hw, cb, nl, nb), ref, drift, "backward maps")


@functools.lru_cache(maxsize=None)
def _aligned(hw, cb, nl, nb):
    eng = _engine(hw, cb, nl, nb)
    return fs.oracle_with_masks(_case(hw, cb, nl, nb), {k[1:]: v for k, v in eng.items()
                                                        if isinstance(k, tuple) and k[0] == "t"})


@pytest.mark.parametrize("hw,cb,nl,nb", CASES)
def test_relu_masks_differ_from_fp64_only_inside_fp32_rounding(hw, cb, nl, nb):
    """Every element where the engine's ReLU mask (t > 0) differs from fp64's (z > 0) has
    |z| within the a-priori bound on the fp32 rounding error of conv1's sum there
    (fp32_stages.Z_TOL: any summation order), and they are few: below 1e-5 of the map."""
    ref, _ = _oracle(hw, cb, nl, nb)
    eng = _engine(hw, cb, nl, nb)
    flips, bad = fs.mask_flips(ref, {k[1:]: v for k, v in eng.items() if isinstance(k, tuple) and k[0] == "t"})
    print(f"\nReLU decisions that differ from fp64: {flips}")
    assert not bad, (bad, flips)


@pytest.mark.parametrize("hw,cb,nl,nb", CASES)
def test_backward_maps_vs_mask_aligned_oracle(hw, cb, nl, nb):
    """(c) again, against the fp64 oracle run with the engine's own ReLU masks (which
    test_relu_masks_differ_from_fp64_only_inside_fp32_rounding holds to fp64's wherever
    fp32 can tell): the same maps at the same 5e-5 per image, and every parameter gradient
    at 5e-5 (or ten times its fp32-CPU drift).  With the one legitimate degree of freedom
    of an fp32 backward taken out, any buffer, stride or launch-order error shows."""
    case = _case(hw, cb, nl, nb)
    ref, drift = _aligned(hw, cb, nl, nb), _oracle(hw, cb, nl, nb)[1]
    eng = _engine(hw, cb, nl, nb)
    keys = [("dres",)] + [k for g in range(nl) for k in (("dz", g, 1), ("du", g, 1), ("gin", g))]
    _check_maps(keys, eng, ref, drift, "backward maps, engine's ReLU masks")
    errs = sorted(((rel_l2(eng["grads"][off:off + n].view(shape), ref["grads"][name]), name)
                   for name, off, n, shape in case["table"]), reverse=True)
    print(f"worst parameter gradients: {[(f'{e:.2e}', nm) for e, nm in errs[:3]]}; worst fp32 CPU drift "
          f"{max(drift['grads'].values()):.2e}")
    bad = [(nm, e) for e, nm in errs if not e < max(BAR, 10 * drift["grads"][nm])]
    assert not bad, bad


def _nchw64(x):
    return x.double().permute(0, 3, 1, 2)


@pytest.mark.parametrize("hw,cb,nl,nb", CASES)
def test_first_rcab_filter_gradients_close_over_engine_operands(hw, cb, nl, nb):
    """(d) Group 0's first RCAB: conv1's and conv2's filter gradients and conv1's bias
    gradient recomputed in fp64 from the engine's own hb(0, 0), DZ, t and DU (as they are
    right after group 0's stage) against what the engine's filter-gradient launches, slab
    sets and group-end reduction put into grads: 1e-5 rel-L2."""
    case, eng = _case(hw, cb, nl, nb), _engine(hw, cb, nl, nb)
    c = eng["closure"]
    x, dz, t, du = (_nchw64(c[k]) for k in ("hb00", "dz", "t01", "du"))
    want = {
        "body.0.body.0.body.0.weight": torch.nn.grad.conv2d_weight(x, (64, 64, 3, 3), dz, padding=1),
        "body.0.body.0.body.0.bias": dz.sum((0, 2, 3)),
        "body.0.body.0.body.2.weight": torch.nn.grad.conv2d_weight(t, (64, 64, 3, 3), du, padding=1),
        "body.0.body.0.body.2.bias": du.sum((0, 2, 3)),
    }
    tab = {name: (off, n, shape) for name, off, n, shape in case["table"]}
    bad = []
    for name, w in want.items():
        off, n, shape = tab[name]
        err = rel_l2(eng["grads"][off:off + n].view(shape), w)
        print(f"\nclosure {name}: {err:.2e}")
        if not err < 1e-5:
            bad.append((name, err))
    assert not bad, bad


@pytest.mark.parametrize("hw,cb,nl,nb", SPLIT_CASES)
def test_batch_of_two_equals_two_single_images(hw, cb, nl, nb):
    """(e) Oracle-free: the B = 2 run against the same two images run alone, on an engine of
    capacity 2 called with n = 1 and on an engine of capacity 1.  No map kernel sums across
    images, so every per-image map of (a) and (c) is bit-identical; every parameter-gradient
    tensor of the B = 2 run equals the fp64 sum of the two single-image runs to 1e-6 rel-L2
    (fp32 summation order)."""
    case = _case(hw, cb, nl, nb)
    both = _engine(hw, cb, nl, nb)
    map_keys = [k for k in both if isinstance(k, tuple)]
    for capacity in (2, 1):
        singles = [fs.engine_stages(case, dev(), capacity=capacity, images=slice(n, n + 1)) for n in range(2)]
        differ = [(k, f"image {n}", f"capacity {capacity}", f"{rel_l2(both[k][n], singles[n][k][0]):.2e}")
                  for k in map_keys for n in range(2) if not torch.equal(both[k][n], singles[n][k][0])]
        assert not differ, differ
        assert all(s["clobbered"] == [] for s in singles)
        gsum = singles[0]["grads"].double() + singles[1]["grads"].double()
        errs = sorted(((rel_l2(both["grads"][off:off + n], gsum[off:off + n]), name)
                       for name, off, n, _ in case["table"]), reverse=True)
        print(f"\ncapacity {capacity}: worst B=2 vs sum of singles {[(f'{e:.2e}', nm) for e, nm in errs[:3]]}")
        assert errs[0][0] < 1e-6, errs[:4]


def test_engine_buffer_refuses_what_the_engine_lacks():
    from srmi._lib import SrmiError
    from srmi.engine import Engine, NetSpec
    d = dev()
    rcan = NetSpec(arch="rcan", nchannels_in=1, nchannels_out=1, nlayers=2, nblocks=2, scale=4, dtype="fp32")
    edsr = NetSpec(arch="edsr", nchannels_in=1, nchannels_out=1, nlayers=2, scale=4, dtype="fp32")
    tr = Engine(rcan, 2, (8, 32), train=True, device=d)
    assert tr.buffer("HB", 2, 0).shape == (2, 8, 32, 64) and tr.buffer("HB", 2, 0).dtype == torch.float32
    assert tr.buffer("REC", 1, 2).shape == (2, 160) and tr.buffer("BREC", 0, 1).shape == (2, 224)
    assert tr.buffer("T", 0, 1).data_ptr() >= tr.workspace.data_ptr()  # a view, not a copy
    # the two fp32 gradient streams alternate from group to group
    assert tr.buffer("GROUP_IN_GRAD", 1).data_ptr() != tr.buffer("GROUP_IN_GRAD", 0).data_ptr()
    for name, g, b in (("HB", 3, 0), ("HB", 2, 1), ("HB", 0, 3), ("T", 0, 0), ("T", 0, 3), ("U", 2, 1), ("REC", 0, 0),
                       ("GROUP_IN_GRAD", 2, 0), ("GROUP_IN_GRAD", -1, 0)):
        with pytest.raises(SrmiError):
            tr.buffer(name, g, b)
    with pytest.raises(SrmiError):
        tr.buffer("NOPE")
    inf = Engine(rcan, 2, (8, 32), train=False, device=d)
    assert inf.buffer("X0F").shape == (2, 8, 32, 64)
    for name in ("HB", "T", "U", "REC", "BREC", "DU", "DZ", "DRESF", "GROUP_IN_GRAD"):
        with pytest.raises(SrmiError):
            inf.buffer(name, 0, 1 if name in ("T", "U", "REC", "BREC") else 0)
    ed = Engine(edsr, 2, (8, 32), train=True, device=d)
    assert ed.buffer("HB", 2, 0).shape == (2, 8, 32, 64) and ed.buffer("T", 1, 1).shape == (2, 8, 32, 64)
    assert ed.buffer("DZ").dtype == torch.float32
    for name, g, b in (("U", 0, 1), ("REC", 0, 1), ("BREC", 0, 1), ("DU", 0, 0), ("GROUP_IN_GRAD", 0, 0), ("HB", 0, 1)):
        with pytest.raises(SrmiError):
            ed.buffer(name, g, b)
    bf = Engine(NetSpec(arch="rcan", nchannels_in=1, nchannels_out=1, nlayers=1, nblocks=1, scale=4), 1, (48, 48),
                train=True, device=d)
    assert bf.buffer("T", 0, 1).dtype == torch.bfloat16 and bf.buffer("X0F").dtype == torch.float32
    # the backward trace: off by default and refused where there is nothing to trace
    with pytest.raises(SrmiError):
        tr.trace_view("DZ", 0, 1)
    for other in (inf, ed):
        with pytest.raises(SrmiError):
            other.trace(True)
    tr.trace(True)
    assert tr.trace_view("STREAM", 1, 0).shape == (2, 8, 32, 64) and tr.trace_view("DZ", 0, 2).dtype == torch.float32
    assert tr.trace_view("PACC", 0, 1).shape[0] == 2 and tr.trace_view("PACC", 0, 1).shape[2] == 128
    assert bf.trace(True) is not None and bf.trace_view("GRB", 0, 0).dtype == torch.bfloat16
    for name, g, b in (("GRB", 0, 1), ("GRB", 2, 0), ("STREAM", 0, 3), ("STREAM", 0, -1), ("PACC", 0, 0), ("DZ", 0, 3),
                       ("DU", -1, 1), ("DU", 0, 0)):
        with pytest.raises(SrmiError):
            tr.trace_view(name, g, b)
    with pytest.raises(SrmiError):
        tr.trace_view("NOPE")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_trace_off_leaves_the_backward_bit_identical(dtype):
    """One step with the trace on, then one without on the same engine, and a fresh engine
    that never had one: the same outputs and gradients bit for bit (the trace adds copies
    between the launches and changes no launch); with it off nothing is written to the buffer."""
    import dataclasses
    from srmi.engine import Engine
    case = _case((48, 48), 16, 2, 3)
    spec = dataclasses.replace(case["spec"], dtype=dtype)
    d = dev()
    lr, dy, flat = case["lr"].to(d), case["dy"].to(d), case["flat"].to(d)

    def step(eng):
        out = eng.forward(flat, lr)
        grads = torch.zeros(eng.n_params, device=d)
        eng.backward(flat, lr, grads, dy=dy)
        torch.cuda.synchronize()
        return out.clone(), grads

    eng = Engine(spec, case["B"], (48, 48), train=True, device=d)
    eng.pack(flat)
    buf = eng.trace(True)
    traced = step(eng)
    assert bool(buf.any())
    eng.trace(False)
    buf.zero_()
    plain = step(eng)
    assert not bool(buf.any())
    fresh = Engine(spec, case["B"], (48, 48), train=True, device=d)
    fresh.pack(flat)
    never = step(fresh)
    for a, b in ((traced, never), (plain, never)):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
