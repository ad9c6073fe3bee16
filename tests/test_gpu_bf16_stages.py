"""The bf16 engine's RCAB backward, launch by launch (bf16_stages.py): the fused dgrad ||
filter-gradient launches with the bf16 in-group gradient stream (epilogues 11 - 13), the
CALayer backward inside the conv2 backward, the bf16 partial slabs with the group-end batched
reduction, and the batched CA parameter gradients -- none of which an op-level entry point
reaches.  Each launch's outputs are recomputed in fp64 from the operands the engine itself
consumed (read through Engine.buffer and the backward trace), against bars derived from the
number formats alone (bf16_stages' docstring); every check is reported per image and (g, b).

Cases: 2 groups (the two gradient buffers swap) of 3 RCABs (a last, a middle and a first one:
epilogues 12, 11, 13); fused launches at 48-wide tiles of 4 (one row chunk per image), 8, 12
and 48 rows, the separate launches with du in memory at 8 x 32 (fp32 slabs) and 24 x 96 (bf16
slabs, two column blocks); 1 and 3 images; CA bottlenecks of 32 and 4 channels; the whole chip
and the two-engine trainer's half (other run lengths and row chunks); SRMI_FLAG_DU_PASS once."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import bf16_stages as bs  # noqa: E402
from srmi._lib import SRMI_FLAG_DU_PASS  # noqa: E402

#        (h, w)   cb   B  cu_budget flags
CONFIGS = [
    ((4, 48), 2, 1, 0, 0),
    ((4, 48), 16, 3, 128, 0),
    ((8, 48), 16, 1, 0, 0),
    ((8, 48), 2, 3, 128, 0),
    ((8, 48), 16, 3, 0, SRMI_FLAG_DU_PASS),
    ((12, 48), 2, 1, 128, 0),
    ((12, 48), 16, 3, 0, 0),
    ((48, 48), 16, 3, 0, 0),
    ((48, 48), 2, 1, 128, 0),
    ((48, 48), 2, 3, 128, 0),
    ((8, 32), 2, 3, 0, 0),
    ((8, 32), 16, 1, 128, 0),
    ((24, 96), 16, 3, 0, 0),
    ((24, 96), 2, 1, 128, 0),
]
CASES = [pytest.param(*c, id=f"{c[0][0]}x{c[0][1]}-cb{c[1]}-B{c[2]}-cu{c[3]}" + ("-dupass" if c[4] else ""))
         for c in CONFIGS]


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _run(hw, cb, B, cu, flags):
    rep, info = bs.run_case(bs.make_case(hw, cb, B, cu, flags), dev())
    print(f"\n{hw} cb {cb} B {B} cu {cu} flags {flags}: {info}")
    for cls in "abcdef":
        for kind, (ratio, row) in sorted(rep.worst(cls).items()):
            print(f"  ({cls}) worst {kind}: {row[4]:.3e} (bar {row[5]:.3e}) {row[1]} {row[2]} {row[3]}")
    return rep, info


def _check(cls, args):
    rep, _ = _run(*args)
    assert any(r[0] == cls for r in rep.rows)
    assert not rep.failures(cls), rep.failures(cls)


@pytest.mark.parametrize("hw,cb,B,cu,flags", CASES)
def test_launch_paths_are_the_ones_the_case_is_for(hw, cb, B, cu, flags):
    """48-wide tiles run the fused launches with bf16 partial slabs and du formed inside F2
    (unless SRMI_FLAG_DU_PASS); the others run separate launches with du in memory; H = 4 is
    one row chunk per image."""
    info = _run(hw, cb, B, cu, flags)[1]
    assert info["fused"] == (hw[1] == 48)
    assert info["du_fused"] == (hw[1] == 48 and not flags)
    assert info["slab16"] == (hw[1] % 48 == 0)
    assert hw[0] % info["rs1"] == 0 and (hw[0] // info["rs1"]) % 4 == 0
    assert hw[0] % info["rs2"] == 0 and (hw[0] // info["rs2"]) % 4 == 0
    if hw[0] == 4:
        assert info["rs1"] == info["rs2"] == 1


@pytest.mark.parametrize("hw,cb,B,cu,flags", CASES)
def test_group_tail_closes(hw, cb, B, cu, flags):
    """(a) Epilogue 12: the stream's start = bf16(dgrad of the group tail over the bf16 group
    output gradient); pacc = the sums of the stored bf16 stream and of stream * u(g, nb); the
    group tail's filter and bias gradient over (hb(g, nb), that gradient)."""
    _check("a", (hw, cb, B, cu, flags))


@pytest.mark.parametrize("hw,cb,B,cu,flags", CASES)
def test_ca_backward_records_close(hw, cb, B, cu, flags):
    """(b) BREC's dz2, dz1, conv2-bias-gradient segment and dm = the fp64 MLP backward from
    pacc, REC (m, z1, s; the hidden ReLU decisions from z1) and the fp32 w1, w2."""
    _check("b", (hw, cb, B, cu, flags))


@pytest.mark.parametrize("hw,cb,B,cu,flags", CASES)
def test_conv2_dgrad_role_closes(hw, cb, B, cu, flags):
    """(c) dz = bf16(dgrad_conv2(du) (t > 0)) with du = bf16(g s + dm / HW) from the traced
    stream and the engine's records (or the engine's own du map where it writes one, itself
    held to that formula)."""
    _check("c", (hw, cb, B, cu, flags))


@pytest.mark.parametrize("hw,cb,B,cu,flags", CASES)
def test_conv2_filter_role_closes(hw, cb, B, cu, flags):
    """(d) conv2's filter gradient = the sum of the (bf16-rounded) partials of wgrad(t, du),
    its bias gradient = sum du: the only observation of the du the filter role forms."""
    _check("d", (hw, cb, B, cu, flags))


@pytest.mark.parametrize("hw,cb,B,cu,flags", CASES)
def test_conv1_backward_closes(hw, cb, B, cu, flags):
    """(e) Epilogue 11 (b > 1): stream = bf16(dgrad_conv1(dz) + stream), pacc its sums with
    u(g, b - 1); epilogue 13 (b = 1): the fp32 group input gradient = dgrad_conv1(dz) + stream
    + the group output gradient (+ dRES for group 0) and the stream's end its bf16 rounding;
    conv1's filter and bias gradient over (hb(g, b - 1), dz)."""
    _check("e", (hw, cb, B, cu, flags))


@pytest.mark.parametrize("hw,cb,B,cu,flags", CASES)
def test_ca_parameter_gradients_close(hw, cb, B, cu, flags):
    """(f) conv_du.0 / conv_du.2 weight and bias gradients and conv2's bias gradient of every
    RCAB slot = its REC / BREC records summed over the images."""
    _check("f", (hw, cb, B, cu, flags))


@pytest.mark.parametrize("hw,cb,B,cu,flags", CASES)
def test_saved_forward_state_survives_every_stage(hw, cb, B, cu, flags):
    """(g) Every hb, t, u and CA record is bit-identical to its post-forward snapshot after
    every backward stage."""
    assert _run(hw, cb, B, cu, flags)[1]["clobbered"] == []


@pytest.mark.parametrize("hw,cu,flags", [((48, 48), 0, 0), ((8, 48), 128, SRMI_FLAG_DU_PASS), ((8, 32), 0, 0)])
def test_trace_changes_nothing(hw, cu, flags):
    """One training-shaped step (forward, whole backward) with the trace off, on, and off
    again on the same engine: outputs and gradients bit-identical; the trace buffer is
    untouched while off."""
    from srmi.engine import Engine
    case = bs.make_case(hw, 16, 3, cu, flags)
    d = dev()
    lr, dy, flat = case["lr"].to(d), case["dy"].to(d), case["flat"].to(d)
    eng = Engine(case["spec"], 3, hw, train=True, device=d, cu_budget=cu)
    eng.pack(flat)
    runs = []
    for on in (False, True, False):
        if on:
            buf = eng.trace(True)
        elif len(runs):
            eng.trace(False)
            buf.zero_()
        out = eng.forward(flat, lr)
        grads = torch.zeros(eng.n_params, device=d)
        eng.backward(flat, lr, grads, dy=dy)
        torch.cuda.synchronize()
        runs.append((out.clone(), grads))
        if on:
            assert bool(buf.any())
    assert not bool(buf.any())
    for out, grads in runs[1:]:
        assert torch.equal(out, runs[0][0]) and torch.equal(grads, runs[0][1])
