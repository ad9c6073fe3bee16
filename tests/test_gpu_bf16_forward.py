"""The bf16 engine's forward, launch by launch (bf16_forward.py), in training and in inference:
the head, conv1 with its strip sums (EPI_RELU_POOL), the CA scale rebuilt from t's statistics
(ca_scale.hpp, conv1's partial means) or from conv2's pooled output, conv2 with the residual
pair update in its epilogue (EPI_CA_RESID_U; EPI_CA_RESID in the one-launch inference RCAB of
rcab_infer.hip), the group and body tails, the upsamplers and the tail conv -- the engine's own
epilogues, which no op-level entry point reaches.  Each launch's outputs are recomputed in fp64
from the operands the engine itself consumed (Engine.buffer and the forward trace) against bars
derived from the number formats alone (bf16_forward's docstring); every check is reported per
image and (g, b).

Cases: 2 groups (a group boundary: the fp32 group output and its bf16 copy) of 3 RCABs (the
fp32-input RCAB b = 1 and the pair-input ones).  Training at 48-wide tiles of 4 rows (the top
and the bottom border in one strip), 8, 12 and 48, 1 and 3 images, CA bottlenecks of 32, 8 and 4
channels, the whole chip and a 128-CU budget (another run partition of conv1's partial means),
the CA inside conv2 and SRMI_FLAG_CA_PASS, a capacity of 3 with 2 images; 8 x 32 and 24 x 96
tiles (always the CA pass; 96 wide: two column blocks per row).  Inference at 48-wide tiles of 4,
8, 32 and 48 rows, 1, 3 and 5 images, the one-launch RCAB and SRMI_FLAG_NO_RCAB_INFER."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import bf16_forward as bfw  # noqa: E402
import bf16_stages as bs  # noqa: E402
from srmi._lib import SRMI_FLAG_CA_PASS, SRMI_FLAG_NO_RCAB_INFER  # noqa: E402

#         (h, w)   cb   B  cu_budget flags capacity
TRAIN = [
    ((4, 48), 2, 1, 0, 0, None),
    ((4, 48), 16, 3, 128, 0, None),
    ((4, 48), 8, 3, 0, SRMI_FLAG_CA_PASS, None),
    ((8, 48), 16, 1, 0, 0, None),
    ((8, 48), 2, 3, 128, 0, None),
    ((8, 48), 8, 2, 0, 0, 3),
    ((8, 48), 16, 3, 0, SRMI_FLAG_CA_PASS, None),
    ((12, 48), 8, 1, 128, 0, None),
    ((12, 48), 16, 3, 0, 0, None),
    ((12, 48), 2, 2, 128, SRMI_FLAG_CA_PASS, 3),
    ((48, 48), 16, 3, 0, 0, None),
    ((48, 48), 2, 1, 128, 0, None),
    ((48, 48), 8, 3, 128, 0, None),
    ((48, 48), 2, 3, 0, SRMI_FLAG_CA_PASS, None),
    ((8, 32), 2, 3, 0, 0, None),
    ((8, 32), 16, 1, 128, 0, None),
    ((24, 96), 16, 3, 0, 0, None),
    ((24, 96), 8, 1, 128, 0, None),
]
INFER = [
    ((4, 48), 2, 1, 0, 0, None),
    ((4, 48), 16, 5, 0, 0, None),
    ((4, 48), 8, 3, 0, SRMI_FLAG_NO_RCAB_INFER, None),
    ((8, 48), 16, 1, 0, 0, None),
    ((8, 48), 8, 3, 0, 0, None),
    ((8, 48), 2, 5, 0, SRMI_FLAG_NO_RCAB_INFER, None),
    ((32, 48), 2, 3, 0, 0, None),
    ((32, 48), 16, 1, 0, SRMI_FLAG_NO_RCAB_INFER, None),
    ((48, 48), 8, 1, 0, 0, None),
    ((48, 48), 16, 5, 0, 0, None),
    ((48, 48), 2, 3, 0, 0, None),
    ((48, 48), 16, 3, 0, SRMI_FLAG_NO_RCAB_INFER, None),
]


def _id(kind, c):
    return (f"{kind}-{c[0][0]}x{c[0][1]}-cb{c[1]}-B{c[2]}-cu{c[3]}" + (f"-flags{c[4]}" if c[4] else "")
            + (f"-cap{c[5]}" if c[5] else ""))


CASES = [pytest.param(True, *c, id=_id("train", c)) for c in TRAIN] + \
        [pytest.param(False, *c, id=_id("infer", c)) for c in INFER]
INFER_CASES = [pytest.param(False, *c, id=_id("infer", c)) for c in INFER]
ARGS = "train,hw,cb,B,cu,flags,cap"


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _run(train, hw, cb, B, cu, flags, cap):
    rep, info = bfw.run_case(bs.make_case(hw, cb, B, cu, flags), dev(), train=train, capacity=cap)
    info = {k: (f"{min(v):.3g} - {max(v):.3g}" if isinstance(v, list) else v) for k, v in info.items()}
    print(f"\n{'train' if train else 'infer'} {hw} cb {cb} B {B} cu {cu} flags {flags} cap {cap}: {info}")
    for cls in "abcdefgr":
        for kind, (ratio, row) in sorted(rep.worst(cls).items()):
            print(f"  ({cls}) worst {kind}: {row[4]:.3e} (bar {row[5]:.3e}) {row[1]} {row[2]} {row[3]}")
    return rep, info


def _check(cls, args):
    rep, _ = _run(*args)
    assert any(r[0] == cls for r in rep.rows)
    assert not rep.failures(cls), rep.failures(cls)


@pytest.mark.parametrize(ARGS, CASES)
def test_launch_paths_are_the_ones_the_case_is_for(train, hw, cb, B, cu, flags, cap):
    """Training at 48-wide tiles runs the CA inside conv2's launch unless SRMI_FLAG_CA_PASS,
    other widths always the CA pass; inference at 48-wide tiles runs the one-launch RCAB unless
    SRMI_FLAG_NO_RCAB_INFER (srmi_engine_probe which = 8)."""
    info = _run(train, hw, cb, B, cu, flags, cap)[1]
    if train:
        want = 1 if hw[1] == 48 and not flags & SRMI_FLAG_CA_PASS else 0
    else:
        want = 2 if hw[1] == 48 and not flags & SRMI_FLAG_NO_RCAB_INFER else 0
    assert info["form"] == want, bfw.FORMS[info["form"]]
    assert info["n"] == B and info["capacity"] == (cap or B)


@pytest.mark.parametrize(ARGS, CASES)
def test_head_closes(train, hw, cb, B, cu, flags, cap):
    """(a) X0F = the fp64 head conv of lr (fp32 weights); hb(0, 0) bit-identical to the
    round-to-nearest-even of the engine's X0F (head_fwd_kernel: f2bf)."""
    _check("a", (train, hw, cb, B, cu, flags, cap))


@pytest.mark.parametrize(ARGS, CASES)
def test_conv1_closes(train, hw, cb, B, cu, flags, cap):
    """(b) t(g, b) = bf16(relu(conv(hb(g, b - 1)) + b1)); where conv1 writes the strip records
    (the CA inside conv2, the one-launch RCAB) each record = the sums of the STORED bf16 t."""
    _check("b", (train, hw, cb, B, cu, flags, cap))


@pytest.mark.parametrize(ARGS, CASES)
def test_ca_scale_closes(train, hw, cb, B, cu, flags, cap):
    """(c) REC = m | z1 | s: m per image and channel = b2 + mean(conv2_fp64(stored t, bf16(W2)))
    (in the CA-pass forms also each strip record of conv2's fp32 output); z1, s = the fp64 MLP of
    the engine's m; a bottleneck ReLU decision that differs from fp64's lies within z1's bound."""
    _check("c", (train, hw, cb, B, cu, flags, cap))


@pytest.mark.parametrize(ARGS, [c for c in CASES if c.values[0]])
def test_conv2_closes(train, hw, cb, B, cu, flags, cap):
    """(d) Training: the stored u(g, b) = bf16(conv(t) + b2)."""
    _check("d", (train, hw, cb, B, cu, flags, cap))


@pytest.mark.parametrize(ARGS, CASES)
def test_residual_pair_closes(train, hw, cb, B, cu, flags, cap):
    """(e) decode(hb(g, b), lo(g, b)) = h_in + s_engine u to the multiply-add's fp32 rounding
    plus the codec's 128 fp32 steps, h_in the fp32 group input (b = 1) or the decoded pair
    before; hi == (A' + 0x8000) >> 16 bit for bit.  u is the stored bf16 u in training and
    bf16(conv2_fp64(t) + b2), or a bf16 neighbour the accumulation bound admits, in inference:
    the engine adds s bf16(u), in the one-launch RCAB too -- with the
    fp32 u the elements would be off by up to half a bf16 ulp of u times s, between the
    candidates and far outside this bound."""
    _check("e", (train, hw, cb, B, cu, flags, cap))


@pytest.mark.parametrize(ARGS, CASES)
def test_group_tail_closes(train, hw, cb, B, cu, flags, cap):
    """(f) The fp32 group output = conv(hb(g, nb)) + b + the group input; hb(g + 1, 0)
    bit-identical to its round-to-nearest-even."""
    _check("f", (train, hw, cb, B, cu, flags, cap))


@pytest.mark.parametrize(ARGS, CASES)
def test_tails_and_upsamplers_close(train, hw, cb, B, cu, flags, cap):
    """(g) RESb = bf16(conv(hb(nl, 0)) + b + X0F); PS[k] = bf16(pixel_shuffle(conv(.) + b)) in
    torch's channel order; sr = the fp64 tail conv (bf16-rounded weights) of the last PS."""
    _check("g", (train, hw, cb, B, cu, flags, cap))


@pytest.mark.parametrize(ARGS, INFER_CASES)
def test_inference_pair_allowance_is_rare(train, hw, cb, B, cu, flags, cap):
    """(r) The guard of (e) in inference, where u is not stored: at most 1e-3 of any map may be
    held to a bound wider than training's.  None is: an element whose exact conv2 output lies
    within the accumulation bound of a bf16 rounding boundary is not given its ulp x s as
    allowance but must match r = bf16(conv2_fp64(t) + b2) or the admissible neighbour across
    that boundary at that candidate's own bound.  (About half of every map has such a
    neighbour -- 0.47 - 0.55 measured, and the same for the fp64 oracle alone on the CPU: the
    any-order bound of a 577-term sum that cancels is about 0.4 of half a bf16 ulp of the
    result -- so an allowance for them would have hollowed the check out; _run prints the
    shares of elements with an admissible neighbour and of those that took one.)"""
    _check("r", (train, hw, cb, B, cu, flags, cap))


@pytest.mark.parametrize("train,hw,cu,flags", [(True, (48, 48), 0, 0), (True, (8, 48), 128, SRMI_FLAG_CA_PASS),
                                                (True, (8, 32), 0, 0), (False, (8, 48), 0, 0),
                                                (False, (48, 48), 0, SRMI_FLAG_NO_RCAB_INFER)])
def test_forward_trace_changes_nothing(train, hw, cu, flags):
    """(h) A forward with the forward trace off, on, and off again on the same engine: sr and
    every persisting map (X0F, RESb, PS[k]; training: every hb, t, u and CA record) are
    bit-identical; the trace buffer is written while on and untouched while off."""
    differ, written, untouched = bfw.trace_changes_nothing(bs.make_case(hw, 16, 3, cu, flags), dev(), train)
    assert differ == []
    assert written and untouched
