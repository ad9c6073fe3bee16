"""The bf16 engine's backward outside the residual groups, launch by launch (bf16_outer.py): the
tail conv's dgrad (tail_dgrad_kernel<64 | 32>) and filter gradient (tail_wgrad_lds_kernel<1..4>
with slab_reduce_kernel<1>), the upsamplers' unshuffle dgrads and filter gradients, the body
tail's, and the head's filter gradient (head_wgrad_kernel with slab_reduce_kernel<0>) -- stage 0
and stage nlayers + 1 of srmi_backward_stages, as the engine issues them -- and EDSR's one-stage
backward (res_scale as the filter gradient's alpha).  Each launch's outputs are recomputed in fp64
from the operands the engine itself consumed (Engine.buffer: DPS, DRESB, BODY_GRAD, HEAD_GRAD and
the saved forward maps), against bars derived from the number formats alone (bf16_outer's
docstring); tests/test_bf16_outer_checks.py shows on the CPU what each class catches.

Cases (bf16_outer.CONFIGS): the smallest shapes the engine accepts that reach TWT 64 and 32, a
partial last tail segment (HR widths 96 and 288), 1 .. 4 output and input channels, 1, 2 and 3
upsamplers, both dy forms (explicit; (sr - hr) * loss4[2] formed on the fly), n below the engine's
capacity, a cu_budget, several row bands and images per slab reduction; EDSR at nlayers 1
(res_scale 0.5, the whole ResBlock backward and the forward from saved maps) and 2."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import bf16_outer as bo  # noqa: E402

CASES = [pytest.param(c, id=bo.case_id(c)) for c in bo.CONFIGS]
RCAN = [pytest.param(c, id=bo.case_id(c)) for c in bo.CONFIGS if c[0] == "rcan"]
EDSR = [pytest.param(c, id=bo.case_id(c)) for c in bo.CONFIGS if c[0] == "edsr"]
EDSR1 = [pytest.param(c, id=bo.case_id(c)) for c in bo.CONFIGS if c[0] == "edsr" and c[9] == 1]


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _run(c):
    case = bo.make_case(*c)
    st = bo.engine_state(case, dev())
    rep = bo.check_all(st)
    print(f"\n{bo.case_id(c)}: {bo.launch_paths(c)}")
    print("\n".join(bo.report_lines(rep, bo.classes_of(case))))
    return case, st, rep


def _check(cls, c):
    rep = _run(c)[2]
    assert any(r[0] == cls for r in rep.rows)
    assert not rep.failures(cls), rep.failures(cls)


def test_launch_paths_are_the_ones_the_case_is_for():
    """From shapes alone: the cases together reach both tail dgrad tile widths, a partial last
    segment of the tail filter gradient, every channel count of the tail and head kernels, one
    to three upsamplers, both dy forms, n below capacity and a cu_budget."""
    paths = [bo.launch_paths(c) for c in bo.CONFIGS]
    assert {p["twt"] for p in paths} == {64, 32}
    assert any(p["partial_segment"] for p in paths)
    assert {p["cc"] for p in paths} == {1, 2, 3, 4}
    assert {p["head_c"] for p in paths} == {1, 2, 3, 4}
    assert {p["nups"] for p in paths} == {1, 2, 3}
    assert {p["dy_form"] for p in paths} == {"rmse", "explicit"}
    assert any(p["below_capacity"] for p in paths)
    assert any(p["cu"] for p in paths)
    assert {(c[0], c[9]) for c in bo.CONFIGS} >= {("rcan", 2), ("edsr", 1), ("edsr", 2)}


@pytest.mark.parametrize("c", CASES)
def test_tail_dgrad_closes(c):
    """(a) DPS[nups - 1] = bf16(convT(dy, the fp32 tail filter)), dy explicit or (sr - hr) *
    loss4[2] formed in fp64 from the engine's fp32 sr, hr and loss4[2]."""
    _check("a", c)


@pytest.mark.parametrize("c", CASES)
def test_tail_filter_gradient_closes(c):
    """(b) tail.weight and tail.bias = the fp64 filter gradient of (PS[nups - 1], the same dy)."""
    _check("b", c)


@pytest.mark.parametrize("c", CASES)
def test_upsamplers_backward_closes(c):
    """(c) Every upsampler, last to first: its filter and bias gradient over (RESB | PS[k - 1],
    pixel_unshuffle(DPS[k])), its dgrad DPS[k - 1] or (k = 0) DRESF, and DRESB its rounding."""
    _check("c", c)


@pytest.mark.parametrize("c", CASES)
def test_body_tail_backward_closes(c):
    """(d) The body tail's filter and bias gradient over (HB(nl, 0), DRESB), BODY_GRAD 0 its
    fp32 dgrad and BODY_GRAD 1 the rounding of that stored map."""
    _check("d", c)


@pytest.mark.parametrize("c", CASES)
def test_head_filter_gradient_closes(c):
    """(e) head.weight and head.bias = the fp64 filter gradient of (lr, HEAD_GRAD)."""
    _check("e", c)
    if c[0] == "rcan":
        assert _run(c)[1]["head_grad_is_group_in_grad"]


@pytest.mark.parametrize("c", EDSR)
def test_edsr_block_backward_closes(c):
    """(f) nlayers 1: the ResBlock's whole backward with res_scale; nlayers 2: block 0's conv1
    filter gradient from the maps that survive the one-stage backward."""
    _check("f", c)


@pytest.mark.parametrize("c", EDSR1)
def test_edsr_forward_closes(c):
    """(g) EDSR at nlayers 1, the forward from saved maps, bf16_forward's class g bars."""
    _check("g", c)


def test_staged_reads_change_nothing():
    """The gradients (and sr) of the staged run with the reads between the stages equal those of
    one srmi_backward call, bit for bit (the case with n below capacity and the RMSE form)."""
    c = bo.CONFIGS[3]
    case, st, _ = _run(c)
    one = bo.engine_state(case, dev(), staged=False)
    assert torch.equal(one["sr"], st["sr"])
    assert torch.equal(one["grads"], st["grads"])


def test_accessors_refuse_what_the_engine_does_not_have():
    """One assertion per refused combination: the new ids on an inference engine, DPS outside
    0 .. nups - 1, BODY_GRAD's b outside 0 .. 1; and DPS is shaped as PS."""
    from srmi._lib import SrmiError
    from srmi.engine import Engine
    case = bo.make_case(*bo.CONFIGS[0])
    m = case["meta"]
    inf = Engine(case["spec"], 1, (m["h"], m["w"]), train=False, device=dev())
    for key in (("DPS", 0), ("DRESB",), ("BODY_GRAD", 0, 0), ("BODY_GRAD", 0, 1), ("HEAD_GRAD",)):
        with pytest.raises(SrmiError):
            inf.buffer(*key)
    eng = Engine(case["spec"], 1, (m["h"], m["w"]), train=True, device=dev())
    for key in (("DPS", -1), ("DPS", m["nups"]), ("BODY_GRAD", 0, -1), ("BODY_GRAD", 0, 2)):
        with pytest.raises(SrmiError):
            eng.buffer(*key)
    for k in range(m["nups"]):
        assert eng.buffer("DPS", k).shape == eng.buffer("PS", k).shape
        assert eng.buffer("DPS", k).dtype == torch.bfloat16
    assert eng.buffer("DRESB").shape == eng.buffer("DRESF").shape == eng.buffer("HEAD_GRAD").shape
    assert eng.buffer("BODY_GRAD", 0, 0).dtype == torch.float32 and eng.buffer("BODY_GRAD", 0, 1).dtype == torch.bfloat16
    assert eng.buffer("HEAD_GRAD").data_ptr() == eng.buffer("GROUP_IN_GRAD", 0).data_ptr()
