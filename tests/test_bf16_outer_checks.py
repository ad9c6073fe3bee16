"""The checkers of tests/bf16_outer.py, fed from the reference side (no GPU): the fp64 restatement
of the engine's outer backward, rounded where the engine stores, sits inside every bar; and each
way a launch could be subtly wrong (bf16_outer.MUTATIONS), applied to the "engine" side, fails
the class that closes over that launch.  A mutated launch's output is consumed downstream as it
is, so the classes closing over other launches still pass."""
import functools

import pytest

import bf16_outer as bo

#          first, second, fourth and the EDSR nl = 1 case
SHAPES = [0, 1, 3, 7]


@functools.lru_cache(maxsize=None)
def _case(i):
    return bo.make_case(*bo.CONFIGS[i])


@functools.lru_cache(maxsize=None)
def _report(i, mut=0):
    return bo.check_all(bo.reference_state(_case(i), mut))


def _failed(rep):
    return {cls for cls in bo.CLASSES if rep.failures(cls)}


@pytest.mark.parametrize("i", SHAPES, ids=[bo.case_id(bo.CONFIGS[i]) for i in SHAPES])
def test_reference_sits_inside_every_bar(i):
    rep = _report(i)
    for cls in bo.classes_of(_case(i)):
        assert any(r[0] == cls for r in rep.rows), cls
    print("\n".join(bo.report_lines(rep, bo.classes_of(_case(i)))))
    assert not [r[:6] for r in rep.rows if not r[6]]


#   mutation, case, the classes that must fail (no other may)
MUTANTS = [
    (1, 0, {"a"}),
    (2, 1, {"b"}),
    (3, 0, {"a"}),
    (3, 1, {"a"}),
    (4, 0, {"a", "b"}),   # both tail kernels form dy
    (4, 3, {"a", "b"}),
    (5, 1, {"c"}),
    (6, 3, {"c"}),
    (7, 3, {"e"}),
    (8, 1, {"e"}),
    (8, 3, {"e"}),
    (9, 7, {"f"}),
    (10, 0, {"b"}),
    (10, 3, {"b"}),
    (10, 7, {"b"}),
]


@pytest.mark.parametrize("mut,i,classes", MUTANTS, ids=[f"m{m}-{bo.case_id(bo.CONFIGS[i])}" for m, i, _ in MUTANTS])
def test_mutation_fails_its_class(mut, i, classes):
    rep = _report(i, mut)
    failed = _failed(rep)
    print(bo.MUTATIONS[mut], "->", sorted(failed))
    for cls in sorted(failed):
        print("  ", rep.failures(cls)[:3])
    assert failed == classes


def test_cases_reach_every_launch_path():
    """From shapes alone (the GPU file asserts the same of the cases it runs)."""
    paths = [bo.launch_paths(c) for c in bo.CONFIGS]
    assert {p["twt"] for p in paths} == {64, 32}
    assert any(p["partial_segment"] for p in paths)
    assert {p["cc"] for p in paths} == {1, 2, 3, 4} == {p["head_c"] for p in paths}
    assert {p["nups"] for p in paths} == {1, 2, 3}
    assert {p["dy_form"] for p in paths} == {"rmse", "explicit"}
    assert any(p["below_capacity"] for p in paths) and any(p["cu"] for p in paths)
