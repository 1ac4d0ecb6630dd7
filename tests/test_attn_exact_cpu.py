"""CPU-only half of the exact-data attention tests (tests/attn_exact.py, tests/test_attn_exact_gpu.py): every case of the GPU lists
meets its family's preconditions, a plain CPU model of the kernels' rounding points passes the checkers under a running and under a
deferred maximum, and the checkers reject every planted fault that the module's table claims - the evidence that the GPU tests would
fail on a subtly wrong kernel."""
import math

import numpy as np
import pytest
import torch

from tests import attn_exact as X

CASES = X.all_cases()
IDS = [c.id for c in CASES]


def test_the_case_lists_are_what_the_header_names():
    assert len(set(IDS)) == len(IDS)
    sp = [c for c in CASES if c.kernel == "spatial"]
    assert {c.Sq for c in sp if c.nqb == 3 and c.nb == 3} == set(X.SPATIAL_S) and {c.Sq for c in sp if c.nqb == 2} == {129, 449}
    assert {(c.pre, c.nqb) for c in sp if c.family == "C"} == {(0, 3), (1, 3), (0, 2), (1, 2)} and any(c.Sq == 705 for c in sp if c.family == "C")
    ge = [c for c in CASES if c.kernel == "general"]
    assert {c.D for c in ge} == {64, 80, 128} and {c.D for c in ge if c.lse} == {64, 128}
    assert {(c.Sq, c.Sk) for c in ge if not c.fused and c.family != "C"} == set(X.GENERAL_S)
    assert all({c.family for c in ge if c.lse and c.D == D} == {"A0", "Am", "B", "C"} for D in (64, 128))
    assert all(any(c.family == "C" and c.Sk == 289 and c.D == D for c in CASES) for D in (64, 80, 128, 512))
    te = [c for c in CASES if c.kernel == "temporal"]
    assert {c.Sk for c in te} == set(X.SHORT_F + X.LONG_F) and {c.groups for c in te} == {5, 18} and {c.family for c in te} == {"A0", "Am", "B"}
    assert {c.nb for c in CASES if c.kernel == "d512"} == {3, 9}
    assert max(c.Sk for c in CASES) <= 1024


def test_float32_ln2_times_log2e_is_one():
    """scale = float32(ln 2) makes the entry points' cexp = scale * 1.4426950408889634f exactly 1.0f: the product is 1 - 1.06e-8, inside
    half a float spacing below 1."""
    ln2 = np.float32(math.log(2.0))
    assert ln2 * np.float32(1.4426950408889634) == np.float32(1.0)
    assert abs(float(ln2) * float(np.float32(1.4426950408889634)) - 1.0) < 2.0 ** -25
    assert X.cexp_of(X.LN2_32) == 1.0


def test_ulp16():
    x = torch.tensor([1.0, 1.5, 2.0, 0.75, 2.0 ** -14, 2.0 ** -20, 0.0, -3.0], dtype=torch.float64)
    want = torch.tensor([2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -11, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -9], dtype=torch.float64)
    assert torch.equal(X.ulp16(x), want)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_generators_meet_their_preconditions(case):
    info = X.self_check(case)
    q, k, v = X.problem(case)
    assert q.shape == (case.groups, case.Sq, case.D) and k.shape == v.shape == (case.groups, case.Sk, case.D)
    if case.groups > 1:
        assert not torch.equal(v[0], v[1]), "every group has its own data"
    if case.family == "B" and case.kernel != "temporal" and case.Sk in (130, 449, 1024):
        assert info["margin"] >= 60                              # D = 64: 86 at 449 keys, 75 at 1024 with one group's seed


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_rounding_model_passes_the_checkers(case):
    """Under the kernel's own softmax bookkeeping and under the other one (the temporal kernels' single pass included)."""
    for softmax in ("online", "defer", "full"):
        o, lse, _ = X.emulate(case, softmax=softmax)
        v = X.judge(case, o, lse)
        assert v.ok, (softmax, v.text)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_planted_faults_are_rejected(case):
    """MUST_CATCH, the table of the module docstring: wherever a fault can be expressed at this case, the family that claims it rejects
    it."""
    for fault, families in X.MUST_CATCH.items():
        if case.family not in families:
            continue
        got = X.emulate(case, fault)
        if got is None:
            continue
        o, lse, _ = got
        assert not X.judge(case, o).ok, fault


def test_every_fault_is_claimed_at_every_shape_where_it_can_be_expressed():
    """For every kernel shape (a case without its family) and every fault: if any family can express the fault there, a family that must
    catch it can."""
    shapes = {}
    for c in CASES:
        shapes.setdefault((c.kernel, c.nb, c.heads, c.pos, c.Sq, c.Sk, c.D, c.nqb, c.fused), []).append(c)
    assert set(X.MUST_CATCH) == set(X.FAULTS)
    for key, cs in shapes.items():
        if not {"A0", "Am", "B"} <= {c.family for c in cs}:
            continue                                             # (a shape that only one family runs: 705, 1024, the 289-key C cases)
        for fault in X.FAULTS:
            able = [c for c in cs if X.emulate(c, fault) is not None]
            if able:
                assert any(c.family in X.MUST_CATCH[fault] for c in able), (key, fault)


def test_the_table_in_the_docstring_is_must_catch():
    rows = {}
    for line in X.__doc__.splitlines():
        w = line.split()
        if w and w[0] in X.FAULTS:
            rows[w[0]] = tuple(f for f, mark in zip(X.FAMILIES, w[1:5]) if mark == "x")
    assert rows == X.MUST_CATCH


def test_a_family_b_match_in_a_late_tile_moves_the_maximum():
    """The re-base paths are on the route of family B: at 449 keys every tile after the first moves some query's maximum, under both
    bookkeepings."""
    case = X.Case("spatial", "B", 3, 3, 449, 449, 64)
    for softmax, tiles in (("defer", 8), ("online", 15)):
        assert X.emulate(case, softmax=softmax)[2] == list(range(1, tiles))


def test_layout_round_trip():
    for case in (X.Case("temporal", "B", 2, 3, 17, 17, 64, pos=3), X.Case("general", "B", 3, 3, 5, 3, 80)):
        q, k, v = X.problem(case)
        rows = X.to_rows(case, v)
        assert torch.equal(X.from_rows(case, rows, case.Sk), v)
        if case.kernel == "temporal":                            # row = (clip F + frame) positions + position, column = head D + d
            assert torch.equal(rows[(1 * 17 + 4) * 3 + 2, 2 * 64:3 * 64], v[(1 * 3 + 2) * 3 + 2, 4])
        else:
            assert torch.equal(rows[2 * 3 + 1, 80:160], v[2 * 3 + 1, 1])
