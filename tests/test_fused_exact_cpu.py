"""tests/fused_exact.py, checked without a GPU: every table entry meets its preconditions (problem() asserts them: exact partial sums,
a saturated gate, |h| < 65504, |out| < 60000, pre_res an fp16 integer, no y zero by cancellation, the fp32 LayerNorm emulations of both
kernels - as they are and perturbed by +-2^-15 - rounding to the expected fp16); the tables reach the code they name; the index models
agree with vec_index of igemm_tail.h and with the prologue's expression, written out again here; pt_gelu_erf's formula gives max(g, 0)
for every gate value that occurs; and the CPU models of both kernels reproduce the references, while every planted fault changes at
least one output of the case that names it: "the GPU test would fail if the kernel were subtly wrong" is itself tested here."""
import numpy as np
import pytest
import torch

from tests import fused_exact as E
from tests.test_igemm_exact_cpu import gelu_erf_f32

name_of = lambda c: c.name


# ------------------------------------------------------------------------------------------------- preconditions and tables
@pytest.mark.parametrize("c", E.FF_CASES, ids=name_of)
def test_feed_forward_preconditions(c):
    pr = E.ff_problem(c)
    assert pr["out"].shape == (c.M, E.C) and pr["out"].dtype == torch.float16 and bool(torch.isfinite(pr["out"].float()).all())
    if c.pre:
        assert sorted(set(pr["gamma"].tolist())) == [-4.0, 4.0] and set(pr["beta"].tolist()) == {-1.0, 0.0, 1.0}
        assert float(pr["pre_res"].float().abs().max()) > 64         # the projection is worth something against the pattern it leaves
    if c.vec == 2 or c.pre_vec == 2:                              # the index wraps
        m = np.arange(c.M)
        assert int(((m // E.V2[0]) * E.V2[1] + m % E.V2[1]).max()) >= E.V2[2]
    if c.vec == 1 or c.pre_vec == 1:
        assert c.M > E.VG and 128 % E.VG and 16 % E.VG


@pytest.mark.parametrize("c", E.LL_CASES, ids=name_of)
def test_ln_linear_preconditions(c):
    pr = E.ll_problem(c)
    assert pr["out"].shape == (c.M, c.N) and bool(torch.isfinite(pr["out"].float()).all())
    if c.M >= 128:                                                # 16-row fragments: all near, all far, exactly one far row, and everything mixed
        far = pr["far"][:c.M // 16 * 16].view(-1, 16).sum(1).tolist()
        flat = (pr["kind"] >= E.ZERO)[:c.M // 16 * 16].view(-1, 16).sum(1).tolist()
        assert {0, 1, 16} <= set(far) and any(0 < f < 16 and z for f, z in zip(far, flat))
        assert int((pr["kind"] == E.CONST).sum()) > 0 and int((pr["kind"] == E.ZERO).sum()) > 0
        a, cc, live = pr["a"], pr["c"].abs(), pr["kind"] < E.ZERO
        assert bool((cc[live & ~pr["far"]] < 8 * a[live & ~pr["far"]]).all())
        f = live & pr["far"]
        assert bool(((cc[f] >= 9 * a[f]) & (cc[f] <= 100 * a[f]) & (cc[f] + a[f] <= 2048)).all())


def test_the_tables_reach_what_they_name():
    ff, ll = E.FF_CASES, E.LL_CASES
    plain = [c for c in ff if not c.pre]
    assert {c.M for c in plain if c.inner == 64} >= {1, 17, 128, 129, 300, 1157}
    assert {c.inner // 64 for c in plain if c.M == 300} >= {1, 2, 3, 20}
    assert {(c.res, c.vec, c.blend) for c in plain} >= {(False, 0, False), (True, 0, False), (True, 1, False), (True, 2, False), (True, 0, True), (False, 1, True)}
    assert any(not c.b1 for c in plain) and any(not c.b2 for c in plain) and any(c.kpad2_extra for c in plain)
    pre = [c for c in ff if c.pre]
    assert {c.M for c in pre if c.inner == 64} >= {1, 17, 129, 300} and {c.inner for c in pre if c.M == 300} >= {64, 192, 1280}
    assert {c.pre_vec for c in pre} == {0, 1, 2, 3} and any(not c.pre_b for c in pre) and {c.blend for c in pre} == {False, True}
    assert any(c.vec == 1 and c.pre_vec for c in pre) and not any(c.res for c in pre)
    assert {-(-c.N // 128) for c in ll if c.M == 300} >= set(range(1, 9)) and {c.N for c in ll if c.M == 300} >= {8, 72, 1000}
    assert {c.M for c in ll if c.N == 960} >= {1, 17, 128, 129} and any(c.M == 1157 and c.N == 128 for c in ll)
    assert {c.cs_cols for c in ll} >= {0, 64, 320, 960} and {c.cs_scale for c in ll if c.cs_cols} == {0.25, 4.0}
    assert any(c.xpad != 8 for c in ll) and any(c.lead for c in ll)
    lds = {E.C + E.PAD[k] for k in ("x", "out", "res", "blend")}
    assert len(lds) == 4
    assert sum(E.ff_problem(c)["rounded"] for c in ff) > 1000 and all(E.ff_problem(c)["rounded"] for c in plain if c.M >= 128)


# ------------------------------------------------------------------------------------------------- index models
def kernel_vec_index(mode, m, vG, vFS, vS, vB):
    """vec_index / vec_index_clip of igemm_tail.h:94-104 and the prologue's expression (ffn.hip:136-142), one row at a time in integer
    arithmetic, with what the host hands over: mode 3 gets vB / vG (the table's rows per clip), mode 2 runs the shared expression with
    vG = 1."""
    if mode == 1:
        return m // vG
    if mode == 2:
        tail = ((m // vFS) * vS + m % vS) % vB
        vG = 1
    else:
        vB = vB // vG
    b = m // vFS
    h = b // vG
    vi = ((h * vS + m % vS) % vB) * vG + (b - h * vG)
    assert mode == 3 or vi == tail
    return vi


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_the_row_vector_index(mode):
    M = 1157
    prm = {1: (E.VG, 0, 0, 0), 2: (0,) + E.V2, 3: E.V3}[mode]
    want = [kernel_vec_index(mode, m, *prm) for m in range(M)]
    assert E.vec_rows(mode, M).tolist() == want
    m = E.vec_boundary(mode, 300)
    assert want[m] != want[m + 1]
    if mode == 3:                                                 # a clip reads its own rows only: row half * vG + clip
        vG, vFS = E.V3[0], E.V3[1]
        assert all(want[m] % vG == (m // vFS) % vG for m in range(M)) and set(want[:300]) == set(range(E.V3[3]))


# ------------------------------------------------------------------------------------------------- the saturated gate
def test_gelu_is_saturated_at_every_gate_value_that_occurs():
    """As tests/test_igemm_exact_cpu.py: the formula of pt_gelu_erf gives g exactly for g > 0 and for g < 0 a value in (-2^-50 |g|, 0]
    whose product with any |value| < 2^24 rounds to a signed zero in fp16 - so fp16(val * gelu(g)) is fp16(val * max(g, 0)) up to that sign."""
    gates = np.unique(np.concatenate([E.ff_problem(c)["gate"].numpy().ravel() for c in E.FF_CASES] + [np.array([8.0, -8.0])]))
    assert np.abs(gates).min() == 8 and np.all(gates % 16 == 8)
    y, qz = gelu_erf_f32(gates)
    assert qz[np.abs(gates) == 8].min() > 52 and np.all(np.diff(qz[gates > 0]) > 0)
    pos = gates > 0
    assert np.array_equal(y[pos], gates[pos].astype(np.float32))
    neg = y[~pos]
    assert np.all(neg <= 0) and np.all(-neg < np.abs(gates[~pos]) * 2.0 ** -50)
    assert np.all((neg.astype(np.float64) * 2.0 ** 24).astype(np.float16) == 0)
    c = E.CASES["ff_m300_res"]
    pr = E.ff_problem(c)
    h = (pr["val"].numpy().astype(np.float32) * gelu_erf_f32(pr["gate"].numpy())[0]).astype(np.float16)
    want = (pr["val"] * pr["gate"].clamp(min=0)).half()
    assert torch.equal(E.positive_zero(torch.from_numpy(h)), E.positive_zero(want))


# ------------------------------------------------------------------------------------------------- the emulations notice what they should
def test_the_emulations_reject_a_cancelling_beta():
    """gamma = +-2 with beta = -+1 on a skewed row: n gamma + beta = 0 exactly, and the fp32 LayerNorm leaves a non-zero subnormal."""
    kind, a, c = torch.tensor([E.SKEW_HI]), torch.tensor([4]), torch.tensor([10])
    x, n = E.pattern(kind, a, c, 1)
    gamma, beta = torch.full((E.C,), -2.0, dtype=torch.float64), torch.full((E.C,), -1.0, dtype=torch.float64)
    with pytest.raises(AssertionError):
        E.expected_y(x, n, gamma, beta)
    y = (n * gamma + beta).numpy().astype(np.float16)
    assert int((y == 0).sum()) == 256
    for got in (E.ln_ffn_f32(x.numpy(), gamma.numpy(), beta.numpy()), E.ln_lnlin_f32(x.half().numpy(), gamma.numpy(), beta.numpy())[0]):
        assert not np.array_equal(got, y)


# ------------------------------------------------------------------------------------------------- models and planted faults
@pytest.mark.parametrize("c", E.FF_CASES, ids=name_of)
def test_the_feed_forward_model_is_the_reference(c):
    assert E.differing(E.ff_model(c), E.ff_images(c)[1]) == (0, -1)


@pytest.mark.parametrize("c", E.LL_CASES, ids=name_of)
def test_the_ln_linear_model_is_the_reference(c):
    assert E.differing(E.ll_model(c), E.ll_images(c)[1]) == (0, -1)


FF_PLANTED = [("wo_ktile", "pre_m300"), ("wo_ktile", "pre_m1"), ("w1_ktile", "ff_m300_res"), ("w1_ktile", "pre_inner192"), ("w2_ktile", "ff_inner192"),
              ("w2_ktile", "ff_inner1280"), ("w2_ktile", "pre_inner1280"), ("w2_ktile", "ff_kpad2"),
              ("pre_vec_neighbour", "pre_vec1"), ("pre_vec_neighbour", "pre_vec2"), ("pre_vec_neighbour", "pre_vec3"), ("pre_vec_neighbour", "pre_m129"),
              ("vec_neighbour", "ff_m300_res_vec1"), ("vec_neighbour", "ff_m300_res_vec2"), ("vec_neighbour", "ff_m129"), ("vec_neighbour", "pre_vec2_tail_vec1"),
              ("clamped_row", "ff_m1"), ("clamped_row", "ff_m17"), ("clamped_row", "ff_m129"), ("clamped_row", "pre_m1"), ("clamped_row", "pre_m17"),
              ("half_swap", "pre_m300"), ("mean_kept", "pre_m300"), ("mean_kept", "pre_m17"), ("beta_dropped", "pre_m300"), ("beta_dropped", "pre_m1"),
              ("h_unrounded", "ff_m300_res"), ("h_unrounded", "ff_inner1280"), ("h_unrounded", "pre_inner1280")]
LL_PLANTED = [("w_ktile", "ll_n8"), ("w_ktile", "ll_n960"), ("clamped_row", "ll_m1"), ("clamped_row", "ll_m17"), ("clamped_row", "ll_m129"),
              ("other_row_stats", "ll_n128"), ("mean_kept", "ll_n128"), ("mean_kept", "ll_m17"), ("far_one_pass", "ll_n128"), ("far_one_pass", "ll_m1157"),
              ("cs_chunk", "ll_cs64"), ("cs_chunk", "ll_cs320"), ("cs_chunk", "ll_n72"), ("swap16", "ll_n72"), ("swap16", "ll_out_block"),
              ("beta_dropped", "ll_n128"), ("beta_dropped", "ll_m1")]


def test_every_fault_is_planted():
    assert {f for f, _ in FF_PLANTED} == set(E.FF_FAULTS) and {f for f, _ in LL_PLANTED} == set(E.LL_FAULTS)


@pytest.mark.parametrize("fault,name", FF_PLANTED)
def test_a_planted_fault_changes_the_feed_forward_case_that_names_it(fault, name):
    c = E.CASES[name]
    bad, _ = E.differing(E.ff_model(c, fault), E.ff_images(c)[1], relax_zero=True)
    assert bad > 0


@pytest.mark.parametrize("fault,name", LL_PLANTED)
def test_a_planted_fault_changes_the_ln_linear_case_that_names_it(fault, name):
    c = E.CASES[name]
    bad, _ = E.differing(E.ll_model(c, fault), E.ll_images(c)[1])
    assert bad > 0
