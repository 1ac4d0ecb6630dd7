"""The case tables and references of tests/test_gemm_exact_gpu.py, checked without a GPU: recipe() - pt_gemm_f16's own summation in torch
fp32 (K steps of 64, gemm_splits' ranges, the convolution gather by explicit indexing with the dox / doy / dimg carries of Stager::next,
csrc/gemm.hip:108-122) - must reproduce the fp64 weight gradient of every gathered case bit for bit, and the same recipe with a broken
carry must not: "the GPU test would fail if the kernel were subtly wrong" is itself tested here."""
import pytest
import torch

from tests import test_gemm_exact_gpu as G


def test_the_tables_reach_what_they_name():
    G.check_tables()


def test_ints_are_the_six_values_without_zeros():
    v = G.ints(4096, seed=1)
    assert v.dtype == torch.float16 and sorted(set(v.tolist())) == [-3.0, -2.0, -1.0, 1.0, 2.0, 3.0]
    counts = torch.bincount((v + 3).long(), minlength=7)
    assert all(550 < int(c) < 820 for i, c in enumerate(counts) if i != 3)      # 4096 / 6 = 683 each, +- 5 sigma


def test_fp16_rounding_of_the_reference_is_the_fp32_one():
    """(ref64 * alpha).half() is what the kernel's fp32 -> fp16 conversion gives: both round the same exact value once."""
    n = torch.arange(-60000, 60000, dtype=torch.float64)
    for alpha in (0.5, 0.25, 1.0):
        assert torch.equal((n * alpha).half(), (n.float() * alpha).half())


@pytest.mark.parametrize("case", G.GATHERED, ids=G.ids)
def test_the_kernels_recipe_gives_the_fp64_weight_gradient(case):
    x, dy, ref = G.gathered_problem(case)
    G.exact_precondition(ref, 1.0, False)
    geometry = G.gather_geometry(case)
    for splits in [1] + G.split_choices(case):
        got = G.recipe(x, dy, geometry, splits)
        assert got.dtype == torch.float32 and torch.equal(got.double(), ref), splits


def changes_the_walk(case, broken):
    """Whether a breakage of Stager::next changes which pixels a case reads.  The carry arithmetic runs only from the second K step of
    a split on, so K > GK (no split of the table is shorter than two steps).  "dox" (GK % (OW + 1) for GK % OW): the two remainders
    must differ - they are both 64 for OW > 64, both 4 for OW = 5, both 0 for OW = 1.  "carry" (the carry from ox into oy dropped): some
    lane must carry, which takes dox > 0 - a lane with ox = OW - 1, or ox >= 8 at OW = 72, then carries at the first step."""
    N, H, W, OH, OW, *_ = G.gather_geometry(case)
    if N * OH * OW <= G.GK:
        return False
    return G.GK % (OW + 1) != G.GK % OW if broken == "dox" else G.GK % OW != 0


def test_the_breakages_reach_every_case_that_steps():
    """Between them the two breakages change every case of more than one K step with OW != 1, every split case among them; the four
    one-step cases exercise Stager::start and the halo mask only."""
    steps = [c for c in G.GATHERED if G.gather_geometry(c)[0] * G.gather_geometry(c)[3] * G.gather_geometry(c)[4] > G.GK]
    assert len(G.GATHERED) - len(steps) == 4 and all(c in steps for c in G.GATHERED if c[7] is not None)
    for c in steps:
        assert changes_the_walk(c, "dox") or changes_the_walk(c, "carry") or G.gather_geometry(c)[4] == 1
    assert sum(changes_the_walk(c, "dox") for c in G.GATHERED) == 5 and sum(changes_the_walk(c, "carry") for c in G.GATHERED) == 6


@pytest.mark.parametrize("broken", ["dox", "carry"])
@pytest.mark.parametrize("case", G.GATHERED, ids=G.ids)
def test_the_reference_notices_a_broken_carry(case, broken):
    """Every case whose walk the breakage changes (changes_the_walk) must then differ from the fp64 reference, in every split count
    it runs with; where it changes nothing the recipe is still exact."""
    x, dy, ref = G.gathered_problem(case)
    geometry = G.gather_geometry(case)
    for splits in [1] + G.split_choices(case):
        got = G.recipe(x, dy, geometry, splits, broken=broken)
        assert torch.equal(got.double(), ref) != changes_the_walk(case, broken), splits
