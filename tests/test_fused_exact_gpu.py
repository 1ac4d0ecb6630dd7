"""pt_ffn_geglu_f16 (csrc/ffn.hip, plain and with its pre= prologue) and pt_ln_linear_f16 (csrc/lnlin.hip) on the MI355X against fp64,
BIT FOR BIT.  The argument, the case tables, the references and their asserted preconditions are tests/fused_exact.py's (checked on
the CPU, planted faults included, by tests/test_fused_exact_cpu.py): integer GEMM operands, a saturated GEGLU gate, LayerNorm rows whose
normalised values are exactly {+-1, +-2, +-1/2, 0} so that fp16(y) is a known small integer although the kernels' statistics are
fp32.  There is no tolerance anywhere.

Calls go through the raw bindings (hip.FfnParams, hip.LnLinParams, hip.lib()): the pitches under test are the ones the kernel sees.
Every pointer lives in a NaN-filled guarded buffer (guarded() of tests/test_gemm_exact_gpu.py): a pitch pad of 8 (x: 16, residual:
24, blend: 32 - all pitches differ), 64 NaN rows in front and behind - the whole packed weight images, the biases and gamma / beta
included (the guard rows of a vector have its own length).  `out` starts NaN-filled; afterwards every element outside [M, N] must still
be that NaN and every element inside bit-equal to the reference, so a NaN in the output is a read outside an operand, or past a pitch.
The one relaxation: -0 is +0 in the feed-forward cases (the saturated GELU returns a negative zero-sized value for a negative gate).

Section D is the one test on generic N(0, 1) data: both kernels' statistics and MFMA dot products are per row, in an order that does
not depend on the row's position, so a launch on row-permuted inputs must give the row-permuted output bit for bit, and a launch of
every single row (M = 1: the row replicated through a whole fragment) that row.

One line per run is printed: case, variant, number of differing elements, and the file's time at the end; with PT_FUSED_EXACT=<file>
the lines are also appended to that file (profiles/r20/fused_exact.txt is such a run)."""
import ctypes
import time

import pytest
import torch

from tests import fused_exact as E
from tests.test_gemm_exact_gpu import NAN, bits

pytestmark = pytest.mark.gpu

TALLY = dict(runs=0, exact=0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from posetraj_amd import ops
    d = torch.device("cuda:0")
    ops.ensure_ready(d)
    TALLY.update(runs=0, exact=0)
    t0 = time.perf_counter()
    yield d
    torch.cuda.synchronize()
    E.report(f"total: {TALLY['runs']} runs, {TALLY['exact']} bit-exact, {time.perf_counter() - t0:.1f} s for this file (references on the CPU included)")


def launch(entry, p):
    from posetraj_amd import hip
    L = hip.lib()
    rc = getattr(L, entry)(ctypes.byref(p), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.pt_last_error().decode()


def run(dev, c):
    """One launch of a case -> (elements of out's whole buffer - guard and pad included - whose bits differ from the reference image, the
    first such index as (row, column) relative to out[0, 0])."""
    ff = isinstance(c, E.FF)
    im, want = (E.ff_images if ff else E.ll_images)(c)
    d = {k: v[0].to(dev) for k, v in im.items()}
    base = {k: t.data_ptr() for k, t in d.items()}
    assert all(b % 256 == 0 for b in base.values()) and all((2 * v[1]) % 16 == 0 for v in im.values())
    launch("pt_ffn_geglu_f16" if ff else "pt_ln_linear_f16", (E.ff_params if ff else E.ll_params)(c, im, base))
    torch.cuda.synchronize()
    bad, first = E.differing(d["out"].cpu(), want, relax_zero=ff)
    for k, v in im.items():                                       # no operand was written
        assert k == "out" or bool((bits(d[k].cpu()) == bits(v[0])).all()), k
    _, off, ld = im["out"]
    return bad, ((first - off) // ld, (first - off) % ld)


def check(dev, c):
    bad, at = run(dev, c)
    TALLY["runs"] += 1
    TALLY["exact"] += int(bad == 0)
    E.report(f"{c.name} M={c.M} {'inner=' + str(c.inner) + ' ' if isinstance(c, E.FF) else ''}{c.variant}: {bad} elements differ")
    assert bad == 0, at


# ------------------------------------------------------------------------------------------------- A. the plain feed-forward
@pytest.mark.parametrize("c", E.FF_PLAIN, ids=lambda c: c.name)
def test_feed_forward(dev, c):
    check(dev, c)


# ------------------------------------------------------------------------------------------------- B. with the prologue
@pytest.mark.parametrize("c", E.FF_PRE, ids=lambda c: c.name)
def test_feed_forward_with_prologue(dev, c):
    check(dev, c)


# ------------------------------------------------------------------------------------------------- C. LayerNorm + linear layer
@pytest.mark.parametrize("c", E.LL_CASES, ids=lambda c: c.name)
def test_ln_linear(dev, c):
    check(dev, c)


def test_ln_linear_ablations_are_reported(dev):
    """The checker notices what it should: with the kernel's own tuning ablations (pt_ln_linear_set_ablation; restored whatever happens)
    bit 1, no output stores, leaves the whole inside of `out` NaN and every element of it is counted; bit 4, no MFMAs, writes zeros and
    every non-zero element of the reference is counted.  The guard stays NaN in both."""
    from posetraj_amd import hip
    L = hip.lib()
    c = E.CASES["ll_n1000"]
    want = E.ll_problem(c)["out"]
    for ablation, expect in ((1, c.M * c.N), (4, int((want != 0).sum()))):
        try:
            assert L.pt_ln_linear_set_ablation(ablation) == 0
            bad, _ = run(dev, c)
        finally:
            L.pt_ln_linear_set_ablation(0)
        E.report(f"{c.name} M={c.M} {c.variant} ablation={ablation}: {bad} elements differ (must be {expect})")
        assert bad == expect and expect > c.M * c.N // 2


# ------------------------------------------------------------------------------------------------- D. row locality on generic data
def locality(dev, name, entry, params, row_inputs, M, N):
    """``params(inputs, out, M)`` -> the call's parameters for row tensors ``inputs`` ([rows, 320] each, contiguous); the launch on
    permuted rows and the launches of every single row against the launch on all rows."""
    def go(inputs, rows):
        out = torch.full((rows, N), NAN, dtype=torch.float16, device=dev)
        launch(entry, params(inputs, out, rows))
        return out
    full = go(row_inputs, M)
    assert bool(torch.isfinite(full.float()).all())
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(5)).to(dev)
    permuted = go([t[perm].contiguous() for t in row_inputs], M)
    single = torch.full((M, N), NAN, dtype=torch.float16, device=dev)
    for m in range(M):
        launch(entry, params([t[m:m + 1] for t in row_inputs], single[m:m + 1], 1))
    torch.cuda.synchronize()
    for what, got, want in (("row-permuted inputs", permuted, full[perm]), ("every row alone (M = 1)", single, full)):
        bad = int((bits(got.cpu()) != bits(want.cpu())).sum())
        TALLY["runs"] += 1
        TALLY["exact"] += int(bad == 0)
        E.report(f"{name} M={M} N(0,1) data, {what}: {bad} elements differ")
        assert bad == 0, what


def normal(dev, *shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).half().to(dev)


def test_row_locality_feed_forward_with_prologue(dev):
    from posetraj_amd import hip, packing
    M, I = 300, 1280
    att, res = normal(dev, M, E.C, seed=1), normal(dev, M, E.C, seed=2)
    gamma, beta = 1.0 + normal(dev, E.C, seed=3, scale=0.1), normal(dev, E.C, seed=4, scale=0.1)
    po = packing.pack_linear(normal(dev, E.C, E.C, seed=5, scale=E.C ** -0.5), normal(dev, E.C, seed=6, scale=0.1), dev)
    p1 = packing.pack_linear(normal(dev, 2 * I, E.C, seed=7, scale=E.C ** -0.5), normal(dev, 2 * I, seed=8, scale=0.1), dev, geglu=True)
    p2 = packing.pack_linear(normal(dev, E.C, I, seed=9, scale=I ** -0.5), normal(dev, E.C, seed=10, scale=0.1), dev)

    def params(inputs, out, rows):
        p = hip.FfnParams()
        p.x, p.ldx, p.M, p.C, p.inner = inputs[0].data_ptr(), E.C, rows, E.C, I
        p.w1, p.b1, p.kpad1, p.w2, p.b2, p.kpad2 = p1.w.data_ptr(), p1.bias.data_ptr(), E.C, p2.w.data_ptr(), p2.bias.data_ptr(), I
        p.out, p.ldo = out.data_ptr(), E.C
        p.pre_w, p.pre_b, p.pre_kpad, p.pre_res, p.pre_ldr = po.w.data_ptr(), po.bias.data_ptr(), E.C, inputs[1].data_ptr(), E.C
        p.ln_gamma, p.ln_beta, p.ln_eps = gamma.data_ptr(), beta.data_ptr(), E.EPS
        return p
    locality(dev, "pre= feed-forward", "pt_ffn_geglu_f16", params, [att, res], M, E.C)


def test_row_locality_ln_linear(dev):
    from posetraj_amd import hip, packing
    M, N = 300, 384
    x = normal(dev, M, E.C, seed=11)
    gamma, beta = 1.0 + normal(dev, E.C, seed=12, scale=0.1), normal(dev, E.C, seed=13, scale=0.1)
    pw = packing.pack_linear(normal(dev, N, E.C, seed=14, scale=E.C ** -0.5), None, dev)

    def params(inputs, out, rows):
        p = hip.LnLinParams()
        p.x, p.ldx, p.M, p.N, p.K = inputs[0].data_ptr(), E.C, rows, N, E.C
        p.w, p.kpad, p.bias = pw.w.data_ptr(), E.C, None
        p.ln_gamma, p.ln_beta, p.ln_eps = gamma.data_ptr(), beta.data_ptr(), E.EPS
        p.out, p.ldo, p.cs_cols, p.cs_scale = out.data_ptr(), N, 64, 0.1767766952966369
        return p
    locality(dev, "pt_ln_linear_f16", "pt_ln_linear_f16", params, [x], M, N)
