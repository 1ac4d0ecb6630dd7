"""The attention backward kernels of the training step on the MI355X against fp64, with a CPU rounding model as the yardstick:
pt_attn_bwd_f16 (rowdot_kernel, attn_bwd_dq_kernel, attn_bwd_dkv_kernel), the lse of pt_attn_fwd_lse_f16 that it consumes, and the
one-block kernel of pt_attn_temporal_bwd_f16 (F <= 16; tests/test_temporal_bwd_long_gpu.py has the two-block one).

Reference: torch fp64 autograd of softmax(Q K^T / sqrt(d)) V on the CPU over the same fp16-representable inputs; ``rel`` is the
rel-L2 of tests/test_backward_gpu.py.

Bound, per block (dQ, dK, dV): rel(kernel, fp64) <= 1.25 * rel(model, fp64).  The model (spatial_model / temporal_model below) is
the same fp64 computation with a .half().double() at exactly the points where the kernel's source rounds to fp16 - every such
line names the source line it mirrors.  Only fp32 accumulation (1e-6 class) separates kernel and model; 1.25 is the project's
customary margin.  In the N(0, 1) regime the operator's 1.5e-3 over [dQ|dK|dV] is asserted too.  dq_dot and lse are checked per
element against bounds derived from the fp32 arithmetic that forms them (see the two tests).

Regimes: ``normal`` N(0, 1); ``peaked`` Q and K x 3 (mean max P 0.8, most dS below the fp16 normal range); ``small`` dO x 2^-10;
``offset`` K + 4.0 in every column (the exact dQ does not depend on it: the rows of dS sum to zero, rounding dS breaks that).  The
2^-10 of ``small`` is NOT a magnitude observed in a training run: it is the scale at which dS leaves the fp16 normal range at these
sizes (71 - 90 % subnormal), where the order of scaling and rounding dS would show.

Inputs travel in NaN-padded buffers: every padding column of every input holds NaN, 64 NaN rows follow the last row, NaN entries
follow lse, and the gradient buffer and dq_dot start as NaN - a masked key is multiplied by p = 0 and 0 * NaN is NaN, so a read
past Sq / Sk or a row that should have been staged as zeros reaches the output.

Every distance and ratio is printed; with PT_ATTN_BWD_PARITY=<file> it is also appended to that file (profiles/r09/
attn_bwd_parity.txt is such a run).  The recomputing path (autodiff._attention_backward) is printed beside each case for the
record only: it forms sum P dP without the stored O and is legitimately more accurate on peaked data."""
import functools
import math
import os
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

# (nbatch, S, heads, head_dim): streamed tiles are 32 rows, a workgroup holds 64 stationary rows
SPATIAL = [(2, 33, 1, 64),           # one full tile + a one-row tail; batch 1 lies directly behind batch 0: an unmasked key read lands in real data
           (1, 64, 2, 64),           # exact tiles, nothing masked
           (2, 65, 3, 64),           # second stationary block: one live row, three dead waves (the Sq - 1 clamp); 6 groups < 8: the grp >= ngroups return
           (3, 97, 3, 64),           # 9 groups > 8: the group index runs a second round
           (2, 50, 2, 128),          # head_dim 128
           (1, 97, 10, 128)]         # rowdot_kernel: 160 chunks per row = three trips of its lane loop, the last one partial
# (B, F, S, heads, head_dim)
TEMPORAL = [(1, 2, 5, 1, 64),        # 5 tasks: the last workgroup has one live wave
            (2, 14, 7, 2, 64),       # the workload's frame count; two clips adjacent in memory
            (1, 16, 4, 1, 64),       # a full block
            (2, 15, 3, 3, 128), (1, 9, 2, 2, 128)]
CHAINED = [(3, 97, 3, 64), (2, 50, 2, 128)]
REGIMES = ("normal", "peaked", "small", "offset")
BLOCKS = ("dQ", "dK", "dV")
MARGIN = 1.25
GUARD = 64                           # NaN rows behind every input and output, NaN entries behind lse and dq_dot
LOG2E = 1.4426950408889634
U = 2.0 ** -24                       # fp32 unit roundoff
NAN = float("nan")
ids = lambda c: "x".join(map(str, c))


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def report(line: str):
    print(line)
    path = os.environ.get("PT_ATTN_BWD_PARITY")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from posetraj_amd import ops
    d = torch.device("cuda:0")
    ops.ensure_ready(d)
    return d


@pytest.fixture(scope="module")
def AD():
    from posetraj_amd import autodiff
    return autodiff


def h16(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).half()


def inputs(rows, Cc, regime, seed):
    """(q, k, v, dO), [rows, C] fp16 each, of a regime."""
    q, k, v, dy = (h16(rows, Cc, seed=seed + i) for i in range(4))
    if regime == "peaked":
        q, k = (q.float() * 3).half(), (k.float() * 3).half()
    elif regime == "small":
        dy = (dy.float() * 2.0 ** -10).half()
    elif regime == "offset":
        k = (k.float() + 4.0).half()
    return q, k, v, dy


def r16(t):
    return t.half().double()


# ------------------------------------------------------------------------------------------------- the rounding models (CPU, fp64)
def spatial_model(q, k, v, do, o16, scale):
    """pt_attn_bwd_f16 in fp64 with the kernel's fp16 roundings; q, k, v, do, o16: [..., S, hd] fp64 (o16: the fp16 O the kernel is given)."""
    p = torch.softmax(q @ k.transpose(-1, -2) * scale, dim=-1)           # attn_bwd.hip:138 / :261  P = exp2(s c - L), fp32: unrounded
    dq_dot = (do * o16).sum(-1, keepdim=True)                            # :42   Dq = sum_d dO O over the stored fp16 O, fp32: unrounded
    dp = do @ v.transpose(-1, -2)                                        # :129 / :251  fp32 accumulators
    ds = r16(p * (dp - dq_dot))                                          # :139 / :263  dS to fp16, P unrounded inside
    p16 = r16(p)                                                         # :262  P to fp16 for dV
    dq = r16((ds @ k) * scale)                                           # :158  scaled after the sum, then fp16
    dk = r16((ds.transpose(-1, -2) @ q) * scale)                         # :286
    dv = r16(p16.transpose(-1, -2) @ do)                                 # :287
    return dq, dk, dv


def temporal_model(q, k, v, do, scale, scale_after_sum=False):
    """attn_temporal_bwd_kernel in fp64 with the kernel's fp16 roundings; [..., F, hd] fp64.  scale_after_sum: the SECOND model,
    which rounds dS and scales the sums like the spatial passes (printed for comparison, never asserted)."""
    p = torch.softmax(q @ k.transpose(-1, -2) * scale, dim=-1)           # attn_bwd.hip:356 / :378  fp32: unrounded
    dp = do @ v.transpose(-1, -2)                                        # :342 / :344
    dd = (p * dp).sum(-1, keepdim=True)                                  # :357-359 / :378-380  no stored O; fp32: unrounded
    p16 = r16(p)                                                         # :360  P to fp16 for dV
    if scale_after_sum:
        ds = r16(p * (dp - dd))
        dq, dk = r16((ds @ k) * scale), r16((ds.transpose(-1, -2) @ q) * scale)
    else:
        ds = r16(p * (dp - dd) * scale)                                  # :361 / :382  the scale goes in BEFORE the rounding
        dq, dk = r16(ds @ k), r16(ds.transpose(-1, -2) @ q)              # :401 / :402
    dv = r16(p16.transpose(-1, -2) @ do)                                 # :403
    return dq, dk, dv


# ------------------------------------------------------------------------------------------------- layouts
def spatial_heads(t, case):
    """[N S, C] -> [N, heads, S, hd]"""
    N, S, heads, hd = case
    return t.view(N, S, heads, hd).transpose(1, 2)


def spatial_rows(t, case):
    N, S, heads, hd = case
    return t.transpose(1, 2).reshape(N * S, heads * hd)


def temporal_heads(t, case):
    """[B F S, C] (row (b F + f) S + s) -> [B, S, heads, F, hd]"""
    B, Fr, S, heads, hd = case
    return t.view(B, Fr, S, heads, hd).permute(0, 2, 3, 1, 4)


def temporal_rows(t, case):
    B, Fr, S, heads, hd = case
    return t.permute(0, 3, 1, 2, 4).reshape(B * Fr * S, heads * hd)


def reference(q, k, v, dy, to_heads, to_rows, case):
    """fp64 autograd -> (out [rows, C], (dQ, dK, dV) [rows, C], scores [.., L, L])."""
    hd = case[-1]
    leaves = [t.double().requires_grad_(True) for t in (q, k, v)]
    qh, kh, vh = (to_heads(t, case) for t in leaves)
    s = qh @ kh.transpose(-1, -2) / math.sqrt(hd)
    y = to_rows(torch.softmax(s, dim=-1) @ vh, case)
    y.backward(dy.double())
    return y.detach(), tuple(t.grad.detach() for t in leaves), s.detach()


@functools.lru_cache(maxsize=None)
def spatial_problem(case, regime):
    """Inputs, fp64 reference and the reference's own O (fp16) and lse (log2 domain) of a spatial case; computed once, never modified."""
    N, S, heads, hd = case
    rows, Cc = N * S, heads * hd
    q, k, v, dy = inputs(rows, Cc, regime, seed=300 + S + hd)
    out, grads, s = reference(q, k, v, dy, spatial_heads, spatial_rows, case)
    lse2 = (LOG2E * torch.logsumexp(s, dim=-1)).transpose(1, 2).reshape(rows, heads)                   # [N, heads, S] -> [rows, heads]
    qk_abs = (spatial_heads(q.double(), case).abs() @ spatial_heads(k.double(), case).abs().transpose(-1, -2)).amax(-1)
    return SimpleNamespace(q=q, k=k, v=v, dy=dy, out=out, o16=out.half(), grads=grads, lse2=lse2,
                           qk_abs=qk_abs.transpose(1, 2).reshape(rows, heads))


@functools.lru_cache(maxsize=None)
def temporal_problem(case, regime):
    B, Fr, S, heads, hd = case
    rows, Cc = B * Fr * S, heads * hd
    q, k, v, dy = inputs(rows, Cc, regime, seed=400 + Fr + hd)
    _, grads, _ = reference(q, k, v, dy, temporal_heads, temporal_rows, case)
    return SimpleNamespace(q=q, k=k, v=v, dy=dy, grads=grads)


def run_model(model, pr, to_heads, to_rows, case, *extra, **kw):
    hs = [to_heads(t.double(), case) for t in (pr.q, pr.k, pr.v, pr.dy) + extra]
    return tuple(to_rows(t, case) for t in model(*hs, case[-1] ** -0.5, **kw))


@functools.lru_cache(maxsize=None)
def spatial_model_of_reference_o(case, regime):
    pr = spatial_problem(case, regime)
    return run_model(spatial_model, pr, spatial_heads, spatial_rows, case, pr.o16)


# ------------------------------------------------------------------------------------------------- device buffers
def guarded(t, ld, dev):
    """t's rows at pitch ld on the device with GUARD rows behind them; padding columns and guard rows hold NaN."""
    buf = torch.full((t.shape[0] + GUARD, ld), NAN, dtype=t.dtype, device=dev)
    buf[:t.shape[0], :t.shape[1]] = t.to(dev)
    return buf


def guarded_vec(t, dev):
    buf = torch.full((t.numel() + GUARD,), NAN, dtype=torch.float32, device=dev)
    buf[:t.numel()] = t.reshape(-1).float().to(dev)
    return buf


def stream():
    return torch.cuda.current_stream().cuda_stream


def spatial_operands(pr, Cc, pad, dev):
    """(buffers kept alive, (q ptr, ldq, k ptr, ldk, v ptr, ldv)): the tape's fused [Q|K|V] rows at ld = 3 C, or three buffers of three pitches."""
    if pad:
        bufs = [guarded(t, Cc + 8 * (i + 1), dev) for i, t in enumerate((pr.q, pr.k, pr.v))]
        return bufs, tuple(x for b in bufs for x in (b.data_ptr(), b.stride(0)))
    buf = guarded(torch.cat([pr.q, pr.k, pr.v], dim=1), 3 * Cc, dev)
    return [buf], tuple(x for i in range(3) for x in (buf.data_ptr() + 2 * i * Cc, 3 * Cc))


def spatial_backward(dev, case, regime, pad, o16, lse):
    """pt_attn_bwd_f16 through the raw binding on (o16 [rows, C] fp16, lse [rows, heads]) -> the whole NaN-initialised gradient buffer
    [rows + GUARD, ldd] and dq_dot [rows heads + GUARD], on the CPU."""
    from posetraj_amd import hip
    N, S, heads, hd = case
    rows, Cc = N * S, heads * hd
    pr = spatial_problem(case, regime)
    keep, qkv_args = spatial_operands(pr, Cc, pad, dev)
    ldout, ldo, ldd = (Cc + 8, Cc + 16, 3 * Cc + 4) if pad else (Cc, Cc, 3 * Cc)
    ob, dyb, lb = guarded(o16, ldout, dev), guarded(pr.dy, ldo, dev), guarded_vec(lse, dev)
    dot = torch.full((rows * heads + GUARD,), NAN, dtype=torch.float32, device=dev)
    g = torch.full((rows + GUARD, ldd), NAN, dtype=torch.float16, device=dev)
    g0 = g.data_ptr()
    rc = hip.lib().pt_attn_bwd_f16(*qkv_args, ob.data_ptr(), ldout, dyb.data_ptr(), ldo, lb.data_ptr(), dot.data_ptr(), g0, g0 + 2 * Cc, g0 + 4 * Cc, ldd,
                                   N, S, heads, hd, hd ** -0.5, stream())
    assert rc == 0, hip.lib().pt_last_error().decode()
    torch.cuda.synchronize()
    del keep
    return g.cpu(), dot.cpu()


_runs = {}


def spatial_backward_alone(dev, case, regime, pad):
    """The backward on the REFERENCE's O and lse (isolated from the forward kernel); one launch per (case, regime, pad)."""
    key = (case, regime, pad)
    if key not in _runs:
        pr = spatial_problem(case, regime)
        _runs[key] = spatial_backward(dev, case, regime, pad, pr.o16, pr.lse2)
    return _runs[key]


def spatial_forward(dev, case, regime):
    """pt_attn_fwd_lse_f16 as the tape calls it (fused rows, tight pitches) -> NaN-initialised (out [rows + GUARD, C], lse [rows heads + GUARD])."""
    key = ("fwd", case, regime)
    if key not in _runs:
        from posetraj_amd import hip
        N, S, heads, hd = case
        rows, Cc = N * S, heads * hd
        keep, qkv_args = spatial_operands(spatial_problem(case, regime), Cc, False, dev)
        out = torch.full((rows + GUARD, Cc), NAN, dtype=torch.float16, device=dev)
        lse = torch.full((rows * heads + GUARD,), NAN, dtype=torch.float32, device=dev)
        rc = hip.lib().pt_attn_fwd_lse_f16(*qkv_args, out.data_ptr(), Cc, N, S, S, heads, hd, hd ** -0.5, lse.data_ptr(), stream())
        assert rc == 0, hip.lib().pt_last_error().decode()
        torch.cuda.synchronize()
        del keep
        _runs[key] = (out.cpu(), lse.cpu())
    return _runs[key]


def temporal_backward(dev, case, regime, pad):
    """pt_attn_temporal_bwd_f16 at the pitches of test_temporal_bwd_long_gpu.run_kernel -> the whole gradient buffer [rows + GUARD, ldd]."""
    from posetraj_amd import hip
    B, Fr, S, heads, hd = case
    Cc = heads * hd
    pr = temporal_problem(case, regime)
    ld, ldo, ldd = (3 * Cc + 8, Cc + 8, 3 * Cc + 4) if pad else (3 * Cc, Cc, 3 * Cc)
    a, b = guarded(torch.cat([pr.q, pr.k, pr.v], dim=1), ld, dev), guarded(pr.dy, ldo, dev)
    g = torch.full((a.shape[0], ldd), NAN, dtype=torch.float16, device=dev)
    rc = hip.lib().pt_attn_temporal_bwd_f16(a.data_ptr(), ld, Cc, 2 * Cc, b.data_ptr(), ldo, g.data_ptr(), ldd, B, Fr, S, heads, hd, hd ** -0.5, stream())
    assert rc == 0, hip.lib().pt_last_error().decode()
    torch.cuda.synchronize()
    return g.cpu()


def recompute(AD, dev, kind, case, regime):
    """Distances to fp64, per block, of the recomputing path on the case's tight-pitch inputs (printed, never asserted)."""
    key = ("recompute", kind, case, regime)
    if key not in _runs:
        heads, hd = case[-2:]
        Cc = heads * hd
        if kind == "spatial":
            pr, (N, S) = spatial_problem(case, regime), case[:2]
            geom = (S, 1, (N, S, 1, 0), N)
        else:
            pr, (B, Fr, S) = temporal_problem(case, regime), case[:3]
            geom = (Fr, S, (B, Fr * S, S, 1), 1)
        got = AD._attention_backward(torch.cat([pr.q, pr.k, pr.v], dim=1).to(dev), pr.dy.to(dev), Cc, heads, hd, *geom).cpu()
        _runs[key] = [rel(got[:, i * Cc:(i + 1) * Cc], pr.grads[i]) for i in range(3)]
    return _runs[key]


def written_and_untouched(g, rows, Cc):
    """Every [dQ|dK|dV] element is written with a finite value; padding columns and guard rows are still NaN."""
    assert bool(torch.isfinite(g[:rows, :3 * Cc]).all()), "every [dQ|dK|dV] column of every row is written and finite"
    assert bool(torch.isnan(g[:rows, 3 * Cc:]).all()), "padding columns are not touched"
    assert bool(torch.isnan(g[rows:]).all()), "rows behind the last one are not touched"


def check_blocks(label, case, regime, g, want, model, rec, second=None):
    """Prints, then asserts, the per-block bound of the header (and the operator's 1.5e-3 in the N(0, 1) regime)."""
    Cc = case[-2] * case[-1]
    rows = want[0].shape[0]
    got = [g[:rows, i * Cc:(i + 1) * Cc] for i in range(3)]
    kd, md = [rel(a, b) for a, b in zip(got, want)], [rel(a, b) for a, b in zip(model, want)]
    total = rel(g[:rows, :3 * Cc], torch.cat(want, dim=1))
    sd = [rel(a, b) for a, b in zip(second, want)] if second is not None else None
    report(f"{label} {case} {regime}: dqkv {total:.3e}; " + "; ".join(
        f"{n} kernel {a:.3e} model {b:.3e} ratio {a / b:.3f}" + (f" scale-after-sum model {sd[i]:.3e} ratio {a / sd[i]:.3f}" if sd else "") +
        f" recompute {rec[i]:.3e}" for i, (n, a, b) in enumerate(zip(BLOCKS, kd, md))))
    if regime == "normal":
        assert total <= 1.5e-3
    for n, a, b in zip(BLOCKS, kd, md):
        assert a <= MARGIN * b, (n, a, b, a / b)


cases = lambda c: pytest.mark.parametrize("case", c, ids=ids)
regimes = pytest.mark.parametrize("regime", REGIMES)
pads = pytest.mark.parametrize("pad", [False, True], ids=["tight", "padded"])


# ------------------------------------------------------------------------------------------------- 1. spatial backward alone
@regimes
@pads
@cases(SPATIAL)
def test_spatial_backward_alone_against_fp64(dev, AD, case, pad, regime):
    """pt_attn_bwd_f16 fed the reference's O (fp16) and lse: tight = the tape's fused rows at ld = 3 C; padded = q, k, v in three
    buffers of pitches C + 8 / 16 / 24, ldout = C + 8, ldo = C + 16, dq / dk / dv column blocks of one buffer at ldd = 3 C + 4."""
    N, S, heads, hd = case
    pr = spatial_problem(case, regime)
    g, _ = spatial_backward_alone(dev, case, regime, pad)
    written_and_untouched(g, N * S, heads * hd)
    check_blocks("spatial alone, " + ("padded" if pad else "tight"), case, regime, g, pr.grads, spatial_model_of_reference_o(case, regime),
                 recompute(AD, dev, "spatial", case, regime))


# ------------------------------------------------------------------------------------------------- 2. dq_dot
@regimes
@pads
@cases(SPATIAL)
def test_dq_dot_per_element(dev, case, pad, regime):
    """rowdot_kernel's output of the same calls: |dq_dot - sum_d dO O| <= 2 D 2^-24 sum_d |dO| |O| per element - the worst case of an
    fp32 dot product of D exact fp16 x fp16 products (D - 1 additions, each within 2^-24 relative), doubled; reference in fp64 over
    the fp16 O that was passed in."""
    N, S, heads, hd = case
    rows = N * S
    pr = spatial_problem(case, regime)
    _, dot = spatial_backward_alone(dev, case, regime, pad)
    assert bool(torch.isnan(dot[rows * heads:]).all()), "entries behind the last row are not touched"
    prod = (pr.dy.double() * pr.o16.double()).view(rows, heads, hd)
    want, bound = prod.sum(-1), 2 * hd * U * prod.abs().sum(-1)
    err = (dot[:rows * heads].double().view(rows, heads) - want).abs()
    assert bool(torch.isfinite(err).all())
    report(f"dq_dot {case} {regime} {'padded' if pad else 'tight'}: worst |error| / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


# ------------------------------------------------------------------------------------------------- 3. lse and out of the forward
@regimes
@cases(SPATIAL)
def test_forward_lse_per_element(dev, case, regime):
    """lse of pt_attn_fwd_lse_f16 against ref2 = log2 e * logsumexp(scale s) in fp64, per element, u = 2^-24:
    |lse - ref2| <= 2 D u cexp max_k sum_d |q_d| |k_d|  (the fp32 score dot product, in log2 units: an error of every score by at most e
                                                         moves the log-sum-exp by at most e)
                  + (Sk + 8) u / ln 2                    (the fp32 sum of Sk exponentials + exp2 and log2, relative, hence / ln 2 in log2 units)
                  + 4 u |ref2|                           (m_run + log2(l) and its operands in fp32)."""
    N, S, heads, hd = case
    rows = N * S
    pr = spatial_problem(case, regime)
    out, lse = spatial_forward(dev, case, regime)
    assert bool(torch.isnan(out[rows:]).all()) and bool(torch.isnan(lse[rows * heads:]).all()), "nothing behind the last row is written"
    got = lse[:rows * heads].double().view(rows, heads)
    assert bool(torch.isfinite(got).all())
    cexp = hd ** -0.5 * LOG2E
    bound = 2 * hd * U * cexp * pr.qk_abs + (S + 8) * U / math.log(2) + 4 * U * pr.lse2.abs()
    err = (got - pr.lse2).abs()
    d_out = rel(out[:rows], pr.out)
    report(f"forward {case} {regime}: out {d_out:.3e}; lse worst |error| {float(err.max()):.3e}, worst |error| / bound {float((err / bound).max()):.3f} "
           f"(bound {float(bound.min()):.2e} .. {float(bound.max()):.2e})")
    assert bool((err <= bound).all())
    assert d_out < 8e-4


# ------------------------------------------------------------------------------------------------- 4. chained, as the tape runs it
@regimes
@cases(CHAINED)
def test_spatial_backward_chained_to_the_forward_kernel(dev, AD, case, regime):
    """pt_attn_fwd_lse_f16, then pt_attn_bwd_f16 on the forward's own O and lse (tight pitches); the model is fed the kernel's O."""
    N, S, heads, hd = case
    rows = N * S
    pr = spatial_problem(case, regime)
    out, lse = spatial_forward(dev, case, regime)
    g, _ = spatial_backward(dev, case, regime, False, out[:rows], lse[:rows * heads])
    written_and_untouched(g, rows, heads * hd)
    model = run_model(spatial_model, pr, spatial_heads, spatial_rows, case, out[:rows])
    check_blocks("spatial chained", case, regime, g, pr.grads, model, recompute(AD, dev, "spatial", case, regime))


# ------------------------------------------------------------------------------------------------- 5. the one-block temporal kernel
@regimes
@pads
@cases(TEMPORAL)
def test_temporal_one_block_kernel_against_fp64(dev, AD, case, pad, regime):
    """attn_temporal_bwd_kernel (F <= 16) per block against its model; the second model (dS rounded unscaled, the scale on the
    fp32 sums as in the spatial passes) is printed beside it: what the kernel's order of scaling and rounding costs."""
    B, Fr, S, heads, hd = case
    pr = temporal_problem(case, regime)
    g = temporal_backward(dev, case, regime, pad)
    written_and_untouched(g, B * Fr * S, heads * hd)
    model = run_model(temporal_model, pr, temporal_heads, temporal_rows, case)
    second = run_model(temporal_model, pr, temporal_heads, temporal_rows, case, scale_after_sum=True)
    check_blocks("temporal one-block, " + ("padded" if pad else "tight"), case, regime, g, pr.grads, model, recompute(AD, dev, "temporal", case, regime), second)


# ------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_of_the_spatial_entry_point(dev):
    from posetraj_amd import hip
    L = hip.lib()
    N, S, heads = 1, 8, 1

    def call(hd=64, S=S, ldq=None, dq_off=0):
        Cc = heads * hd
        qkv, o, dy, g = (torch.zeros((N * 8, w), dtype=torch.float16, device=dev) for w in (3 * Cc, Cc, Cc, 3 * Cc))
        lse, dot = (torch.zeros((N * 8, heads), dtype=torch.float32, device=dev) for _ in range(2))
        p0, g0, ld = qkv.data_ptr(), g.data_ptr(), 3 * Cc
        rc = L.pt_attn_bwd_f16(p0, ld if ldq is None else ldq, p0 + 2 * Cc, ld, p0 + 4 * Cc, ld, o.data_ptr(), Cc, dy.data_ptr(), Cc, lse.data_ptr(), dot.data_ptr(),
                               g0 + dq_off, g0 + 2 * Cc, g0 + 4 * Cc, ld, N, S, heads, hd, hd ** -0.5, stream())
        torch.cuda.synchronize()
        return rc, L.pt_last_error().decode()

    for kw, cause in ((dict(hd=80), "head_dim 80 unsupported"), (dict(ldq=3 * 64 + 4), "pitches must be multiples of 8"),
                      (dict(dq_off=2), "misaligned pointer"), (dict(S=0), "bad sizes")):
        rc, msg = call(**kw)
        assert rc != 0 and "pt_attn_bwd_f16" in msg and cause in msg, (kw, rc, msg)
    assert call()[0] == 0
