"""Shared by tests/test_fused_exact_cpu.py and tests/test_fused_exact_gpu.py: case tables, operand builders, fp64 references, the fp32
LayerNorm emulations and the CPU fault models for pt_ffn_geglu_f16 (csrc/ffn.hip, with its pre= prologue) and pt_ln_linear_f16
(csrc/lnlin.hip), which the GPU file holds against these references BIT FOR BIT.  Nothing here needs a GPU.

The argument.  GEMM parts are those of tests/test_igemm_exact_gpu.py: fp16 operands that are small integers (or integers times a power
of two), every partial sum below 2^24 in units of the smallest weight, so the fp32 accumulator is THE value whatever the order.  The
GEGLU gate is saturated (every gate accumulator = 8 mod 16: pt_gelu_erf2 returns max(g, 0) up to a signed zero), and the intermediate
h = fp16(fp32(val * gelu(g))) is one RNE rounding of a known integer - a real rounding point, reproduced here.

A LayerNorm in the middle does not spoil this when the rows are chosen for it.  Every row is one of (c, a integers, a a power of two)
    balanced   160 x (c + a), 160 x (c - a)                normalised values exactly +-1
    skewed     64 x (c + a), 256 x (c - a), or the mirror  mean c -+ 0.6 a, sigma 0.8 a, normalised values {2, -1/2} or {1/2, -2}
    all-zero                                               y = beta exactly
    constant   (pt_ln_linear_f16 only)                     its centred second pass gives mean = P = c exactly: y = beta
so with gamma in {+-4, +-8} and beta in {-1, 0, 1} the exact y = n gamma + beta is a small non-zero integer, the kernel's fp32 value
lies within ~2^-15 relative of it (eps = 1e-5 alone moves it by 2^-17 at a = 1) - 8 x below half an fp16 ulp - and fp16(y) IS that
integer.  problem() asserts this with fp32 emulations of both kernels' statistics in the kernels' own order (ln_ffn_f32: two passes,
per-lane partial sums, the two wave halves through LDS; ln_lnlin_f32: one pass on the matrix pipe, the m^2 > 64 var centred second
pass), once as they are and with the mean moved by +-2^-15 sigma and rstd by +-2^-15 relative (PERTURB: twice a crude worst-case bound
of a 320-term fp32 sum, 320 * 2^-24 = 2^-15.7) - which covers what the emulations cannot know: fused multiply-adds, the matrix
pipe's internal order, v_rsq_f32's last bit.  Rows without variance are exact in the kernels (mean and every difference are exact)
and are not perturbed.  A y that is zero by cancellation (n gamma + beta = 0) would come out as ~1e-6, an fp16 subnormal: "no
expected y is zero unless the row has no variance" is asserted.

For the pre= path the prologue's h must be such a row: draw the target T (pattern rows), integer attention rows, Wo, bo and the row
vector, and set pre_res = T - (a Wo^T + bo + vec[idx(m)]) on the CPU (asserted: integers, |pre_res| <= 2048).  A dropped K tile of
Wo, a wrong row-vector index or bias column destroys the pattern and changes the output grossly.

Sizing (what the asserted preconditions left): feed-forward gamma = +-4 (|y| <= 9), W1 rows sparse - one entry per 64-deep K tile -
and a gate bias of 8.  With gate entries +-16 and value entries +-1 (the smallest sizing that saturates the gate) every product
val * g is a multiple of 8 below 16384 and fp16 holds it exactly: the rounding of h would not be exercised.  Committed instead:
plain cases (|x| <= 3) value +-2, gate +-128 (|val| <= 33, |g| <= 1928, |val g| <= 63 624 < 65504 by construction); without b1 odd
data, value +-3, gate +-72 = 8 * 9 (five odd terms: g = 8 mod 16 without a bias; |val g| <= 48 600); pre= cases value +-1, gate +-32
(observed |val g| < 30 000, asserted < 65504).  Products reach beyond 16384 where odd multiples of 8 are no fp16 numbers, so h is
really rounded (pr["rounded"] counts where).  W2 rows: one entry +-2^-k per 64-column chunk, k = 0 up to three chunks and 3 at
inner = 1280, which keeps |out| < 60000.  pt_ln_linear_f16: gamma in {+-4, +-8}, dense weights {+-1, +-2}: |out| <= 4 * 320 * 17 * 2 = 43 520.

ff_model / ll_model are the reference arithmetic again, evaluated numerically from the operands (LayerNorm in fp64), with one planted
fault each: tests/test_fused_exact_cpu.py shows that every fault changes the case that names it."""
import dataclasses
import functools
import os
import zlib

import numpy as np
import torch

from tests.independent_clips import mode2_index, mode3_index
from tests.test_gemm_exact_gpu import NAN, bits, guarded, ints, wints
from tests.test_igemm_exact_gpu import exact_chain, positive_zero

C = 320
EPS = 1e-5
ALPHA = 0.25                          # alpha and 1 - alpha are exact in binary
VG = 77                               # mode 1: a period that straddles fragments, wave pairs and workgroups
V2 = (100, 30, 45)                    # mode 2 (vFS, vS, vB): (m / 100) * 30 + m % 30 reaches 89 at M = 300 and wraps at 45
V3 = (2, 50, 10, 6)                   # mode 3 (vG, vFS, vS, vB)
PERTURB = 2.0 ** -15
PAD = dict(x=16, out=8, res=24, blend=32, vec=8, pre_res=40, pre_vec=8)      # pitch pads: ldx, ldo, ldr and ldb all differ
BAL, SKEW_HI, SKEW_LO, ZERO, CONST = range(5)


def report(line: str):
    print(line)
    path = os.environ.get("PT_FUSED_EXACT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


# ------------------------------------------------------------------------------------------------- case tables
@dataclasses.dataclass(frozen=True)
class FF:
    """One launch of pt_ffn_geglu_f16."""
    name: str
    M: int
    inner: int = 64
    pre: bool = False
    res: bool = False
    vec: int = 0                      # the tail's vec_mode (1 or 2)
    blend: bool = False
    b1: bool = True
    b2: bool = True
    kpad2_extra: int = 0              # NaN pad columns behind every row of the W2 image
    pre_vec: int = 0                  # pre_vec_mode (1, 2, 3)
    pre_b: bool = True

    @property
    def w2_shift(self):               # W2 entries are +-2^-k
        return 3 if self.inner > 192 else 0

    @property
    def w1_scales(self):              # magnitude of the value rows' and of the gate rows' entries (module docstring: sizing)
        return (1, 32) if self.pre else ((2, 128) if self.b1 else (3, 72))

    @property
    def variant(self):
        tail = "+".join(k for k, on in (("res", self.res), (f"vec{self.vec}", self.vec), ("blend", self.blend)) if on) or "none"
        return ("pre" + (f"(vec{self.pre_vec})" if self.pre_vec else "") + " " if self.pre else "") + f"V_P{int(self.res) + int(self.vec > 0) + int(self.blend)} {tail}"


TAILS = {"none": dict(), "res": dict(res=True), "res_vec1": dict(res=True, vec=1), "res_vec2": dict(res=True, vec=2),
         "res_blend": dict(res=True, blend=True), "vec_blend": dict(vec=1, blend=True)}
# A. the plain feed-forward.  A workgroup has 128 rows, a wave pair 32, a fragment 16
FF_PLAIN = ([FF(f"ff_m{M}", M, **kw) for M, kw in ((1, TAILS["res"]), (17, TAILS["none"]), (128, TAILS["res_blend"]), (129, TAILS["res_vec1"]))] +
            [FF(f"ff_m300_{k}", 300, **kw) for k, kw in TAILS.items()] +
            [FF("ff_inner128", 300, 128, res=True),               # nch = 2: the ring's first refill
             FF("ff_inner192", 300, 192, res=True, vec=1),        # nch = 3
             FF("ff_inner1280", 300, 1280, res=True),             # nch = 20: the product's own width
             FF("ff_m1157", 1157, res=True, vec=2),               # ten workgroups, through pt_xcd_remap
             FF("ff_no_b1", 300, res=True, b1=False),
             FF("ff_no_b2", 300, res=True, b2=False),
             FF("ff_kpad2", 300, 128, res=True, kpad2_extra=64)])
# B. with the prologue: out-projection + residual + row vector, LayerNorm, the feed-forward's residual is h
FF_PRE = ([FF(f"pre_m{M}", M, pre=True, **kw) for M, kw in ((1, dict()), (17, dict(blend=True)), (129, dict(pre_vec=1)), (300, dict()))] +
          [FF("pre_inner192", 300, 192, pre=True, pre_vec=2),
           FF("pre_inner1280", 300, 1280, pre=True, pre_vec=1, blend=True),
           FF("pre_vec1", 300, pre=True, pre_vec=1),
           FF("pre_vec2", 300, pre=True, pre_vec=2, blend=True),
           FF("pre_vec3", 300, pre=True, pre_vec=3),
           FF("pre_no_bias", 300, pre=True, pre_b=False, pre_vec=1),
           FF("pre_blend", 300, pre=True, blend=True),
           FF("pre_vec2_tail_vec1", 300, pre=True, pre_vec=2, vec=1),       # the tail's own row vector beside the prologue's
           FF("pre_m1157", 1157, pre=True, pre_vec=3, vec=1)])
FF_CASES = FF_PLAIN + FF_PRE


@dataclasses.dataclass(frozen=True)
class LL:
    """One launch of pt_ln_linear_f16."""
    name: str
    M: int
    N: int
    cs_cols: int = 0
    cs_scale: float = 4.0
    xpad: int = 8
    lead: int = 0                     # out is the column block [lead, lead + N) of a wider NaN-filled buffer

    @property
    def variant(self):
        return f"N={self.N} cs_cols={self.cs_cols} cs_scale={self.cs_scale} ldx={C + self.xpad} out+{self.lead}"


def _cs(i, N):
    """cs_cols cycles over {0, 64, 320, the largest multiple of 64 <= N} (kept <= N), cs_scale over {0.25, 4}"""
    top = N // 64 * 64
    return dict(cs_cols=min((0, 64, 320, top)[i % 4], top), cs_scale=(0.25, 4.0)[(i // 2) % 2])


# C. chunk counts 1 .. 8 (the three peeled chunks, both parities of the loop unrolled by two and both of its exits), ragged last chunk
# and wave half (8, 72, 1000)
LL_CASES = ([LL(f"ll_n{N}", 300, N, **_cs(i + 1, N)) for i, N in enumerate((8, 72, 128, 256, 384, 512, 640, 768, 896, 960, 1000))] +
            [LL(f"ll_m{M}", M, 960, **_cs(i, 960)) for i, M in enumerate((1, 17, 128, 129))] +
            [LL("ll_m1157", 1157, 128, cs_cols=64, cs_scale=0.25),
             LL("ll_cs0", 300, 640, cs_cols=0), LL("ll_cs64", 300, 640, cs_cols=64, cs_scale=0.25), LL("ll_cs320", 300, 640, cs_cols=320),
             LL("ll_cs_top", 300, 1000, cs_cols=960, cs_scale=0.25),
             LL("ll_ldx", 300, 384, cs_cols=320, xpad=40),
             LL("ll_out_block", 300, 384, cs_cols=64, lead=16)])
CASES = {c.name: c for c in FF_CASES + LL_CASES}
assert len(CASES) == len(FF_CASES) + len(LL_CASES)


def seed_of(c):
    return zlib.crc32(c.name.encode()) % 1000003


# ------------------------------------------------------------------------------------------------- index models
def vec_rows(mode, M):
    """Row of the row-vector table for every output row (include/posetraj_hip.h: vec_mode); mode 3 from tests/independent_clips.py"""
    m = np.arange(M)
    idx = m // VG if mode == 1 else (mode2_index(m, *V2) if mode == 2 else mode3_index(m, *V3))
    return torch.from_numpy(idx.astype(np.int64))


def vec_boundary(mode, M):
    """A row m < M - 1 whose neighbour m + 1 reads another row of the table (a period boundary)."""
    idx = vec_rows(mode, M)
    m = (idx[1:] != idx[:-1]).nonzero().flatten()
    assert m.numel()
    return int(m[0])


# ------------------------------------------------------------------------------------------------- operand builders
def sparse_rows(rows, K, seed):
    """[rows, K] fp32: one entry +-1 in every 64-deep K tile of every row."""
    g = torch.Generator().manual_seed(seed)
    nt = K // 64
    col = torch.randint(0, 64, (rows, nt), generator=g) + 64 * torch.arange(nt)
    sign = (torch.randint(0, 2, (rows, nt), generator=g) * 2 - 1).float()
    return torch.zeros(rows, K).scatter_(1, col, sign)


def pattern(kind, a, c, seed):
    """Rows of the given kinds -> (x [M, 320] fp64 integers, n [M, 320] fp64: the exactly normalised values)."""
    g = torch.Generator().manual_seed(seed)
    M = len(kind)
    hi = torch.zeros(M, C, dtype=torch.bool)
    for m in range(M):
        k = {BAL: 160, SKEW_HI: 64, SKEW_LO: 256}.get(int(kind[m]), 0)
        hi[m, torch.randperm(C, generator=g)[:k]] = True
    kind, a, c = kind[:, None], a.double()[:, None], c.double()[:, None]
    x = torch.where(hi, c + a, c - a)
    n = torch.where(hi, 1.0, -1.0).double()
    n = torch.where(kind == SKEW_HI, torch.where(hi, 2.0, -0.5), n)
    n = torch.where(kind == SKEW_LO, torch.where(hi, 0.5, -2.0), n)
    flat = kind >= ZERO
    return torch.where(flat, c.expand(M, C), x), torch.where(flat, torch.zeros(()).double(), n)


def ff_rows(M, seed):
    """B: balanced / skewed / all-zero mixed, a in {1 .. 16} and c in [-40, 40] per row"""
    g = torch.Generator().manual_seed(seed)
    kind = torch.randint(0, 4, (M,), generator=g)
    a = 2 ** torch.randint(0, 5, (M,), generator=g)
    c = torch.randint(-40, 41, (M,), generator=g)
    return kind, a, torch.where(kind == ZERO, 0, c)


def ll_rows(M, seed):
    """C: near rows |c| <= 5 a (|mean| <= 5.6 a = 7 sigma at most: inside the kernel's |mean| < 8 sigma on every pattern), far rows
    9 a <= |c| <= 100 a with |c| + a <= 2048, constant and all-zero rows.  The kernel decides `far` per row but runs the centred second
    pass per 16-row fragment (__ballot): fragments cycle through all near / all far / exactly one far row / everything mixed.
    -> (kind, a, c, far as designed)"""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))
    kind, a, c, far = (torch.zeros(M, dtype=torch.int64) for _ in range(4))
    for m in range(M):
        frag, r = divmod(m, 16)
        mode = frag % 4
        is_far = mode == 1 or (mode == 2 and r == (5 * frag) % 16) or (mode == 3 and r % 2 == 1)
        k = ri(0, 2)
        if mode == 3 and r % 4 == 0:
            k = ZERO
        if mode == 3 and r % 4 == 3:
            k = CONST
        e = ri(0, 4)
        lo, hi = (9, 100) if is_far else (0, 5)
        mag = ri(lo << e, min(hi << e, 2048 - (1 << e)))
        if k == CONST:
            mag = ri(1, 2048)
        kind[m], a[m], far[m] = k, 1 << e, int(k == CONST or (is_far and k != ZERO))
        c[m] = 0 if k == ZERO else mag * (ri(0, 1) * 2 - 1)
    return kind, a, c, far.bool()


def affine(seed, gammas):
    g = torch.Generator().manual_seed(seed)
    gamma = torch.tensor(gammas, dtype=torch.float64)[torch.randint(0, len(gammas), (C,), generator=g)]
    return gamma, torch.randint(-1, 2, (C,), generator=g).double()


# ------------------------------------------------------------------------------------------------- fp32 LayerNorm emulations
def _finish_f32(h, mean, rstd, gamma, beta, live, dmean, drstd):
    f = np.float32
    mean = np.where(live, mean + f(dmean) / rstd, mean).astype(f)         # rows without variance are exact in the kernels
    rstd = np.where(live, rstd * f(1.0 + drstd), rstd).astype(f)
    y = ((h - mean[:, None]) * rstd[:, None]) * gamma.astype(f) + beta.astype(f)
    assert y.dtype == f
    return y.astype(np.float16)


def _rsqrt_f32(v):
    return (1.0 / np.sqrt(v.astype(np.float64))).astype(np.float32)


def ln_ffn_f32(h, gamma, beta, dmean=0.0, drstd=0.0):
    """ffn320_kernel's prologue (ffn.hip:181-224) in numpy fp32: per lane the 40 values (ni, j) of its quarter of a wave half in order,
    then lanes (fq, fq ^ 1), (fq ^ 2): (s0 + s1) + (s2 + s3), then the two halves from LDS; mean = sum * fl(1 / 320); the second pass on
    h - mean.  h: [M, 320] exact fp32 values -> fp16 [M, 320]"""
    f = np.float32
    h = h.astype(f)
    r320 = f(1.0) / f(320.0)

    def halves(v):
        v = v.reshape(-1, 2, 10, 4, 4)                            # [row, wave half, ni, fq, j]: column 160 wc + 16 ni + 4 fq + j
        s = np.zeros((v.shape[0], 2, 4), f)
        for ni in range(10):
            for j in range(4):
                s = s + v[:, :, ni, :, j]
        s = (s[:, :, 0] + s[:, :, 1]) + (s[:, :, 2] + s[:, :, 3])
        return s[:, 0] + s[:, 1]

    mean = halves(h) * r320
    d = h - mean[:, None]
    var = halves(d * d) * r320
    rstd = _rsqrt_f32(var + f(EPS))
    return _finish_f32(h, mean, rstd, gamma, beta, var > 0, dmean, drstd)


def ln_lnlin_f32(x16, gamma, beta, dmean=0.0, drstd=0.0, keep_one_pass=False):
    """lnlin320_kernel's statistics (lnlin.hip:113-164) in numpy: sum and sum of squares from ten MFMA steps of 32 products (modelled
    as fp32(acc + the exact sum of a step)), m = s * fl(1 / 320), var = q * fl(1 / 320) - m m, far = m m > 64 var; far rows again on
    fragments centred in fp16 on P = fp16(m).  x16: [M, 320] numpy fp16 -> (fp16 [M, 320], far [M])"""
    f = np.float32
    r320 = f(1.0) / f(320.0)

    def mfma(v64):
        acc = np.zeros(v64.shape[0], f)
        for t in range(10):
            acc = (acc.astype(np.float64) + v64[:, 32 * t:32 * t + 32].sum(1)).astype(f)
        return acc

    x64 = x16.astype(np.float64)
    m = mfma(x64) * r320
    var = mfma(x64 * x64) * r320 - m * m
    far = m * m > f(64.0) * var
    p = m.astype(np.float16)
    d = x16 - p[:, None]
    assert d.dtype == np.float16
    d64 = d.astype(np.float64)
    dm = mfma(d64) * r320
    dv = mfma(d64 * d64) * r320 - dm * dm
    sel = far & (not keep_one_pass)
    m, var = np.where(sel, p.astype(f) + dm, m).astype(f), np.where(sel, dv, var).astype(f)
    rstd = _rsqrt_f32(np.maximum(var, f(0.0)) + f(EPS))
    live = x64.max(1) != x64.min(1)
    return _finish_f32(x16.astype(f), m, rstd, gamma, beta, live, dmean, drstd), far


PERTURBATIONS = [(0.0, 0.0)] + [(dm, dr) for dm in (-PERTURB, PERTURB) for dr in (-PERTURB, PERTURB)]


def expected_y(x, n, gamma, beta):
    """y = n gamma + beta: integers, and none zero by cancellation"""
    y = n * gamma + beta
    live = (x.max(1).values != x.min(1).values)[:, None]
    assert bool((y == y.round()).all()) and float(y.abs().max()) <= 17 and bool(((y != 0) | ~live).all())
    assert torch.equal(y.half().double(), y)
    return y


# ------------------------------------------------------------------------------------------------- the feed-forward: problem and reference
def _same_in_fp32(a64, *factors):
    """a64 = the fp64 product of ``factors`` (or a value): the fp32 evaluation agrees"""
    if factors:
        a32 = factors[0].float() @ factors[1].float().t()
        assert torch.equal(a32.double(), a64)
    assert torch.equal(a64.float().double(), a64)
    return a64


@functools.lru_cache(maxsize=None)
def ff_problem(c):
    """Operands (fp16 / fp32 CPU tensors), packs and the fp64 reference of a feed-forward case, every precondition asserted."""
    from posetraj_amd import packing
    seed, M, I = seed_of(c), c.M, c.inner
    pr = dict()
    w1 = sparse_rows(2 * I, C, seed + 1)
    vw, gw = c.w1_scales
    w1[:I] *= vw                                                  # rows [value | gate]
    w1[I:] *= gw
    b1 = torch.cat([ints(I, seed=seed + 2).float(), torch.full((I,), 8.0)]) if c.b1 else None
    w2 = sparse_rows(C, I, seed + 3) * 2.0 ** -c.w2_shift
    b2 = ints(C, seed=seed + 4).float() if c.b2 else None
    pr.update(w1=w1, b1=b1, w2=w2, b2=b2, p1=packing.pack_linear(w1, b1, "cpu", geglu=True), p2=packing.pack_linear(w2, b2, "cpu"))
    assert pr["p1"].w.shape == (2 * I, C) and pr["p2"].w.shape == (384, I) and torch.equal(pr["p2"].w[:C].float(), w2)
    h = None
    if c.pre:
        kind, a, cc = ff_rows(M, seed + 5)
        T, n = pattern(kind, a, cc, seed + 6)
        gamma, beta = affine(seed + 7, (-4.0, 4.0))
        y = expected_y(T, n, gamma, beta)
        for dm, dr in PERTURBATIONS:                              # the kernel's fp32 LayerNorm rounds to these integers
            got = ln_ffn_f32(T.numpy(), gamma.numpy(), beta.numpy(), dm, dr)
            assert np.array_equal(got, y.numpy().astype(np.float16)), (c.name, dm, dr)
        att, wo = ints(M, C, seed=seed + 8), wints(C, C, seed=seed + 9)
        bo = ints(C, seed=seed + 10).float() if c.pre_b else None
        proj = _same_in_fp32(att.double() @ wo.double().t(), att, wo)
        init = torch.zeros(M, C, dtype=torch.float64) + (bo.double() if c.pre_b else 0.0)
        pidx = pvec = None
        if c.pre_vec:
            pidx = vec_rows(c.pre_vec, M)
            pvec = ints(int(pidx.max()) + 1, C, seed=seed + 11)
            assert c.pre_vec == 1 or pvec.shape[0] == (V2[2] if c.pre_vec == 2 else V3[3])
            init = init + pvec.double()[pidx]
        pre_res = T - (proj + init)
        assert bool((pre_res == pre_res.round()).all()) and float(pre_res.abs().max()) <= 2048
        assert float((att.double().abs() @ wo.double().abs().t() + init.abs() + pre_res.abs()).max()) < 2 ** 24
        h = _same_in_fp32(proj + init + pre_res)
        assert torch.equal(h, T)
        pr.update(kind=kind, T=T, gamma=gamma, beta=beta, att=att, wo=wo, bo=bo, po=packing.pack_linear(wo, bo, "cpu"), pidx=pidx, pvec=pvec,
                  pre_res=pre_res.half())
        x = att
    else:
        x = ints(M, C, seed=seed + 8)
        if not c.b1:                                              # odd data: five odd terms x 8 = 8 (mod 16) without a gate bias
            x = torch.where(x.abs() == 2, x / 2, x)
        y = x.double()
    t1 = _same_in_fp32(y @ w1.double().t(), y, w1) + (b1.double() if c.b1 else 0.0)
    val, gate = t1[:, :I], t1[:, I:]
    prod = val * gate.clamp(min=0)
    assert float(gate.abs().min()) >= 8 and bool((gate % 16 == 8).all())
    assert float((val * gate).abs().max()) < min(2 ** 24, 65504)
    h2 = _same_in_fp32(prod).half()                               # the rounding point: fp32 product -> fp16
    t2 = h2.double() @ w2.double().t()
    base = t2 + (b2.double() if c.b2 else 0.0) + (h if c.pre else 0.0)
    top = h2.double().abs() @ w2.double().abs().t() + (b2.double().abs() if c.b2 else 0.0) + (h.abs() if c.pre else 0.0)
    assert float(top.max()) * 2 ** c.w2_shift < 2 ** 24           # every partial sum, whatever the order
    _same_in_fp32(base)
    steps = []
    res = ints(M, C, seed=seed + 12) if c.res else None
    vidx = vec = None
    if c.res:
        steps.append(lambda a, dt: a + res.to(dt))
    if c.vec:
        vidx = vec_rows(c.vec, M)
        vec = ints(int(vidx.max()) + 1, C, seed=seed + 13)
        rows = vec[vidx]
        steps.append(lambda a, dt: a + rows.to(dt))
    v = exact_chain(base, steps)
    blend = ints(M, C, seed=seed + 14) if c.blend else None
    if c.blend:
        exact_chain(v, [lambda a, dt: (1.0 - ALPHA) * a])
        v = exact_chain(v, [lambda a, dt: ALPHA * blend.to(dt) + (1.0 - ALPHA) * a])
    assert float(v.abs().max()) < 60000
    pr.update(x=x, y=y, gate=gate, val=val, rounded=int((h2.double() != prod).sum()), res=res, vec=vec, vidx=vidx, blend=blend, out=v.half())
    return pr


def nan_block(t, pad, lead=0):
    """guarded() for a tensor that is the column block [lead, lead + cols) of a wider NaN-filled one"""
    wide = torch.full((t.shape[0], lead + t.shape[1]), NAN, dtype=t.dtype)
    wide[:, lead:] = t
    buf, off, ld = guarded(wide, pad)
    return buf, off + lead, ld


def ff_images(c):
    """name -> (flat CPU buffer, element offset, pitch) of every pointer of the call: NaN pitch pads, 64 NaN rows in front and behind -
    the packed weight images and the vectors (rows of their own length) included - and `want`, what `out` must be afterwards."""
    pr = ff_problem(c)
    row = lambda t: guarded(t.half()[None], 0)
    w2 = pr["p2"].w
    if c.kpad2_extra:
        w2 = torch.cat([w2, torch.full((w2.shape[0], c.kpad2_extra), NAN, dtype=w2.dtype)], 1)
    im = {"x": guarded(pr["x"], PAD["x"]), "w1": guarded(pr["p1"].w, 0), "w2": guarded(w2, 0),
          "out": guarded(torch.full((c.M, C), NAN, dtype=torch.float16), PAD["out"])}
    if c.b1:
        im["b1"] = row(pr["p1"].bias)
    if c.b2:
        im["b2"] = row(pr["p2"].bias)
    for k in ("res", "vec", "blend"):
        if pr[k] is not None:
            im[k] = guarded(pr[k], PAD[k])
    if c.pre:
        im.update(wo=guarded(pr["po"].w, 0), pre_res=guarded(pr["pre_res"], PAD["pre_res"]), gamma=row(pr["gamma"]), beta=row(pr["beta"]))
        if c.pre_b:
            im["bo"] = row(pr["po"].bias)
        if c.pre_vec:
            im["pre_vec"] = guarded(pr["pvec"], PAD["pre_vec"])
    return im, guarded(pr["out"], PAD["out"])[0]


def ff_params(c, im, base):
    """hip.FfnParams of a case; base: name -> device address of that buffer."""
    from posetraj_amd import hip
    at = lambda k: base[k] + 2 * im[k][1] if k in im else None
    ld = lambda k: im[k][2] if k in im else 0
    p = hip.FfnParams()
    p.x, p.ldx, p.M, p.C, p.inner = at("x"), ld("x"), c.M, C, c.inner
    p.w1, p.b1, p.kpad1 = at("w1"), at("b1"), C
    p.w2, p.b2, p.kpad2 = at("w2"), at("b2"), c.inner + c.kpad2_extra
    p.out, p.ldo, p.res, p.ldr = at("out"), ld("out"), at("res"), ld("res")
    if c.vec:
        p.vec, p.ldv, p.vec_mode, p.vG = at("vec"), ld("vec"), c.vec, VG
        p.vFS, p.vS, p.vB = V2
    if c.blend:
        p.blend, p.ldb, p.alpha = at("blend"), ld("blend"), ALPHA
    if c.pre:
        p.pre_w, p.pre_b, p.pre_kpad = at("wo"), at("bo"), C
        p.pre_res, p.pre_ldr = at("pre_res"), ld("pre_res")
        p.ln_gamma, p.ln_beta, p.ln_eps = at("gamma"), at("beta"), EPS
        if c.pre_vec:
            p.pre_vec, p.pre_ldv, p.pre_vec_mode = at("pre_vec"), ld("pre_vec"), c.pre_vec
            if c.pre_vec == 1:
                p.pre_vG = VG
            elif c.pre_vec == 2:
                p.pre_vFS, p.pre_vS, p.pre_vB = V2
            else:
                p.pre_vG, p.pre_vFS, p.pre_vS, p.pre_vB = V3
    return p


def layernorm64(h, gamma, beta, mean=None, keep_mean=False, drop_beta=False):
    mu = h.mean(1, keepdim=True) if mean is None else mean
    rstd = 1.0 / torch.sqrt(((h - mu) ** 2).mean(1, keepdim=True) + EPS)
    return ((h if keep_mean else h - mu) * rstd * gamma + (0.0 if drop_beta else beta)).half().double()


FF_FAULTS = ("wo_ktile", "w1_ktile", "w2_ktile", "pre_vec_neighbour", "vec_neighbour", "clamped_row", "half_swap", "mean_kept",
             "h_unrounded", "beta_dropped")


def ff_model(c, fault=None):
    """pt_ffn_geglu_f16 from the operands, numerically (the LayerNorm in fp64) -> the whole guarded `out` buffer.  ``fault``:
    wo_ktile / w1_ktile / w2_ktile: one 64-deep K tile of that product dropped;  pre_vec_neighbour / vec_neighbour: the row in front of
    a period boundary takes vec[idx(m + 1)];  clamped_row: the clamped row min(row, M - 1) also written to row M;  half_swap: one row's
    mean from the other wave half's partial sum twice;  mean_kept: mean not subtracted;  h_unrounded: the GEGLU product not rounded to
    fp16 before stage 2;  beta_dropped."""
    pr, M, I = ff_problem(c), c.M, c.inner
    assert fault is None or fault in FF_FAULTS
    drop = lambda w, kt: torch.cat([w[:, :64 * kt], torch.zeros(w.shape[0], 64), w[:, 64 * kt + 64:]], 1)
    h = None
    if c.pre:
        wo = pr["wo"].double()
        if fault == "wo_ktile":
            wo = drop(wo, 3)
        h = pr["att"].double() @ wo.t() + pr["pre_res"].double() + (pr["bo"].double() if c.pre_b else 0.0)
        if c.pre_vec:
            idx = pr["pidx"].clone()
            if fault == "pre_vec_neighbour":
                m = vec_boundary(c.pre_vec, M)
                idx[m] = idx[m + 1]
            h = h + pr["pvec"].double()[idx]
        mean = h.mean(1, keepdim=True)
        if fault == "half_swap":
            uneven = (h[:, :160].sum(1) != h[:, 160:].sum(1)).nonzero().flatten()      # (a random split of a pattern row is rarely even)
            assert uneven.numel() > M // 2
            m = int(uneven[uneven.numel() // 2])
            mean[m] = 2 * h[m, 160:].sum() / 320
        y = layernorm64(h, pr["gamma"], pr["beta"], mean, fault == "mean_kept", fault == "beta_dropped")
    else:
        y = pr["y"]
    w1 = drop(pr["w1"].double(), 1) if fault == "w1_ktile" else pr["w1"].double()
    t1 = y @ w1.t() + (pr["b1"].double() if c.b1 else 0.0)
    prod = t1[:, :I] * t1[:, I:].clamp(min=0)
    h2 = prod if fault == "h_unrounded" else prod.float().half().double()
    w2 = drop(pr["w2"].double(), I // 64 - 1) if fault == "w2_ktile" else pr["w2"].double()
    v = h2 @ w2.t() + (pr["b2"].double() if c.b2 else 0.0) + (h if c.pre else 0.0)
    if c.res:
        v = v + pr["res"].double()
    if c.vec:
        idx = pr["vidx"].clone()
        if fault == "vec_neighbour":
            m = vec_boundary(c.vec, M)
            idx[m] = idx[m + 1]
        v = v + pr["vec"].double()[idx]
    if c.blend:
        v = ALPHA * pr["blend"].double() + (1.0 - ALPHA) * v
    out = v.half()
    buf, off, ld = guarded(out, PAD["out"])
    if fault == "clamped_row":
        buf[off + M * ld:off + M * ld + C] = out[M - 1]
    return buf


# ------------------------------------------------------------------------------------------------- LayerNorm + linear: problem and reference
@functools.lru_cache(maxsize=None)
def ll_problem(c):
    from posetraj_amd import packing
    seed, M, N = seed_of(c), c.M, c.N
    kind, a, cc, far = ll_rows(M, seed + 1)
    x, n = pattern(kind, a, cc, seed + 2)
    assert float(x.abs().max()) <= 2048
    gamma, beta = affine(seed + 3, (-8.0, -4.0, 4.0, 8.0))
    y = expected_y(x, n, gamma, beta)
    x16 = x.half()
    assert torch.equal(x16.double(), x)
    for dm, dr in PERTURBATIONS:
        got, far_emulated = ln_lnlin_f32(x16.numpy(), gamma.numpy(), beta.numpy(), dm, dr)
        assert np.array_equal(got, y.numpy().astype(np.float16)), (c.name, dm, dr)
        assert np.array_equal(far_emulated, far.numpy()), c.name    # the rows take the path they were drawn for
    w = wints(N, C, seed=seed + 4)
    pack = packing.pack_linear(w, None, "cpu")
    assert pack.w.shape == (-(-N // 128) * 128, C) and pack.bias is None
    t = _same_in_fp32(y @ w.double().t(), y, w)
    assert c.cs_cols % 64 == 0 and c.cs_cols <= N
    scale = torch.ones(N, dtype=torch.float64)
    scale[:c.cs_cols] = c.cs_scale
    v = exact_chain(t, [lambda a, dt: a * scale.to(dt)])
    assert float(v.abs().max()) < 60000
    return dict(kind=kind, a=a, c=cc, far=far, x=x16, y=y, gamma=gamma, beta=beta, w=w, pack=pack, scale=scale, out=v.half())


def ll_images(c):
    pr = ll_problem(c)
    row = lambda t: guarded(t.half()[None], 0)
    im = {"x": guarded(pr["x"], c.xpad), "w": guarded(pr["pack"].w, 0), "gamma": row(pr["gamma"]), "beta": row(pr["beta"]),
          "out": nan_block(torch.full((c.M, c.N), NAN, dtype=torch.float16), PAD["out"], c.lead)}
    return im, nan_block(pr["out"], PAD["out"], c.lead)[0]


def ll_params(c, im, base):
    from posetraj_amd import hip
    at = lambda k: base[k] + 2 * im[k][1]
    p = hip.LnLinParams()
    p.x, p.ldx, p.M, p.N, p.K = at("x"), im["x"][2], c.M, c.N, C
    p.w, p.kpad, p.bias = at("w"), C, None
    p.ln_gamma, p.ln_beta, p.ln_eps = at("gamma"), at("beta"), EPS
    p.out, p.ldo = at("out"), im["out"][2]
    p.cs_cols, p.cs_scale = c.cs_cols, c.cs_scale
    return p


LL_FAULTS = ("w_ktile", "clamped_row", "other_row_stats", "mean_kept", "far_one_pass", "cs_chunk", "swap16", "beta_dropped")


def ll_model(c, fault=None):
    """pt_ln_linear_f16 from the operands, numerically -> the whole guarded `out` buffer.  ``fault``: w_ktile: a K tile of W dropped;
    clamped_row: row M - 1 also written to row M;  other_row_stats: one row normalised with its neighbour's mean and rstd;  mean_kept;
    far_one_pass: far rows keep the one-pass variance (the fp32 emulation);  cs_chunk: the column scale chosen per 128-column chunk, not
    per 64-column wave half;  swap16: the two 16-column blocks of a store pair exchanged;  beta_dropped."""
    pr, M, N = ll_problem(c), c.M, c.N
    assert fault is None or fault in LL_FAULTS
    x, gamma, beta = pr["x"].double(), pr["gamma"], pr["beta"]
    if fault == "far_one_pass":
        y = torch.from_numpy(ln_lnlin_f32(pr["x"].numpy(), gamma.numpy(), beta.numpy(), keep_one_pass=True)[0]).double()
    elif fault == "other_row_stats":
        live = (pr["kind"] < ZERO).nonzero().flatten()
        src = torch.arange(M)
        src[live[0]] = live[1]
        mu, sd = x.mean(1, keepdim=True)[src], torch.sqrt(x.var(1, unbiased=False, keepdim=True) + EPS)[src]
        y = ((x - mu) / sd * gamma + beta).half().double()
    else:
        y = layernorm64(x, gamma, beta, None, fault == "mean_kept", fault == "beta_dropped")
    w = pr["w"].double()
    if fault == "w_ktile":
        w = torch.cat([w[:, :256], torch.zeros(N, 64)], 1)
    scale = pr["scale"]
    if fault == "cs_chunk":
        scale = scale.clone()
        col = torch.arange(N)
        scale[:] = torch.where(col // 128 * 128 < c.cs_cols, c.cs_scale, 1.0)
    out = (y @ w.t() * scale).half()
    if fault == "swap16":
        out = out.clone()
        out[:, 0:16], out[:, 16:32] = out[:, 16:32].clone(), out[:, 0:16].clone()
    buf, off, ld = nan_block(out, PAD["out"], c.lead)
    if fault == "clamped_row":
        buf[off + M * ld:off + M * ld + N] = out[M - 1]
    return buf


# ------------------------------------------------------------------------------------------------- checkers
def differing(got, want, relax_zero=False):
    """(elements of the whole buffer - guard and pad included - whose bits differ, the first such index); relax_zero: -0 = +0, the one
    relaxation, for the feed-forward only (NaN still differs from every number)"""
    a, b = (positive_zero(got), positive_zero(want)) if relax_zero else (bits(got), bits(want))
    bad = (a != b).nonzero().flatten()
    return int(bad.numel()), (int(bad[0]) if bad.numel() else -1)
