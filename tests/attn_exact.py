"""Exact-data problems for the attention forward kernels (csrc/attn.hip, csrc/attn_general.hip): generators, the fp64 reference, the
checkers and a CPU model of the kernels' rounding points into which structural faults can be planted.  tests/test_attn_exact_cpu.py
holds all of this together without a GPU; tests/test_attn_exact_gpu.py runs the same cases through the kernels.

A problem is three fp16 tensors q [G, Sq, D], k, v [G, Sk, D], one slice per (image | batch | (clip, position), head) group, every group
drawn from its own seed - data fetched from a neighbouring group is wrong data, not plausible data.  Scores are counted in log2 units:
score = (q . k) * cexp, p = 2^(score - max).  cexp is what the kernel multiplies by, as the fp32 number it computes it as (cexp_of).

Family A - every key counted exactly once.  All scores of a query are equal, so every p is 2^0 = 1, l = Sk, O[q, d] = sum_j V[j, d] / Sk with
  V in {+-1 .. +-8}: an integer sum, exact in fp32, one reciprocal, one product, one fp16 rounding.
    A0: Q = 0.      Am: Q = 2 u, K = -2 u for a +-1 vector u: every score is -4 D, at least 40 log2 units BELOW the score 0 of a zero-staged
    key behind Sk - an unmasked pad key takes the whole softmax.
  Bound per element against fp64: |o - ref| <= ulp16(ref) / 2 + 2^-21 |ref|; ref == 0 must come back as +-0.
Family B - every query routed to its own key.  K = 4 * (+-1 codes), Q[q] = K[pi(q)], pi(q) = (7 q + 3) mod Sk: the matching key leads every
  other by >= 40 log2 units (asserted), every other p is below 2^-40 and rounds to 0 in fp16, l = 1.  O must EQUAL V[pi] bit for bit.  A
  match in a late tile makes the online kernels move their maximum and the spatial kernel re-base by >= 40 units.
Family C - dyadic softmax through the re-base logic.  Integer scores (Q = e_0 + e_r, K[j] = (base of the key's 64-key tile, jitter 0 .. 5
  per column)), cexp == 1 (q_prescaled, or scale = float32(ln 2): asserted), so every p and every re-base factor is a power of two.  The
  tile bases climb by INC - steps of 14 cross the spatial kernel's 2^8 threshold whatever the jitter, the steps of 1 and 2 behind them
  cannot - and every eighth key lies 9 below its tile's base.  Asserted per query: every score >= (the maximum up to and including its
  own 64-key tile) - 14, so P stays in fp16's normal range under a running maximum as well as under a deferred one; with five tiles or
  more at least two tiles cross the threshold and at least two do not.
  Bound per element against fp64: |o - ref| <= ulp16(ref) / 2 + (ceil(Sk / 32) + 8) 2^-23 max|V|.
lse (pt_attn_fwd_lse_f16): |lse - log2 sum_j 2^score_j| <= 2^-18 max(1, |ref|) in every family.

What each family must notice (asserted by test_attn_exact_cpu.py on the CPU model, at every case where the fault can be expressed):

    fault           A0   Am   B    C     planted as
    drop_last       x    x    .    x     the last key is left out                                          (Sk >= 2)
    dup_key         x    x    .    x     the last key is appended once more                                (Sk >= 2)
    pad_unmasked    x    x    .    .     tile - Sk % tile zero keys with zero values appended              (Sk % tile != 0)
    swap_v          .    .    x    .     V rows j and j ^ 1 exchanged, j = pi(0) (B) or the last odd key   (Sk >= 2)
    shift_q         .    .    x    .     output row q holds query q + 1's result                           (Sq >= 2, Sk >= 2)
    skip_rebase     .    .    x    x     the last tile whose maximum moves leaves O and l unscaled         (some maximum moves)
    neighbour_k     .    .    x    .     group g scores against the keys of group g + 1                    (G >= 2, Sk >= 2)

(x: must be rejected; .: not claimed - e.g. A cannot see an exchange of two V rows, B cannot see a key whose p is 0 anyway.)"""
import dataclasses
import functools
import math
import os

import numpy as np
import torch

LOG2E32 = np.float32(1.4426950408889634)          # the constant of pt_attn_*_f16
LN2_32 = float(np.float32(math.log(2.0)))         # scale of family C on the paths that multiply: float32(ln 2) * LOG2E32 == 1.0f
THR = 8.0                                         # attn.hip: THR_LOG2
MARGIN_B = 40.0
SPAN_C = 14
INC = (1, 14, 2, 14, 3, 3, 3, 14, 1, 2, 14, 3, 3, 3, 14, 2)      # base of 64-key tile t + 1 minus base of tile t
FAMILIES = ("A0", "Am", "B", "C")
FAULTS = ("drop_last", "dup_key", "pad_unmasked", "swap_v", "shift_q", "skip_rebase", "neighbour_k")
MUST_CATCH = {"drop_last": ("A0", "Am", "C"), "dup_key": ("A0", "Am", "C"), "pad_unmasked": ("A0", "Am"), "swap_v": ("B",),
              "shift_q": ("B",), "skip_rebase": ("B", "C"), "neighbour_k": ("B",)}


def cexp_of(scale):
    """scale * log2(e) as the entry points compute it: one fp32 product."""
    return float(np.float32(scale) * LOG2E32)


@dataclasses.dataclass(frozen=True)
class Case:
    kernel: str                       # spatial | general | d512 | temporal
    family: str                       # A0 | Am | B | C
    nb: int                           # images | batches | clips
    heads: int
    Sq: int
    Sk: int                           # temporal: Sq = Sk = frames
    D: int
    pos: int = 1                      # temporal: positions per clip
    pre: int = 0                      # spatial: q_prescaled
    nqb: int = 3                      # spatial: pt_attn_spatial_set_nqb
    fused: bool = False               # general: q | k | v are column blocks of one buffer
    lse: bool = False                 # general: through pt_attn_fwd_lse_f16

    @property
    def groups(self):
        return self.nb * self.pos * self.heads

    @property
    def tile(self):
        """keys per staged tile: what is zero-padded behind Sk"""
        if self.kernel == "spatial":
            return 64
        if self.kernel == "temporal":
            return 16 if self.Sk <= 16 else 32 if self.Sk <= 32 else 16 * ((self.Sk + 15) // 16)
        return 32

    @property
    def softmax(self):
        return {"spatial": "defer", "temporal": "full"}.get(self.kernel, "online")

    @property
    def scale(self):
        return LN2_32 if self.family == "C" else self.D ** -0.5

    @property
    def cexp(self):
        """log2 units per unit of q . k (the reference's multiplier)"""
        if self.kernel == "spatial" and self.pre:
            return 1.0
        if self.kernel == "temporal":                 # st * scale in fp32, then __expf
            return float(np.float32(self.scale)) * math.log2(math.e)
        return cexp_of(self.scale)

    @property
    def id(self):
        dims = f"{self.nb}x{self.pos}x{self.heads}" if self.kernel == "temporal" else f"{self.nb}x{self.heads}"
        s = f"{self.kernel}{self.D}-{self.family}-{dims}-{self.Sq}" + (f"x{self.Sk}" if self.Sk != self.Sq else "")
        return s + ("-pre" if self.pre else "") + ("-nqb2" if self.nqb == 2 else "") + ("-fused" if self.fused else "") + ("-lse" if self.lse else "")


# ------------------------------------------------------------------------------------------------- the case lists
SPATIAL_S = (1, 63, 64, 65, 191, 192, 193, 449)                   # 192 (128) queries per workgroup, 64-key tiles; 3 x 3 groups: a second round
GENERAL_S = ((1, 1), (1, 17), (63, 31), (64, 32), (65, 33), (130, 97), (5, 3))
D512_S = ((1, 1), (127, 31), (128, 32), (129, 33), (64, 65))
SHORT_F, LONG_F = (1, 2, 15, 16, 17, 31, 32), (33, 48, 49, 127, 128)
TEMPORAL_DIMS = ((1, 5, 1), (2, 3, 3))                            # (clips, positions, heads): 5 and 18 tasks


def spatial_cases():
    out = []
    for fam in FAMILIES:
        for pre in (0, 1):
            out += [Case("spatial", fam, 3, 3, S, S, 64, pre=pre) for S in SPATIAL_S]
            out += [Case("spatial", fam, 3, 3, S, S, 64, pre=pre, nqb=2) for S in (129, 449)]
    out += [Case("spatial", "C", 1, 1, 705, 705, 64, pre=pre) for pre in (0, 1)]
    out += [Case("spatial", "B", 1, 1, 1024, 1024, 64, pre=pre) for pre in (0, 1)]
    return out


def general_cases():
    out = []
    for D, lse in ((64, False), (80, False), (128, False), (64, True), (128, True)):
        for fam in ("A0", "Am", "B"):
            out += [Case("general", fam, 3, 3, sq, sk, D, lse=lse) for sq, sk in GENERAL_S]      # separate buffers: cross-attention
            out.append(Case("general", fam, 3, 3, 130, 130, D, fused=True, lse=lse))
        out.append(Case("general", "C", 3, 3, 130, 289, D, lse=lse))
    return out


def d512_cases():
    out = []
    for fam in ("A0", "Am", "B"):
        out += [Case("d512", fam, 3, 1, sq, sk, 512) for sq, sk in D512_S]
        out.append(Case("d512", fam, 9, 1, 129, 33, 512))
    out.append(Case("d512", "C", 3, 1, 129, 289, 512))
    return out


def temporal_cases():
    return [Case("temporal", fam, B, heads, Fr, Fr, D, pos=S) for D in (64, 128) for fam in ("A0", "Am", "B") for Fr in SHORT_F + LONG_F
            for B, S, heads in TEMPORAL_DIMS]


def all_cases():
    return spatial_cases() + general_cases() + d512_cases() + temporal_cases()


# ------------------------------------------------------------------------------------------------- generators
def pi_of(Sq, Sk):
    return (7 * torch.arange(Sq) + 3) % Sk


def _values(g, *shape):
    """integers in {+-1 .. +-8}, no zeros"""
    return (torch.randint(1, 9, shape, generator=g) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)).half()


def tile_bases(ntiles):
    b = [0]
    for t in range(1, ntiles):
        b.append(b[-1] + INC[(t - 1) % len(INC)])
    return torch.tensor(b)


@functools.lru_cache(maxsize=None)
def data(family, G, Sq, Sk, D):
    """(q, k, v) fp16 on the CPU; group g from the seed D + Sk + 100003 g.  Never modified."""
    qs, ks, vs = [], [], []
    for grp in range(G):
        g = torch.Generator().manual_seed(D + Sk + 100003 * grp)
        v = _values(g, Sk, D)
        if family == "A0":
            q, k = torch.zeros(Sq, D), _values(g, Sk, D).float()
        elif family == "Am":
            u = (torch.randint(0, 2, (D,), generator=g) * 2 - 1).float()
            q, k = (2 * u).expand(Sq, D), (-2 * u).expand(Sk, D)
        elif family == "B":
            k = 4.0 * (torch.randint(0, 2, (Sk, D), generator=g) * 2 - 1)
            q = k[pi_of(Sq, Sk)]
        else:
            j = torch.arange(Sk)
            k = torch.randint(0, 6, (Sk, D), generator=g).float()
            k[:, 0] = (tile_bases((Sk + 63) // 64)[j // 64] - 9 * (j % 8 == 5)).float()
            q = torch.zeros(Sq, D)
            q[:, 0] = 1.0
            q[torch.arange(Sq), torch.randint(1, D, (Sq,), generator=g)] = 1.0
        qs.append(q.half())
        ks.append(k.half())
        vs.append(v)
    return torch.stack(qs).contiguous(), torch.stack(ks).contiguous(), torch.stack(vs).contiguous()


def problem(case):
    return data(case.family, case.groups, case.Sq, case.Sk, case.D)


@functools.lru_cache(maxsize=None)
def _reference(family, G, Sq, Sk, D, cexp):
    q, k, v = (t.double() for t in data(family, G, Sq, Sk, D))
    s = q @ k.transpose(1, 2) * cexp
    m = s.amax(-1, keepdim=True)
    p = torch.exp2(s - m)
    l = p.sum(-1, keepdim=True)
    return s, (p @ v) / l, (m + torch.log2(l))[..., 0]


def scores(case):
    """fp64 scores in log2 units [G, Sq, Sk]"""
    return _reference(case.family, case.groups, case.Sq, case.Sk, case.D, case.cexp)[0]


def reference(case):
    """fp64 softmax(scores) V [G, Sq, D] and log2 sum 2^score [G, Sq]; computed once, never modified."""
    return _reference(case.family, case.groups, case.Sq, case.Sk, case.D, case.cexp)[1:]


def self_check(case):
    """The preconditions a family's argument rests on, asserted on the fp64 scores.  -> a dict of the figures"""
    q, k, v = problem(case)
    s = scores(case)
    assert bool((v != 0).all()) and float(v.abs().max()) == 8 and bool((v == v.round()).all())
    info = {}
    if case.family in ("A0", "Am"):
        assert bool((s == s[:, :, :1]).all()), "all scores of a query are equal"
        raw = q.double() @ k.double().transpose(1, 2)
        assert bool((raw == raw.round()).all())
        if case.family == "Am":
            assert float(s.max()) <= -MARGIN_B, float(s.max())
        info["score"] = float(s.max())
    elif case.family == "B":
        pi = pi_of(case.Sq, case.Sk)
        lead = s.gather(2, pi.expand(case.groups, -1)[..., None])[..., 0]
        rest = s.clone()
        rest.scatter_(2, pi.expand(case.groups, -1)[..., None], -math.inf)
        margin = float((lead - rest.amax(-1)).min())
        assert margin >= MARGIN_B, margin
        info["margin"] = margin
    else:
        assert case.cexp == 1.0 and np.float32(LN2_32) * LOG2E32 == np.float32(1.0)
        assert bool((s == s.round()).all()), "integer scores"
        nt = (case.Sk + 63) // 64
        tmax = torch.stack([s[:, :, 64 * t:64 * (t + 1)].amax(-1) for t in range(nt)], -1)            # [G, Sq, tiles]
        run = torch.cummax(tmax, -1)[0]
        for t in range(nt):
            low = s[:, :, 64 * t:64 * (t + 1)].amin(-1)
            assert bool((low >= run[..., t] - SPAN_C).all()), "P stays in fp16's normal range under a running maximum"
            if t:
                assert bool((low >= run[..., t - 1] - SPAN_C).all()), "... and against the earlier tiles' maximum"
        m, cross, stay = tmax[..., 0].clone(), torch.zeros_like(tmax[..., 0]), torch.zeros_like(tmax[..., 0])
        for t in range(1, nt):
            hit = tmax[..., t] - m > THR
            cross, stay = cross + hit, stay + ~hit
            m = torch.where(hit, tmax[..., t], m)
        info["crossings"], info["stays"] = int(cross.min()), int(stay.min())
        if nt >= 5:
            assert info["crossings"] >= 2 and info["stays"] >= 2, info
    return info


# ------------------------------------------------------------------------------------------------- checkers
def ulp16(x):
    """2^(max(floor(log2 |x|), -14) - 10)"""
    _, e = torch.frexp(x.abs().double())                       # |x| = m 2^e, m in [0.5, 1)
    fl = torch.where(x == 0, torch.full_like(e, -14), e - 1).clamp(min=-14)
    return torch.exp2((fl - 10).double())


def bits(t):
    return t.contiguous().view(torch.int16)


def _fraction(o, ref, bound, zero_exact):
    o = o.double()
    if not bool(torch.isfinite(o).all()):
        return math.inf
    frac = (o - ref).abs() / bound
    if zero_exact:
        frac = torch.where(ref == 0, torch.where(o == 0, 0.0, math.inf).double(), frac)
    return float(frac.max())


@dataclasses.dataclass
class Verdict:
    ok: bool
    text: str


def judge(case, o, lse=None):
    """o [G, Sq, D] fp16 (and lse [G, Sq] fp32) against the family's bound.  -> Verdict; the text names the worst deviation as a fraction
    of the bound (A, C, lse) or the number of elements that are not bit-equal (B)."""
    ref, lref = reference(case)
    assert o.dtype == torch.float16 and o.shape == ref.shape
    if case.family in ("A0", "Am"):
        w = _fraction(o, ref, 0.5 * ulp16(ref) + 2.0 ** -21 * ref.abs(), True)
        ok, text = w <= 1.0, f"worst {w:.3f} of the bound"
    elif case.family == "B":
        want = problem(case)[2][:, pi_of(case.Sq, case.Sk)]
        bad = int((bits(o) != bits(want)).sum())
        ok, text = bad == 0, f"{bad} of {o.numel()} elements not bit-equal"
    else:
        vmax = float(problem(case)[2].abs().max())
        w = _fraction(o, ref, 0.5 * ulp16(ref) + (math.ceil(case.Sk / 32) + 8) * 2.0 ** -23 * vmax, False)
        ok, text = w <= 1.0, f"worst {w:.3f} of the bound"
    if lse is not None:
        assert lse.dtype == torch.float32 and lse.shape == lref.shape
        w = _fraction(lse, lref, 2.0 ** -18 * lref.abs().clamp(min=1.0), False)
        ok, text = ok and w <= 1.0, text + f"; lse worst {w:.3f} of the bound"
    return Verdict(ok, text)


# ------------------------------------------------------------------------------------------------- the kernels' rounding points on the CPU
def expressible(case, fault):
    if fault in ("drop_last", "dup_key", "swap_v"):
        return case.Sk >= 2
    if fault == "pad_unmasked":
        return case.Sk % case.tile != 0
    if fault == "shift_q":
        return case.Sq >= 2 and case.Sk >= 2
    if fault == "neighbour_k":
        return case.groups >= 2 and case.Sk >= 2
    return True                                                 # skip_rebase: emulate() says (None when no maximum moves)


def emulate(case, fault=None, softmax=None):
    """fp32 scores, P = 2^(s - m) rounded to fp16, fp32 accumulation of P V and of the row sum (the fp16 P's in the spatial kernel, the
    unrounded ones elsewhere), fp32 reciprocal, fp16 store - as forward_model of tests/test_temporal_attn_long_gpu.py, tile by tile:
    ``softmax`` = "online" (running maximum), "defer" (re-base only when a tile's maximum exceeds the reference maximum by more than THR)
    or "full" (one tile: the temporal kernels).  ``fault``: one of FAULTS.  -> (o fp16 [G, Sq, D], lse fp32 [G, Sq], tiles after the
    first in which some maximum moved), or None where the fault cannot be expressed."""
    softmax = softmax or case.softmax
    if fault and not expressible(case, fault):
        return None
    q, k, v = (t.float() for t in problem(case))
    Sk = case.Sk
    if fault == "drop_last":
        k, v = k[:, :-1], v[:, :-1]
    elif fault == "dup_key":
        k, v = torch.cat([k, k[:, -1:]], 1), torch.cat([v, v[:, -1:]], 1)
    elif fault == "pad_unmasked":
        n = case.tile - Sk % case.tile
        k, v = torch.cat([k, torch.zeros_like(k[:, :n])], 1), torch.cat([v, torch.zeros_like(v[:, :n])], 1)
    elif fault == "swap_v":
        j = int(pi_of(case.Sq, Sk)[0]) if case.family == "B" else (Sk - 1 if (Sk - 1) & 1 else Sk - 2)
        v = v.clone()
        v[:, [j, j ^ 1]] = v[:, [j ^ 1, j]]
    elif fault == "neighbour_k":
        k = torch.roll(k, -1, 0)
    s = (q @ k.transpose(1, 2)) * torch.tensor(case.cexp, dtype=torch.float32)
    n = k.shape[1]
    step = n if softmax == "full" else case.tile if softmax == "defer" else min(case.tile, 32)
    sum_half = case.kernel == "spatial"

    def sweep(skip_at):
        m = torch.full(s.shape[:2], -math.inf)
        l, O, moved = torch.zeros(s.shape[:2]), torch.zeros(s.shape[:2] + (v.shape[2],)), []
        for t, j0 in enumerate(range(0, n, step)):
            st = s[:, :, j0:j0 + step]
            mt = st.amax(-1)
            m_new = torch.where(mt - m > THR, mt, m) if softmax == "defer" and t else torch.maximum(m, mt)
            alpha = torch.exp2(m - m_new)
            p = torch.exp2(st - m_new[..., None])
            p16 = p.half().float()
            if t and bool((alpha != 1).any()):
                moved.append(t)
            if t == skip_at:
                alpha = torch.ones_like(alpha)
            l = l * alpha + (p16 if sum_half else p).sum(-1)
            O = O * alpha[..., None] + p16 @ v[:, j0:j0 + step]
            m = m_new
        return (O * (1.0 / l)[..., None]).half(), m + torch.log2(l), moved

    o, lse, moved = sweep(-1)
    if fault == "skip_rebase":
        if not moved:
            return None
        o, lse, _ = sweep(moved[-1])
    if fault == "shift_q":
        o, lse = torch.roll(o, -1, 1), torch.roll(lse, -1, 1)
    return o, lse, moved


# ------------------------------------------------------------------------------------------------- layouts (shared with the GPU runner)
def to_rows(case, x):
    """[G, S, D] -> the kernels' row-major [rows, heads D]: row = batch S + token (temporal: (clip F + frame) positions + position)."""
    S, D = x.shape[1], x.shape[2]
    if case.kernel == "temporal":
        return x.view(case.nb, case.pos, case.heads, S, D).permute(0, 3, 1, 2, 4).reshape(case.nb * S * case.pos, case.heads * D).contiguous()
    return x.view(case.nb, case.heads, S, D).permute(0, 2, 1, 3).reshape(case.nb * S, case.heads * D).contiguous()


def from_rows(case, y, S):
    """inverse of to_rows"""
    D = case.D
    if case.kernel == "temporal":
        return y.reshape(case.nb, S, case.pos, case.heads, D).permute(0, 2, 3, 1, 4).reshape(case.groups, S, D).contiguous()
    return y.reshape(case.nb, S, case.heads, D).permute(0, 2, 1, 3).reshape(case.groups, S, D).contiguous()


def report(line: str):
    print(line)
    path = os.environ.get("PT_ATTN_EXACT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")
