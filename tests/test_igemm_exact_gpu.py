"""pt_igemm_f16 (csrc/igemm.hip, csrc/igemm_tail.h) - every launch route, tail variant, gather, split-K - on the MI355X against fp64,
BIT FOR BIT.

The argument.  The operands are fp16 and the accumulators fp32.  Activations are drawn uniformly from {+-1, +-2, +-3}, weights from
{+-1, +-2}; bias, residual, row vector and blend are small integers.  Every partial sum is an integer below 2^24, so the order of
summation does not matter - K tiles of 64, MFMA lanes, the 8- or 10-phase loop, split-K slabs added in order: the fp32 accumulator is
THE integer.  With alpha, out_scale and cs_scale powers of two (alpha = 0.25, so 1 - alpha = 0.75) every step of the header's epilogue
formula (include/posetraj_hip.h:41-47) is exact in fp32, the fp16 output is the single correct rounding of a known rational, and
out_lo = fp16(v - fp16(v)) is the single rounding of an exactly known difference.  There is no tolerance to choose: the tests assert
bitwise equality with an fp64 CPU reference.  One halo pixel read as data, one row stored twice at a chunk seam, one 8-column segment
with the neighbouring frame's row vector, one K tile dropped in one split, a low half from the wrong pass each change an output.

Every case first asserts its precondition on the reference (problem()): the epilogue chain is evaluated step by step in fp64 and in
fp32 on the CPU and must agree at every step - which holds exactly when each intermediate fits 24 bits - and |out| < 60000 for an fp16
output; out_scale = 2^-k is chosen so that this holds, the reference is never clipped.  (Cases that write out_lo, and the runs they are
compared with, take their bias from the odd multiples of 2^-6 below 4 instead of integers: v then has more than eleven significant
bits wherever |v| >= 32 and the low half is not identically zero.  The same preconditions are asserted.)

GEGLU is exact too, with a saturated gate.  pt_gelu_erf2 (pt_common.h:78-89) computes relu(g) - (|g| / 2) 2^(-q(z) z), z = |g| / sqrt 2,
q increasing, q z ~ 52.3 at |g| = 8: for |g| >= 8 the second term is below 2^-50 |g|, the fp32 result is g exactly for g > 0 and for
g < 0 a negative number (or zero) so small that its product with any value below 2^24 rounds to a signed zero in fp16.  The gate half
has weights in {+-16, +-32} and gate bias 8: every gate accumulator is = 8 (mod 16), so |g| >= 8 always.  Expected:
fp16(out_scale * val * max(g, 0)); preconditions |val * g| < 2^24 and |g| >= 8 on the reference.  GEGLU CASES ONLY are compared after
mapping -0 to +0 - the one relaxation in this file; NaN still fails.  This rests on the fit's coefficients as committed:
tests/test_igemm_exact_cpu.py evaluates the formula in numpy fp32 for every gate value that occurs and is what says so if they change.
SiLU (act == 2) has no exact form and stays with the rel-L2 tests of tests/test_kernels_gpu.py.

Guarded buffers (guarded() of tests/test_gemm_exact_gpu.py).  Every pointer the kernel is given lives in a NaN-filled buffer: x0, x1,
the whole packed weight image, bias, res, res_lo, vec, blend, out, out_lo and the split-K workspace.  The pitch is columns + 8 (x1:
+ 16, so the two sources differ; the weight image and the bias have the pitch the kernel assumes), 64 NaN rows lie in front and behind.
out and out_lo start NaN-filled, or hold the residual when they alias it for res_post.  After the call every element outside
[M, n_out] must still be the NaN it was, every element inside bit-equal to the reference.  Padded taps and rows >= M read the zero
page, so a NaN in the output is a read outside the operand.  The workspace is NaN-filled, exactly pt_igemm_splitk_ws_bytes long, with
a guard tail that must survive.

Calls go through the raw binding (hip.IgemmParams, hip.lib()); weights and bias come from packing.pack_linear / pack_conv2d /
pack_conv2d_upfold / pack_conv_t3.  The hooks (pt_igemm_force_config, pt_igemm_set_tuning) are restored in `finally` (hooks()).

Routes.  pt_igemm_f16 has eleven launch routes (igemm.hip:997-1014): cfg 0 fast (igemm8_kernel) and generic-K (the plain CfgBig loop),
cfg 1, 2, 4 and 5 each fast and generic, cfg 3 fast (igemm10_kernel); a generic-K case under forced cfg 3 falls back to cfg 1, or to
cfg 0 for GEGLU (:942).  A route is written cfg<n>f / cfg<n>g.  Tail variants are named by tail_variant() (igemm_tail.h:361), mirrored
here: res_post with a lone residual is V_P1, res + vec + blend is V_EW with or without out_lo.

recipe() is the kernel's index arithmetic in torch fp32 on the CPU - row_origin, tap_source, walk_step, class_of / out_row - and
tests/test_igemm_exact_cpu.py holds it against the fp64 references without a GPU, confirms every plan this file names with
pt_igemm_plan, and shows that planted breaks are noticed.

One line per run is printed: case, route, variant, number of elements that differ; with PT_IGEMM_EXACT=<file> it is also appended to
that file (profiles/r12/igemm_exact.txt is such a run)."""
import contextlib
import ctypes
import dataclasses
import functools
import os
import zlib
from typing import Optional

import pytest
import torch
import torch.nn.functional as F

from tests.test_gemm_exact_gpu import NAN, bits, guarded, ints, wints

pytestmark = pytest.mark.gpu

BK = 64                               # igemm_tail.h:11  the K tile
X1_PAD = 16                           # x1's pitch pad: the two sources get different pitches
WS_TAIL = 1024                        # NaN floats behind the split-K workspace
ALPHA = 0.25                          # AlphaBlender weight: alpha and 1 - alpha are exact in binary
CS_COLS, CS_SCALE = 320, 4.0
VG = 77                               # vec_mode 1: a period that straddles chunks and tiles
VFS, VS, VB = 150, 30, 90             # vec_mode 2: (m / 150) * 30 + m % 30 reaches 119 at M = 600 and wraps at 90 (vec_index)
FAST_ROUTES = ((0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (5, 5))            # (forced cfg, the cfg the plan must name)
GENERIC_ROUTES = ((0, 0), (1, 1), (2, 2), (3, 1), (4, 4), (5, 5))         # :942  forced 3 falls back to 1
GEGLU_FAST = ((0, 0), (2, 2), (3, 3), (4, 4))                             # cfg 1 and cfg 5 refuse GEGLU (:943-944)
GEGLU_GENERIC = ((0, 0), (2, 2), (3, 0), (4, 4))                          # :942  forced 3 falls back to 0
AUTO = ((-1, 5),)                                                         # :941  N <= 96 on the automatic plan
BM = {0: 256, 1: 128, 2: 128, 3: 256, 4: 128, 5: 256}
BN = {0: 256, 1: 320, 2: 128, 3: 320, 4: 160, 5: 32}
WAVE_W = {0: 128, 1: 80, 2: 64, 3: 160, 4: 160, 5: 32}                    # columns per wave (Cfg<WM, WN, TM, TN>: TN * 16)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    kind: str                         # lin | conv (3 x 3) | up1 (3 x 3 on the nearest-2x source) | fold (upsample2x == 2) | t3 ((3, 1) temporal)
    dims: tuple                       # lin: (M, n_out, K); the others: (Nimg, Hin, Win, C0, C1, Co)
    stride: int = 1
    pad: int = 1
    out_hw: Optional[tuple] = None    # output extent when it is not the symmetric-padding one (Downsample2D)
    geglu: bool = False
    res: bool = False
    res_lo: bool = False
    vec: int = 0                      # vec_mode
    blend: bool = False
    res_post: bool = False            # in place: out aliases res
    out_lo: bool = False
    out_f32: bool = False
    cs: bool = False                  # cs_cols = 320, cs_scale = 4
    out_scale: float = 0.5
    opad: int = 8                     # pitch pad of out / out_lo / res / res_lo
    frac_bias: bool = False           # bias from the odd multiples of 2^-6 (the out_lo cases)
    group_m: int = 0                  # pt_igemm_set_tuning
    routes: tuple = FAST_ROUTES
    splits: int = 1                   # what the automatic plan must split into when the workspace is offered
    operands_of: Optional[str] = None # draw the operands of the case of that name (the same layer through another mode)

    @property
    def variant(self):
        """tail_variant() of igemm_tail.h:361"""
        nside = int(self.res) + int(self.res_lo) + int(self.vec > 0) + int(self.blend)
        if self.geglu:
            return "G0" if nside == 0 and not self.out_lo else "GEW"
        if nside > 2:
            return "EW"
        return ("W" if self.out_lo else "P") + str(nside)


def lin(name, M, N, K, **kw):
    return Case(name, "lin", (M, N, K), **kw)


def conv(name, kind, *dims, **kw):
    return Case(name, kind, dims, **kw)


# ------------------------------------------------------------------------------------------------- section 1: linear layers, every route
LINEAR = [lin("lin_1tile", 300, 320, 64),                       # one, two and three K tiles: prologue and drain of the 8- and 10-phase
          lin("lin_2tiles", 300, 320, 128),                     # loops, whose copies run two tiles ahead
          lin("lin_3tiles", 300, 320, 192),
          lin("lin_ragged", 600, 400, 320),                     # ragged last M tile at 256 and 128; N = 400: fast-tail and element-wise waves
                                                                # in one workgroup (igemm_tail.h:192)
          lin("lin_whole", 600, 640, 128),                      # whole waves everywhere: the 16-byte fast tail
          lin("lin_2rows", 2, 64, 128, res=True),               # two rows: every side load clamped to M - 1 (:200)
          lin("lin_k72", 300, 320, 72, routes=GENERIC_ROUTES),  # generic K: kvalid (igemm.hip:181); the NaN pitch pad lies behind channel 72
          lin("lin_n20", 300, 20, 64),                          # vec_ok false by width: the element-wise path on every route
          lin("lin_n4_f32", 300, 4, 64, out_f32=True),
          lin("lin_pitch4", 600, 640, 128, res=True, opad=4),   # vec_ok false by pitch alone
          lin("lin_group", 1320, 640, 64, group_m=4),           # six M tiles of 256: the second rasterisation group has gm = 2 (tile_of, :39-41)
          lin("geglu_k72", 300, 320, 72, geglu=True, out_scale=2.0 ** -5, routes=GEGLU_GENERIC)]

# ------------------------------------------------------------------------------------------------- section 2: tail variants
TAIL_SHAPES = {"whole": (600, 640, 128), "mixed": (600, 400, 128)}        # the fast tail; fast and element-wise waves side by side
TAILS = {"P0": dict(cs=True),
         "P1_res": dict(res=True),
         "P1_vec1": dict(vec=1),
         "P1_vec2": dict(vec=2),
         "P1_blend": dict(blend=True),
         "P1_post": dict(res=True, res_post=True, out_scale=2.0),                       # in place
         "P2_res_vec": dict(res=True, vec=1),
         "P2_res_blend": dict(res=True, blend=True),
         "P2_res_lo": dict(res=True, res_lo=True),
         "P2_post_lo": dict(res=True, res_lo=True, res_post=True, out_scale=2.0),
         "EW": dict(res=True, vec=1, blend=True),
         "W0": dict(cs=True, out_lo=True),
         "W1_res": dict(res=True, out_lo=True),
         "W1_vec1": dict(vec=1, out_lo=True),
         "W1_blend": dict(blend=True, out_lo=True),
         "W1_post": dict(res=True, res_post=True, out_scale=2.0, out_lo=True),
         "W2_res_vec": dict(res=True, vec=1, out_lo=True),
         "W2_res_blend": dict(res=True, blend=True, out_lo=True),
         "W2_res_lo": dict(res=True, res_lo=True, out_lo=True),
         "W2_post_lo": dict(res=True, res_lo=True, res_post=True, out_scale=2.0, out_lo=True),
         "EW_lo": dict(res=True, vec=1, blend=True, out_lo=True),
         "G0": dict(geglu=True, out_scale=2.0 ** -5, routes=GEGLU_FAST),
         "GEW": dict(geglu=True, res=True, out_scale=2.0 ** -5, routes=GEGLU_FAST)}


def tail_case(shape, tail):
    kw = TAILS[tail]
    M, N, K = TAIL_SHAPES[shape]
    if kw.get("geglu") and shape == "whole":
        N = 320                                                   # 640 packed columns, 320 out (mixed: 800 packed, 400 out: N % 32 == 0)
    return lin(f"tail_{shape}_{tail}", M, N, K, frac_bias=kw.get("out_lo", False), **kw)


TAIL_CASES = [tail_case(s, t) for s in TAIL_SHAPES for t in TAILS]

# ------------------------------------------------------------------------------------------------- section 3: gathers
GATHERS = [conv("c3_2x7x5", "conv", 2, 7, 5, 64, 0, 320),
           conv("c3_3x19x23", "conv", 3, 19, 23, 64, 0, 320),                           # image boundaries inside a tile
           conv("c3_1x1_images", "conv", 70, 1, 1, 64, 0, 64),                          # eight taps fully masked: the centre tap alone
           conv("c3_two_sources", "conv", 2, 7, 5, 64, 64, 320),                        # fast: walk_step's source switch
           conv("c3_two_sources_c24_c8", "conv", 2, 7, 5, 24, 8, 320, routes=GENERIC_ROUTES),
           conv("c3_stride2_odd", "conv", 3, 9, 7, 64, 0, 320, stride=2),
           conv("c3_downsample", "conv", 2, 10, 12, 64, 0, 320, stride=2, pad=0, out_hw=(5, 6)),    # Downsample2D: taps beyond the input read zeros
           conv("up1_c64", "up1", 2, 5, 6, 64, 0, 320),
           conv("up1_c16", "up1", 2, 5, 6, 16, 0, 320, routes=GENERIC_ROUTES),
           conv("t3_5_frames", "t3", 2, 5, 300, 64, 0, 320),                            # foldx: the image (F, S) of 2 clips
           conv("t3_1_frame", "t3", 2, 1, 300, 64, 0, 320),                             # centre tap only
           conv("wide_image", "conv", 1, 3, 2400, 8, 0, 16, stride=2, routes=GENERIC_ROUTES),   # Wout = 1200: the signed 16-bit pair (:68, :79), ix = -1
           conv("narrow_co3", "conv", 2, 7, 5, 64, 0, 3, routes=AUTO),
           conv("narrow_co4", "conv", 2, 7, 5, 64, 0, 4, routes=AUTO),
           conv("narrow_co4_f32", "conv", 2, 7, 5, 64, 0, 4, out_f32=True, routes=AUTO),
           conv("narrow_co16", "conv", 2, 7, 5, 64, 0, 16, routes=AUTO),
           conv("narrow_co96", "conv", 2, 7, 5, 64, 0, 96, routes=AUTO)]
# the folded upsampler, and the same layer on the same operands in mode 1
FOLDED = [conv("fold_3x9x7", "fold", 3, 9, 7, 64, 0, 320),                 # 189 class rows: one ragged class tile
          conv("fold_2x17x16", "fold", 2, 17, 16, 64, 0, 320)]             # 544 class rows: class_tiles = 3 at 256, ragged


def mode1_twin(c):
    return dataclasses.replace(c, name=c.name.replace("fold", "up1"), kind="up1", operands_of=c.name)


# ------------------------------------------------------------------------------------------------- section 4: split-K
SPLIT_EPILOGUES = {"bias": dict(), "res_vec": dict(res=True, vec=1), "post": dict(res=True, res_post=True, out_scale=2.0),
                   "out_lo": dict(out_lo=True, frac_bias=True)}
SPLITK = ([lin(f"splitk_lin_{k}", 300, 320, 3200, splits=8, routes=((-1, 3),), **kw) for k, kw in SPLIT_EPILOGUES.items()] +      # 50 K tiles: 7 x 7 + 1 (:501-503)
          [conv(f"splitk_conv_{k}", "conv", 3, 10, 10, 384, 0, 320, splits=9, routes=((-1, 3),), **kw) for k, kw in SPLIT_EPILOGUES.items()])   # 54 K tiles: 9 x 6

ALL_CASES = LINEAR + TAIL_CASES + GATHERS + FOLDED + [mode1_twin(c) for c in FOLDED] + SPLITK
CASES = {c.name: c for c in ALL_CASES}
assert len(CASES) == len(ALL_CASES)


def report(line: str):
    print(line)
    path = os.environ.get("PT_IGEMM_EXACT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


# ------------------------------------------------------------------------------------------------- problems and references (CPU)
def geometry(c):
    """The pt_igemm_params geometry of a case, as a dict."""
    if c.kind == "lin":
        M, n_out, K = c.dims
        return dict(C0=K, C1=0, Nimg=M, Hin=1, Win=1, Hout=1, Wout=1, KH=1, KW=1, stride=1, pad_h=0, pad_w=0, up=0, M=M, n_out=n_out,
                    N=2 * n_out if c.geglu else n_out, K=K)
    Nimg, H, W, C0, C1, Co = c.dims
    KH, KW, ph, pw, up = {"conv": (3, 3, c.pad, c.pad, 0), "up1": (3, 3, 1, 1, 1), "fold": (2, 2, 0, 0, 2), "t3": (3, 1, 1, 0, 0)}[c.kind]
    Hs, Ws = (2 * H, 2 * W) if up else (H, W)
    Hout, Wout = (Hs, Ws) if up == 2 else ((Hs + 2 * ph - KH) // c.stride + 1, (Ws + 2 * pw - KW) // c.stride + 1)
    if c.out_hw:
        Hout, Wout = c.out_hw
    return dict(C0=C0, C1=C1, Nimg=Nimg, Hin=H, Win=W, Hout=Hout, Wout=Wout, KH=KH, KW=KW, stride=c.stride, pad_h=ph, pad_w=pw, up=up,
                M=Nimg * Hout * Wout, n_out=Co, N=Co, K=KH * KW * (C0 + C1))


def is_fast(c):
    """Plan::fast (igemm.hip:934): channel-aligned K tiles"""
    g = geometry(c)
    return (g["C0"] + g["C1"]) % BK == 0 and g["C0"] % BK == 0 and g["K"] % BK == 0


def route_name(cfg, fast):
    return f"cfg{cfg}{'f' if fast else 'g'}"


def rows_of(t):
    """[N, C, H, W] -> channels-last rows [N H W, C]"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def vec_rows(c, M, broken=None):
    """vec_index (igemm_tail.h:88) of every output row; ``broken`` = "vec_mod": without the % vB."""
    m = torch.arange(M)
    if c.vec == 1:
        return m // VG
    idx = (m // VFS) * VS + m % VS
    return idx if broken == "vec_mod" else idx % VB


def exact_chain(t, steps):
    """Evaluate ``steps`` (functions (value, dtype) -> value) on t in fp64 and in fp32; the two must agree after every step - which they
    do exactly when every intermediate fits the 24 bits of an fp32 significand.  -> the fp64 result"""
    a64, a32 = t.double(), t.float()
    assert torch.equal(a32.double(), a64)
    for f in steps:
        a64, a32 = f(a64, torch.float64), f(a32, torch.float32)
        assert a32.dtype == torch.float32 and torch.equal(a32.double(), a64)
    return a64


@functools.lru_cache(maxsize=None)
def problem(c):
    """Operands, packed weights and the fp64 reference of a case, preconditions asserted.  -> dict: geo, x0, x1, pack, res, res_lo, vec,
    blend (fp16 CPU tensors or None), t64 (product + bias, [M, N] un-interleaved; gathers and GEGLU), gate (the GEGLU gate values), out / out_lo (what the
    kernel must write, in the output's dtype)."""
    from posetraj_amd import packing
    g = geometry(c)
    M, N, n_out, Ct = g["M"], g["N"], g["n_out"], g["C0"] + g["C1"]
    seed = zlib.crc32((c.operands_of or c.name).encode()) % 1000003
    x = ints(g["Nimg"] * g["Hin"] * g["Win"], Ct, seed=seed)
    wshape = {"lin": (N, Ct), "t3": (N, Ct, 3, 1, 1)}.get(c.kind, (N, Ct, 3, 3))
    w = wints(*wshape, seed=seed + 1)
    gb = torch.Generator().manual_seed(seed + 2)
    if c.frac_bias:
        b = (2 * torch.randint(0, 128, (N,), generator=gb) + 1).float() / 64 * (torch.randint(0, 2, (N,), generator=gb) * 2 - 1)
    else:
        b = ints(N, seed=seed + 2).float()
    wmax = 2
    if c.geglu:                                                   # rows [value | gate]: gate weights +-16 / +-32, gate bias 8
        w[n_out:] *= 16
        b[n_out:] = 8
        wmax = 32
    assert g["K"] * 3 * wmax * (4 if c.kind == "fold" else 1) + 4 < 2 ** 24      # every partial sum is an integer (+ bias) below 2^24
    xd, wd = x.double(), w.double()
    if c.kind == "lin":
        t = xd @ wd.t()
        pack = packing.pack_linear(w, b, "cpu", geglu=c.geglu)
    else:
        x4 = xd.view(g["Nimg"], g["Hin"], g["Win"], Ct).permute(0, 3, 1, 2)
        if c.kind == "t3":
            t = rows_of(F.conv3d(x4.unsqueeze(-1), wd, padding=(1, 0, 0))[..., 0])
            pack = packing.pack_conv_t3(w, b, "cpu")
        else:
            if g["up"]:
                x4 = F.interpolate(x4, scale_factor=2.0, mode="nearest")
            if c.out_hw:                                          # Downsample2D(padding=0): F.pad(x, (0, 1, 0, 1)) + stride-2 convolution
                assert c.pad == 0
                x4 = F.pad(x4, (0, 1, 0, 1))
            t = rows_of(F.conv2d(x4, wd, stride=c.stride, padding=1 if g["up"] else c.pad))
            pack = packing.pack_conv2d_upfold(w, b, "cpu") if c.kind == "fold" else packing.pack_conv2d(w, b, "cpu", stride=c.stride, padding=c.pad)
    assert t.shape == (M, N) and pack.N == N and pack.K == g["K"] and bool((pack.w.float().abs() <= 32).all())
    t64 = t + b.double()
    side = lambda *shape, k: ints(*shape, seed=seed + k)
    res = side(M, n_out, k=3) if c.res else None
    res_lo = wints(M, n_out, seed=seed + 4).half() * 0.25 if c.res_lo else None        # {+-0.25, +-0.5}
    vec = side(int(vec_rows(c, M).max()) + 1, n_out, k=5) if c.vec else None
    blend = side(M, n_out, k=6) if c.blend else None
    assert not c.vec or c.vec == 1 or vec.shape[0] == VB
    steps, gate, v0 = [], None, t64
    if c.geglu:
        val, gate = t64[:, :n_out], t64[:, n_out:]
        assert float((val * gate).abs().max()) < 2 ** 24 and float(gate.abs().min()) >= 8 and bool((gate % 16 == 8).all())
        v0 = val * gate.clamp(min=0)
    if c.res and not c.res_post:
        steps.append(lambda a, dt: a + res.to(dt))
        if c.res_lo:
            steps.append(lambda a, dt: a + res_lo.to(dt))
    if c.vec:
        rows = vec[vec_rows(c, M)]
        steps.append(lambda a, dt: a + rows.to(dt))
    scale = torch.full((n_out,), c.out_scale, dtype=torch.float64)
    if c.cs:
        scale[:CS_COLS] *= CS_SCALE
    pre = exact_chain(v0, steps)
    if c.blend:                                                   # each product alone, then the lerp
        exact_chain(blend, [lambda a, dt: ALPHA * a])
        exact_chain(pre, [lambda a, dt: (1.0 - ALPHA) * a])
        pre = exact_chain(pre, [lambda a, dt: ALPHA * blend.to(dt) + (1.0 - ALPHA) * a])
    post = [lambda a, dt: a * scale.to(dt)]
    if c.res_post:
        post.append(lambda a, dt: a + res.to(dt))
        if c.res_lo:
            post.append(lambda a, dt: a + res_lo.to(dt))
    v = exact_chain(pre, post)
    if c.res_lo:                                                  # the element-wise tail and the split-K reducer add res + res_lo first
        exact_chain(res, [lambda a, dt: a + res_lo.to(dt)])
    if c.out_f32:
        out, out_lo = v.float(), None
        assert torch.equal(out.double(), v)
    else:
        assert float(v.abs().max()) < 60000
        out = v.half()
        out_lo = (v - out.double()).half() if c.out_lo else None
        if c.out_lo:
            assert torch.equal((v - out.double()).float().double(), v - out.double())
    x0 = x[:, :g["C0"]].contiguous()
    x1 = x[:, g["C0"]:].contiguous() if g["C1"] else None
    keep = c.kind != "lin" or c.geglu                            # (the fp64 product is kept where a test reads it: gathers and GEGLU)
    return dict(geo=g, x0=x0, x1=x1, pack=pack, res=res, res_lo=res_lo, vec=vec, blend=blend, t64=t64 if keep else None, gate=gate, out=out, out_lo=out_lo)


# ------------------------------------------------------------------------------------------------- the kernel's index arithmetic (CPU, fp32)
def recipe(c, broken=None):
    """Product + bias [M, N] fp32 by the kernel's own index arithmetic in torch on the CPU: class_of (four class-local runs of the folded
    upsampler), row_origin (the top-left tap as a signed 16-bit pair, pix0, foldx), the K walk - walk_step's (tap, source, channel) for
    channel-aligned tiles, the per-chunk division of the generic stage() - tap_source (bounds in the upsampled extent, the >> 1 of mode 1,
    zeros outside) and out_row.  A read outside its operand (the NaN guard, or the NaN pitch pad behind the last channel) gives NaN.
    ``broken`` - what the tests must notice: "bounds" / "bounds_left": the ix < Wlim / the ix >= 0 half of the bounds test dropped; "parity": the class's row shift
    1 - py taken as py; "switch": walk_step's source switch one tile late; "out_row": out_row without py * 2 Win."""
    pr = problem(c)
    g = pr["geo"]
    C0, C1, Hin, Win, KW, stride, up, N, K = (g[k] for k in ("C0", "C1", "Hin", "Win", "KW", "stride", "up", "N", "K"))
    Ct, npad, Kpad = C0 + C1, -(-N // 128) * 128, pr["pack"].w.shape[1]
    Wall, bias = pr["pack"].w.float(), pr["pack"].bias.float()[:N]
    src = [pr["x0"].float(), pr["x1"].float() if C1 else None]
    fold, fast = up == 2, is_fast(c)
    Mc, Hout, Wout = (g["M"] // 4, Hin, Win) if fold else (g["M"], g["Hout"], g["Wout"])      # igemm.hip:988-990: the kernels see one class
    foldx = KW == 1 and g["pad_w"] == 0 and stride == 1 and not up and Wout == Win             # :907
    Hlim, Wlim = (2 * Hin, 2 * Win) if up == 1 else (Hin, Win)
    m = torch.arange(Mc)
    out = torch.full((g["M"], N), NAN, dtype=torch.float32)

    def gather(iy0, ix0, pix0, tap, source, cofs, n):
        """tap_source for every row: [Mc, n]"""
        ky, kx = tap // KW, tap % KW
        iy, ix = iy0 + ky, ix0 + kx
        ok = (iy >= 0) & (iy < Hlim) & ((ix >= 0) if broken != "bounds_left" else True) & ((ix < Wlim) if broken != "bounds" else True)
        if up == 1:
            iy, ix = iy >> 1, ix >> 1
        X = src[source]
        row = pix0 + iy * Win + ix
        outside = ok & ((row < 0) | (row >= X.shape[0]))
        a = X[row.clamp(0, X.shape[0] - 1)]
        a = torch.cat([a, torch.full((Mc, BK), NAN)], 1)[:, cofs:cofs + n]          # behind the last channel lies the NaN pitch pad
        a = torch.where(ok[:, None], a, torch.zeros(()))
        return torch.where(outside[:, None], torch.full((), NAN), a)

    for par in range(4 if fold else 1):
        py, px = par >> 1, par & 1
        pad_h, pad_w = ((py if broken == "parity" else 1 - py), 1 - px) if fold else (g["pad_h"], g["pad_w"])
        img, rem = m // (Hout * Wout), m % (Hout * Wout)
        oy, ox = rem // Wout, rem % Wout
        iyx = (((oy * stride - pad_h) << 16) | ((0 if foldx else ox * stride - pad_w) & 0xffff)) & 0xffffffff       # :68, as 32 bits
        iyx = iyx - ((iyx >> 31) << 32)
        iy0, ix0 = iyx >> 16, ((iyx & 0xffff) ^ 0x8000) - 0x8000                     # :79  (int)(short)
        pix0 = img * Hin * Win + (ox if foldx else 0)
        Wimg = Wall[par * npad:par * npad + N]
        acc = bias.expand(Mc, N).clone()
        if fast:
            tap = source = ci = 0
            for kt in range(Kpad // BK):
                acc += gather(iy0, ix0, pix0, tap, source, ci, BK) @ Wimg[:, kt * BK:(kt + 1) * BK].t()
                ci += BK                                                             # walk_step (:106-113)
                if ci == (C1 if source else C0) + (BK if broken == "switch" and source == 0 and C1 else 0):
                    ci = 0
                    if source == 0 and C1 > 0:
                        source = 1
                    else:
                        source, tap = 0, tap + 1
        else:
            for kg in range(0, Kpad, 8):                                             # :180-191, one 16-byte chunk
                if kg >= K:
                    continue                                                         # kvalid: the zero page
                tap, ci = kg // Ct, kg % Ct
                source, cofs = (0, ci) if ci < C0 else (1, ci - C0)
                acc += gather(iy0, ix0, pix0, tap, source, cofs, 8) @ Wimg[:, kg:kg + 8].t()
        rows = 2 * (m + m // Win * Win) + (0 if broken == "out_row" else py * 2 * Win) + px if fold else m      # igemm_tail.h:251
        out[rows] = acc
    return out


# ------------------------------------------------------------------------------------------------- buffers and parameters
def images(c):
    """name -> (flat CPU buffer, element offset of [0, 0], pitch) for every pointer of the call, and `want`: name -> the buffer an output
    must be afterwards.  Outputs start NaN-filled, or hold the residual they alias (res_post)."""
    pr = problem(c)
    im = {"x0": guarded(pr["x0"]), "w": guarded(pr["pack"].w, 0), "bias": guarded(pr["pack"].bias[None], 0)}
    if pr["x1"] is not None:
        im["x1"] = guarded(pr["x1"], X1_PAD)
    for k in ("res_lo", "blend"):
        if pr[k] is not None:
            im[k] = guarded(pr[k], c.opad if k == "res_lo" else 8)
    if pr["vec"] is not None:
        im["vec"] = guarded(pr["vec"])
    inplace = c.res_post
    if pr["res"] is not None and not inplace:
        im["res"] = guarded(pr["res"], c.opad)
    im["out"] = guarded(pr["res"] if inplace else torch.full(pr["out"].shape, NAN, dtype=pr["out"].dtype), c.opad)
    want = {"out": guarded(pr["out"], c.opad)[0]}
    if c.out_lo:
        im["out_lo"] = guarded(torch.full(pr["out"].shape, NAN, dtype=torch.float16), c.opad)
        want["out_lo"] = guarded(pr["out_lo"], c.opad)[0]
    return im, want


def make_params(c, base, ws=None):
    """hip.IgemmParams of a case; base: name -> address of that buffer's first element (images()); ws: (address, bytes) of the workspace."""
    from posetraj_amd import hip
    g = geometry(c)
    im, _ = images_layout(c)
    at = lambda k: base[k] + im[k][0] * im[k][1] if k in im else None                # (itemsize, offset, pitch)
    p = hip.IgemmParams()
    p.x0, p.x1, p.C0, p.C1, p.ld0, p.ld1 = at("x0"), at("x1"), g["C0"], g["C1"], im["x0"][2], im["x1"][2] if "x1" in im else 0
    for k in ("Nimg", "Hin", "Win", "Hout", "Wout", "KH", "KW", "stride", "pad_h", "pad_w", "M", "N", "K"):
        setattr(p, k, g[k])
    p.upsample2x, p.Kpad = g["up"], -(-g["K"] // BK) * BK
    p.w, p.bias = at("w"), at("bias")
    p.out, p.ldo = at("out"), im["out"][2]
    if c.res:
        p.res, p.ldr = (p.out, p.ldo) if c.res_post else (at("res"), im["res"][2])
    p.res_lo, p.out_lo = at("res_lo"), at("out_lo")
    if c.vec:
        p.vec, p.ldv, p.vec_mode, p.vG, p.vFS, p.vS, p.vB = at("vec"), im["vec"][2], c.vec, VG, VFS, VS, VB
    if c.blend:
        p.blend, p.ldb, p.alpha = at("blend"), im["blend"][2], ALPHA
    p.out_scale, p.act, p.res_post, p.out_f32 = c.out_scale, 1 if c.geglu else 0, int(c.res_post), int(c.out_f32)
    if c.cs:
        p.cs_cols, p.cs_scale = CS_COLS, CS_SCALE
    if ws:
        p.splitk_ws, p.splitk_ws_bytes = ws
    return p


@functools.lru_cache(maxsize=None)
def images_layout(c):
    """(name -> (itemsize, offset, pitch), name -> elements) of images(c): all make_params needs (no tensor is kept)."""
    im, _ = images(c)
    return {k: (v[0].element_size(), v[1], v[2]) for k, v in im.items()}, {k: v[0].numel() for k, v in im.items()}


def fake_bases(c):
    """Addresses for a plan query without a device: 256-byte aligned like the allocator's, never dereferenced (pt_igemm_plan is host only)."""
    return {k: (i + 1) << 28 for i, k in enumerate(sorted(images_layout(c)[0]))}


@contextlib.contextmanager
def hooks(force=-1, group_m=0, ablation=0):
    """The library's process-wide hooks, restored whatever happens."""
    from posetraj_amd import hip
    L = hip.lib()
    try:
        assert L.pt_igemm_force_config(force) == 0 and L.pt_igemm_set_tuning(group_m, ablation) == 0
        yield L
    finally:
        L.pt_igemm_force_config(-1)
        L.pt_igemm_set_tuning(0, 0)


def planned(c, force, offer_ws, base=None):
    """(cfg, splits, group_m, workspace bytes wanted) from pt_igemm_plan under the case's hooks.  Host only."""
    with hooks(force, c.group_m) as L:
        p = make_params(c, base or fake_bases(c))
        need = int(L.pt_igemm_splitk_ws_bytes(ctypes.byref(p)))
        if offer_ws and need:
            p.splitk_ws, p.splitk_ws_bytes = 1 << 40, need
        cfg, splits, gm = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        rc = L.pt_igemm_plan(ctypes.byref(p), ctypes.byref(cfg), ctypes.byref(splits), ctypes.byref(gm))
        assert rc == 0, L.pt_last_error().decode()
    return cfg.value, splits.value, gm.value, need


def all_runs():
    """Every launch of this file: (case, forced cfg, the cfg the plan must name, workspace offered)."""
    for c in ALL_CASES:
        for force, cfg in c.routes:
            yield c, force, cfg, c.splits > 1
        if c.splits > 1:
            yield c, -1, None, False                              # the same problem without a workspace: whatever un-split plan there is


# (label, case, forced cfg, change to the parameters, what pt_last_error must say): calls the library refuses (igemm.hip:915-922, :943-944)
def _set(**kw):
    def change(p):
        for k, v in kw.items():
            setattr(p, k, getattr(p, v) if isinstance(v, str) else v)
    return change


REFUSALS = [("geglu_cfg1", "tail_whole_G0", 1, _set(), "128x320 configuration does not support GEGLU"),
            ("geglu_cfg5", "tail_whole_G0", 5, _set(), "256x32 configuration does not support GEGLU"),
            ("geglu_res_cfg1", "tail_mixed_GEW", 1, _set(), "128x320 configuration does not support GEGLU"),
            ("fold_3x3", "fold_3x9x7", -1, _set(KH=3, KW=3, K=576, Kpad=576), r"folded upsample \(upsample2x=2\) needs KH = KW = 2"),
            ("fold_extent", "fold_3x9x7", -1, _set(Hout=9, Wout=7, M=189), r"folded upsample \(upsample2x=2\) needs KH = KW = 2 and Hout x Wout = 2 Hin x 2 Win"),
            ("fold_x1", "fold_3x9x7", -1, _set(x1="x0", C1=64, ld1=72, K=512, Kpad=512), "folded upsample takes one source"),
            ("fold_res", "fold_3x9x7", -1, _set(res="out", ldr=328), "folded upsample takes no side input"),
            ("fold_vec", "fold_3x9x7", -1, _set(vec="out", ldv=328, vec_mode=1, vG=VG), "folded upsample takes no side input"),
            ("fold_blend", "fold_3x9x7", -1, _set(blend="out", ldb=328), "folded upsample takes no side input"),
            ("fold_out_lo", "fold_3x9x7", -1, _set(out_lo="out"), "folded upsample writes one fp16 output"),
            ("fold_out_f32", "fold_3x9x7", -1, _set(out_f32=1), "folded upsample writes one fp16 output"),
            ("fold_act", "fold_3x9x7", -1, _set(act=2), "folded upsample has no activation and no column scale"),
            ("fold_cs_cols", "fold_3x9x7", -1, _set(cs_cols=8, cs_scale=4.0), "folded upsample has no activation and no column scale"),
            ("fold_c32", "fold_3x9x7", -1, _set(C0=32, K=128, Kpad=128), "folded upsample needs C0 % 64 == 0 and an unpadded K")]


def refused(entry, fn, base=None):
    """Run one REFUSALS entry through ``fn(L, byref(p))`` (the plan, or the launch: both refuse before anything else happens)."""
    import re
    label, name, force, change, message = entry
    c = CASES[name]
    with hooks(force) as L:
        p = make_params(c, base or fake_bases(c))
        change(p)
        rc = fn(L, ctypes.byref(p))
        said = L.pt_last_error().decode()
    assert rc != 0 and re.search(message, said), (label, rc, said)


# ------------------------------------------------------------------------------------------------- the run on the device
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from posetraj_amd import ops
    d = torch.device("cuda:0")
    ops.ensure_ready(d)
    return d


@functools.lru_cache(maxsize=2)
def device_inputs(dev, c):
    """The guarded inputs of a case on the device (uploaded once for all its routes)."""
    im, _ = images(c)
    d = {k: v[0].to(dev) for k, v in im.items() if k not in ("out", "out_lo")}
    assert all(t.data_ptr() % 256 == 0 for t in d.values())
    return d


def positive_zero(t):
    """-0 -> +0 (GEGLU cases only); every other bit pattern, NaN included, as it is."""
    b = bits(t).clone()
    b[b == torch.iinfo(b.dtype).min] = 0
    return b


def run(dev, c, force, offer_ws=False, ablation=0):
    """One call of a case under a forced configuration -> (elements of out's and out_lo's whole buffers - guard and pad included - whose
    bits differ from the reference image, the first such index, cfg, splits, the buffers as they came back)."""
    im, want = images(c)
    d = dict(device_inputs(dev, c))
    for k in want:
        d[k] = im[k][0].to(dev)
    base = {k: t.data_ptr() for k, t in d.items()}
    with hooks(force, c.group_m, ablation) as L:
        p = make_params(c, base)
        ws = None
        if offer_ws:
            need = int(L.pt_igemm_splitk_ws_bytes(ctypes.byref(p)))
            assert need > 0 and need % 4 == 0
            ws = torch.full((need // 4 + WS_TAIL,), NAN, dtype=torch.float32, device=dev)
            p.splitk_ws, p.splitk_ws_bytes = ws.data_ptr(), need
        cfg, splits = ctypes.c_int32(), ctypes.c_int32()
        assert L.pt_igemm_plan(ctypes.byref(p), ctypes.byref(cfg), ctypes.byref(splits), None) == 0, L.pt_last_error().decode()
        rc = L.pt_igemm_f16(ctypes.byref(p), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, L.pt_last_error().decode()
        torch.cuda.synchronize()
    bad, first, got = 0, -1, {}
    for k in want:
        got[k] = d[k].cpu()
        a, b = (positive_zero(got[k]), positive_zero(want[k])) if c.geglu else (bits(got[k]), bits(want[k]))
        diff = (a != b).nonzero().flatten()
        if diff.numel() and first < 0:
            first = int(diff[0])
        bad += int(diff.numel())
    if ws is not None:                                            # every slab element written, nothing behind the workspace
        tail = ws[need // 4:].cpu()
        assert bool((bits(tail) == bits(torch.full((WS_TAIL,), NAN))).all()), "the guard tail of the split-K workspace was written"
        assert not bool(torch.isnan(ws[:need // 4]).any()) or splits.value == 1
    return bad, first, cfg.value, splits.value, got


def locate(c, k, first):
    """(row, column) of a flat index of an output buffer, relative to [0, 0] of the output (negative / beyond: guard or pad)."""
    _, off, ld = images_layout(c)[0][k]
    return (first - off) // ld, (first - off) % ld


def check_routes(dev, c, offer_ws=False):
    """Every route of a case: the plan names what the table names, nothing differs.  -> the last run's buffers"""
    fast = is_fast(c)
    for force, cfg_named in c.routes:
        bad, first, cfg, splits, got = run(dev, c, force, offer_ws)
        variant = "SPLITK" if splits > 1 else c.variant
        report(f"{c.name} force={force} {route_name(cfg, fast)} splits={splits} V_{variant}: {bad} elements differ")
        assert cfg == cfg_named and splits == (c.splits if offer_ws else 1), (force, cfg, splits)
        assert bad == 0, (force, first, locate(c, "out", first))
    return got


# ------------------------------------------------------------------------------------------------- 1. linear layers, every route
@pytest.mark.parametrize("c", LINEAR, ids=lambda c: c.name)
def test_linear_every_route(dev, c):
    check_routes(dev, c)


# ------------------------------------------------------------------------------------------------- 2. tail variants
@pytest.mark.parametrize("c", TAIL_CASES, ids=lambda c: c.name)
def test_tail_variants(dev, c):
    """Both pipelined kernels and one plain-loop route of each of cfg 1, 2, 4 and 5 (GEGLU: the routes that serve it).  A case with out_lo
    also runs without it - same operands - and `out` must come back with the same bits."""
    check_routes(dev, c)
    if c.out_lo:
        twin = dataclasses.replace(c, out_lo=False)
        for force, _ in c.routes:
            a, b = run(dev, c, force)[4]["out"], run(dev, twin, force)[4]["out"]
            same = bool((bits(a) == bits(b)).all())
            report(f"{c.name} force={force} out with and without out_lo: {'identical' if same else 'DIFFERENT'}")
            assert same, force


# ------------------------------------------------------------------------------------------------- 3. gathers
@pytest.mark.parametrize("c", GATHERS, ids=lambda c: c.name)
def test_gathers(dev, c):
    check_routes(dev, c)


@pytest.mark.parametrize("c", FOLDED, ids=lambda c: c.name)
def test_folded_upsampler(dev, c):
    """upsample2x == 2 on folded weights (sums of at most four integers: exact in fp16) and mode 1 on the plain pack of the same layer are
    both bit-equal to fp64 conv2d(interpolate(x)) - hence to each other; out_row's scatter is checked through the NaN guard of the output."""
    a = check_routes(dev, c)["out"]
    b = check_routes(dev, mode1_twin(c))["out"]
    same = bool((bits(a) == bits(b)).all())
    report(f"{c.name} mode 2 against mode 1 on the same operands: {'identical' if same else 'DIFFERENT'}")
    assert same


# ------------------------------------------------------------------------------------------------- 4. split-K
@pytest.mark.parametrize("c", SPLITK, ids=lambda c: c.name)
def test_split_k(dev, c):
    """The automatic plan with the workspace offered (igemm10_kernel<V_SPLITK> + splitk_reduce_kernel) and without: both bit-equal to the
    reference, hence to each other."""
    a = check_routes(dev, c, offer_ws=True)
    bad, first, cfg, splits, b = run(dev, c, -1)
    report(f"{c.name} force=-1 {route_name(cfg, is_fast(c))} splits={splits} V_{c.variant} (no workspace): {bad} elements differ")
    assert splits == 1 and bad == 0, (first, locate(c, "out", first))
    assert all(bool((bits(a[k]) == bits(b[k])).all()) for k in a)


# ------------------------------------------------------------------------------------------------- 5. the tests notice what they claim to
def test_without_stores_every_inside_element_is_reported(dev):
    """Ablation bit 1 (no global stores; the fast tail honours it, so a case of whole waves): the whole inside of `out` is still NaN and
    every element of it is counted."""
    c = CASES["lin_whole"]
    g = geometry(c)
    assert all(g["n_out"] % WAVE_W[f] == 0 for f in (0, 3, 2))
    for force in (0, 3, 2):
        bad, _, _, _, got = run(dev, c, force, ablation=1)
        _, off, ld = images_layout(c)[0]["out"]
        inside = got["out"][off:off + g["M"] * ld].view(g["M"], ld)[:, :g["n_out"]]
        report(f"{c.name} force={force} ablation=1 (no stores): {bad} elements differ")
        assert bool(torch.isnan(inside).all()) and bad == g["M"] * g["n_out"]


def test_without_the_gelu_negative_gates_are_reported(dev):
    """Ablation bit 4 (value * gate, no GELU): wherever the gate is negative (and the value no zero) the output is no zero."""
    c = CASES["tail_whole_G0"]
    pr = problem(c)
    n_out = pr["geo"]["n_out"]
    wrong = int(((pr["gate"] < 0) & (pr["t64"][:, :n_out] != 0)).sum())
    assert wrong > pr["gate"].numel() // 4
    for force in (0, 3):
        bad = run(dev, c, force, ablation=4)[0]
        report(f"{c.name} force={force} ablation=4 (no GELU): {bad} elements differ")
        assert bad == wrong


# ------------------------------------------------------------------------------------------------- 6. refusals
@pytest.mark.parametrize("entry", REFUSALS, ids=lambda e: e[0])
def test_refusals(dev, entry):
    """A case the kernel legitimately refuses is an asserted refusal: pt_igemm_f16 returns non-zero with the message, before any launch."""
    c = CASES[entry[1]]
    base = {k: 1 << 28 for k in images_layout(c)[0]}              # refused by the plan: nothing is dereferenced
    refused(entry, lambda L, p: L.pt_igemm_f16(p, torch.cuda.current_stream().cuda_stream), base)
    report(f"{entry[0]}: refused ({entry[4]})")
