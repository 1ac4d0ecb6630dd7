"""pt_gemm_f16 / ptd_gemm_f16 (csrc/gemm.hip), the convolution gather of the weight gradients and Dense on the tape, on the MI355X
against fp64 - BIT FOR BIT.

The argument.  The operands are fp16 and the accumulators fp32.  Draw every operand uniformly from {+-1, +-2, +-3} (no zeros): every
product is a non-zero integer and every partial sum an integer below 2^24, so whatever the order of summation - K steps of 64, MFMA
lanes, split-K with fp32 atomics, the workspace fold of ptd_gemm_f16 - the fp32 result is THE integer, and an fp16 output is the one
correct rounding of alpha * integer (alpha is always a power of two).  There is no tolerance to choose: the tests assert bitwise
equality with an fp64 CPU reference, and one dropped or duplicated K element, one halo pixel read as data, one tile computed twice
(out_mode 2 / 3 accumulate) or not at all, one split whose range is off by a step each change at least one output.  Every test first
asserts the precondition on its reference: |ref| * max(1, 1 / alpha) < 2^24, and < 60000 for an fp16 output (< 2048 for the fp16
activations of section 3, where every value must be an exact fp16 integer).

Guarded buffers.  Every operand and every C travels inside a NaN-filled buffer: the leading dimension is 8 wider than needed and the
pad holds NaN, 64 NaN rows lie in front of the first row and behind the last.  A read outside the operand reaches the output as NaN;
after the call every element of C's buffer outside [M, N] of every batch entry must still be the NaN it was, every element inside
bit-equal to the reference.  out_mode 0 / 1 start from a NaN-filled inside, out_mode 2 / 3 from ints() and must end as
prefill + alpha A B.  (ptd_gemm_f16 refuses a split-K C that is not one dense block of memory - the store's [T][Co][Ci] gradient is -
so its C has no column pad; the guard rows remain.)

Every case runs through pt_gemm_f16; every accumulating one also through ptd_gemm_f16 with a NaN-filled workspace of
ptd_gemm_ws_floats floats.  Calls go through the raw binding (hip.GemmParams, hip.lib()): the strides and offsets under test are the
ones the kernel sees.

recipe() is the kernel's own summation in torch fp32 on the CPU - K steps of 64, split ranges, the gather by explicit indexing with the
dox / doy / dimg carries of Stager::next - and tests/test_gemm_exact_cpu.py holds it against the fp64 references of section 2 without
a GPU (and shows that a broken carry is noticed).

One line per case is printed; with PT_GEMM_EXACT=<file> it is also appended to that file (profiles/r11/gemm_exact.txt is such a run)."""
import ctypes
import functools
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GK = 64                              # gemm.hip:24  the K step
GUARD = 64                           # NaN rows in front of and behind every operand and every C
PAD = 8                              # NaN columns behind every row
NAN = float("nan")
ids = lambda c: "x".join(str(v) for v in c)

# ------------------------------------------------------------------------------------------------- section 1: plain products
# (M, N, K); the tile follows gemm.hip:384-387, FAST follows regular() at :396-402 (fast() below)
PLAIN = [(16, 16, 64),               # :384  the 32 x 32 tile, one K step
         (13, 11, 70),               # :384  the 32 x 32 tile; :101-104 scalar tails in every direction, 6 elements into a second K step
         (40, 56, 136),              # :385  the 64 x 64 tile, two K steps + 8: the last step's k < k_end select (:86)
         (57, 33, 100),              # :385  the 64 x 64 tile, ragged: the slow Stager, every other row of a [row][k] operand 16-byte aligned (:102)
         (200, 64, 128),             # :386  the 128 x 64 tile, second M tile ragged (r < R, :86)
         (130, 50, 77),              # :386  the 128 x 64 tile, ragged
         (264, 136, 320),            # :387  the 128 x 128 tile, 3 x 2 tiles, all % 8: FAST in every transpose
         (1160, 136, 64),            # :190-192  ten M tiles: the second GROUP_M group has gmm = 2; 20 workgroups, no multiple of 8 (pt_xcd_remap, :185)
         (8, 8, 0)]                  # :267 / :339  K = 0: out_mode 0 / 1 store zeros, 2 / 3 leave C alone
SHIFTED = (264, 136, 320, 1, 4)      # :399  A's base moved by 1 element, B's by 4: a regular shape on the slow instance of the 128 x 128 tile
TRANSPOSES = [(0, 0), (0, 1), (1, 0), (1, 1)]        # A stored [M, K] / [K, M], B stored [K, N] / [N, K]
# (M, N, K, splits asked, the split ranges gemm_splits (:316-324) leaves)
SPLITK = [(130, 50, 1000, 3, (384, 384, 232)),                  # :319  K per split rounded up to whole K steps, a short last split
          (40, 56, 320, 7, (64,) * 5),                          # :321  7 asked, 5 left
          (13, 11, 130, 100, (64, 64, 2)),                      # :320  more splits than K steps: clamped to 3, the last one 2 elements
          (264, 136, 4096, 8, (512,) * 8)]                      # the 128 x 128 tile, 6 tiles x 8 splits
BATCHED = (2, 14, 3, 3, 16)          # (Bc, F, S, heads, hd): :195-201 three batch levels in place inside a fused projection

# ------------------------------------------------------------------------------------------------- section 2: gathered weight gradients
# (kind, N, H, W, Ci, Co, stride, splits); kind c3: 3 x 3 pad 1, c1: 1 x 1 pad 0, t3: (3, 1) pad (1, 0) over the image (F, S) of N clips.
# splits: None - one split only; "auto" - also what autodiff._split_k picks; an int - also that many
GATHERED = [("c3", 1, 5, 72, 8, 16, 1, None),        # :371  OW > GK: dox = 64, a carry into oy at every step (:115-117)
            ("c3", 2, 3, 64, 8, 16, 1, None),        # :371  OW == GK: dox = 0, doy = 1; oy wraps into img every third step (:118-120)
            ("c3", 1, 2, 128, 8, 16, 1, None),       # two K steps per image row: the carry at every second step
            ("c3", 40, 3, 5, 16, 24, 1, None),       # :371  OH OW = 15: dimg = 4, doy = 0, dox = 4; both carries in one step
            ("c3", 33, 2, 2, 8, 16, 1, None),        # dimg = 16, nothing else moves
            ("c3", 70, 1, 1, 8, 16, 1, None),        # 1 x 1 images: :90 masks eight of the nine taps entirely - those matrices are exactly zero
            ("c3", 3, 9, 7, 8, 24, 2, None),         # stride 2, odd extents, OH x OW = 5 x 4 (:89)
            ("c3", 2, 10, 12, 16, 16, 2, None),      # stride 2, even extents: the last tap column reads inside, the first outside
            ("c1", 2, 6, 5, 64, 32, 1, None),        # one tap, no halo
            ("t3", 2, 5, 13, 16, 24, 1, None),       # the temporal convolution's gather tuple (autodiff.py Dense.accumulate)
            ("t3", 3, 1, 7, 16, 24, 1, None),        # one frame: only the centre tap sees data
            ("c3", 4, 40, 72, 8, 16, 1, "auto"),     # the workload's latent geometry, K = 11520: 22 splits asked, 20 left, boundaries mid-row (:73-77)
            ("c3", 2, 64, 64, 72, 136, 1, "auto"),   # the 128 x 128 tile with the gather, K = 8192
            ("c3", 2, 32, 36, 16, 16, 2, 3)]         # stride 2 with splits, K = 576: three splits of 192


def report(line: str):
    print(line)
    path = os.environ.get("PT_GEMM_EXACT")
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


# ------------------------------------------------------------------------------------------------- common machinery
def ints(*shape, seed):
    """fp16, uniform over {+-1, +-2, +-3}."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.randint(1, 4, shape, generator=g)
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (mag * sign).half()


def guarded(t, pad=PAD, shift=0):
    """(flat CPU buffer, element offset of t[0, 0], pitch): t's rows at pitch cols + pad inside NaN - the pad columns, GUARD rows (and
    ``shift`` elements) in front, GUARD rows behind."""
    rows, cols = t.shape
    ld = cols + pad
    front = GUARD * ld + shift
    buf = torch.full((front + (rows + GUARD) * ld,), NAN, dtype=t.dtype)
    buf[front:front + rows * ld].view(rows, ld)[:, :cols] = t
    return buf, front, ld


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def mismatches(got, want):
    """(number of elements of the whole buffer - guard and pad included - whose bits differ, the first such index)"""
    bad = (bits(got.cpu()) != bits(want)).nonzero().flatten()
    return int(bad.numel()), (int(bad[0]) if bad.numel() else -1)


def exact_precondition(ref64, alpha, fp16_out):
    """ref64 = alpha * the integer product: the integer itself stays below 2^24 and an fp16 output in the finite range."""
    top = float(ref64.abs().max()) if ref64.numel() else 0.0
    assert top * max(1.0, 1.0 / alpha) < 2 ** 24
    if fp16_out:
        assert top < 60000


def gemm_splits(K, splits):
    """gemm.hip:316-324 -> (K per split, splits left)"""
    splits = max(1, splits)
    kps = max(GK, (-(-K // splits) + GK - 1) // GK * GK)
    return kps, max(1, -(-K // kps))


def tile(M, N):
    """gemm.hip:384-387 -> (BM, BN)"""
    if M <= 16 and N <= 16:
        return 32, 32
    if M <= 64 and N <= 64:
        return 64, 64
    return (128, 64) if N <= 64 else (128, 128)


def regular(ptr, s_r, s_k, rows, K, ld=0):
    """regular() of gemm_launch (gemm.hip:396-400) for an operand without batch offsets"""
    kc = s_k == 1 and ld == 0
    other = s_r if kc else (ld or s_k)
    return ptr % 16 == 0 and other % 8 == 0 and (K % 8 == 0 if kc else rows % 8 == 0)


def fast(M, N, K, ta, tb, shift_a=0, shift_b=0):
    """Whether a plain product of guarded operands (pitch = columns + 8, bases 16-byte aligned but for the shifts) takes the FAST instance."""
    sa = (1, M + PAD) if ta else (K + PAD, 1)
    sb = (1, K + PAD) if tb else (N + PAD, 1)             # (sb_k, sb_n)
    return regular(2 * shift_a, sa[0], sa[1], M, K) and regular(2 * shift_b, sb[1], sb[0], N, K)


def launch(hip, p, entry, dev):
    """The raw call; ptd: with a NaN-filled workspace of exactly the size the library asks for."""
    L = hip.lib()
    stream = torch.cuda.current_stream().cuda_stream
    if entry == "ptd":
        n = L.ptd_gemm_ws_floats(ctypes.byref(p))
        ws = torch.full((max(int(n), 2),), NAN, dtype=torch.float32, device=dev)
        rc = L.ptd_gemm_f16(ctypes.byref(p), ws.data_ptr(), n, stream)
    else:
        rc = L.pt_gemm_f16(ctypes.byref(p), stream)
    assert rc == 0, L.pt_last_error().decode()
    torch.cuda.synchronize()


def c_images(ref64, out_mode, prefill, pad):
    """(C's buffer before the call, the buffer it must be afterwards, offset, pitch) from the fp64 reference of alpha A B [rows, N]."""
    dtype = torch.float16 if out_mode == 0 else torch.float32
    if out_mode >= 2:
        inside, after = prefill.to(dtype), (prefill.double() + ref64).to(dtype)
    else:
        inside, after = torch.full(ref64.shape, NAN, dtype=dtype), ref64.to(dtype)
    before, off, ld = guarded(inside, pad)
    want, _, _ = guarded(after, pad)
    return before, want, off, ld


@functools.lru_cache(maxsize=None)
def plain_problem(M, N, K):
    A, B = ints(M, K, seed=1000 + M), ints(K, N, seed=2000 + N)
    return A, B, A.double() @ B.double()


@functools.lru_cache(maxsize=1)
def plain_operands(dev, M, N, K, ta, tb, shift):
    """The guarded operands of a plain product on the device (uploaded once for all the runs of a test)."""
    A, B, _ = plain_problem(M, N, K)
    abuf, aoff, lda = guarded(A.t().contiguous() if ta else A, shift=shift[0])
    bbuf, boff, ldb = guarded(B.t().contiguous() if tb else B, shift=shift[1])
    a, b = abuf.to(dev), bbuf.to(dev)
    assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0            # fast() counts on aligned allocations
    return a, aoff, lda, b, boff, ldb


@functools.lru_cache(maxsize=None)
def prefill(rows, cols):
    """What an accumulating run finds in C."""
    return ints(rows, cols, seed=3000 + rows + cols)


def plain_product(dev, M, N, K, ta, tb, out_mode, alpha, *, splits=1, entry="pt", shift=(0, 0)):
    """One product of guarded operands into a guarded C -> (mismatching elements, first index)."""
    from posetraj_amd import hip
    ref = plain_problem(M, N, K)[2] * alpha
    exact_precondition(ref, alpha, out_mode == 0)
    a, aoff, lda, b, boff, ldb = plain_operands(dev, M, N, K, ta, tb, shift)
    before, want, coff, ldc = c_images(ref, out_mode, prefill(M, N) if out_mode >= 2 else None, 0 if entry == "ptd" else PAD)
    c = before.to(dev)
    p = hip.GemmParams()
    p.A, p.B, p.C = a.data_ptr() + 2 * aoff, b.data_ptr() + 2 * boff, c.data_ptr() + c.element_size() * coff
    p.M, p.N, p.K = M, N, K
    p.sa_m, p.sa_k = (1, lda) if ta else (lda, 1)
    p.sb_k, p.sb_n = (1, ldb) if tb else (ldb, 1)
    p.sc_m, p.sc_n = ldc, 1
    p.nb0 = p.nb1 = p.nb2 = 1
    p.alpha, p.out_mode, p.splits = alpha, out_mode, splits
    launch(hip, p, entry, dev)
    return mismatches(c, want)


# ------------------------------------------------------------------------------------------------- 1. plain products
def check_tables():
    """A check on the tables, not on the kernel: per tile shape the plain cases (with SHIFTED) take the FAST and the slow instance, the
    GROUP_M case is what its comment says, and gemm_splits leaves the split ranges SPLITK names."""
    seen = {}
    for M, N, K in PLAIN:
        for ta, tb in TRANSPOSES:
            seen.setdefault(tile(M, N), set()).add(fast(M, N, K, ta, tb))
    M, N, K, da, db = SHIFTED
    for ta, tb in TRANSPOSES:
        assert fast(M, N, K, ta, tb) and not fast(M, N, K, ta, tb, da, db)
    seen[tile(M, N)].add(False)
    assert seen == {t: {True, False} for t in [(32, 32), (64, 64), (128, 64), (128, 128)]}
    tiles_m, tiles_n = -(-1160 // 128), -(-136 // 128)
    assert tiles_m == 10 and tiles_m % 8 == 2 and (tiles_m * tiles_n) % 8 != 0
    for M, N, K, asked, ranges in SPLITK:
        kps, left = gemm_splits(K, asked)
        assert tuple(min(kps, K - s * kps) for s in range(left)) == ranges
    assert gemm_splits(0, 1) == (GK, 1)


def test_the_tables_reach_what_they_name():
    check_tables()


@pytest.mark.parametrize("shape", PLAIN, ids=ids)
def test_plain_products(dev, shape):
    """All four storage combinations; out_mode 0 (fp16, alpha 1/2), 1 (fp32, alpha 1/4) and 3 (fp32 += onto a pre-filled C, alpha 2, also
    through ptd_).  K = 0: zeros, or C as it was."""
    M, N, K = shape
    for ta, tb in TRANSPOSES:
        for out_mode, alpha, entry in ((0, 0.5, "pt"), (1, 0.25, "pt"), (3, 2.0, "pt"), (3, 2.0, "ptd")):
            bad, at = plain_product(dev, M, N, K, ta, tb, out_mode, alpha, entry=entry)
            report(f"plain {M}x{N}x{K} ta={ta} tb={tb} tile={ids(tile(M, N))} fast={int(fast(M, N, K, ta, tb))} out_mode={out_mode} {entry}: "
                   f"{bad} elements differ")
            assert bad == 0, (ta, tb, out_mode, entry, at)


def test_misaligned_bases_take_the_slow_instance(dev):
    M, N, K, da, db = SHIFTED
    for ta, tb in TRANSPOSES:
        for out_mode, alpha in ((0, 0.5), (1, 0.25), (3, 2.0)):
            bad, at = plain_product(dev, M, N, K, ta, tb, out_mode, alpha, shift=(da, db))
            report(f"shifted {M}x{N}x{K} ta={ta} tb={tb} A+{da} B+{db} out_mode={out_mode}: {bad} elements differ")
            assert bad == 0, (ta, tb, out_mode, at)


@pytest.mark.parametrize("case", SPLITK, ids=lambda c: ids(c[:4]))
def test_split_k_onto_a_prefilled_c(dev, case):
    """out_mode 2 in the weight gradients' storage (A as [K, M], B as [K, N]) and in the opposite one: atomics (pt_) and the workspace
    fold (ptd_) both give prefill + A B exactly - hence each other."""
    M, N, K, splits, ranges = case
    for ta, tb in ((1, 0), (0, 1)):
        for entry in ("pt", "ptd"):
            bad, at = plain_product(dev, M, N, K, ta, tb, 2, 1.0, splits=splits, entry=entry)
            report(f"split-K {M}x{N}x{K} ta={ta} tb={tb} splits={splits}->{len(ranges)} {entry}: {bad} elements differ")
            assert bad == 0, (ta, tb, entry, at)


def test_three_level_batches_in_place(dev):
    """The temporal attention's addressing: Q K^T (out_mode 1) and dS K (out_mode 0) over (clip, position, head) batches inside a
    [rows, 3 C + 8] projection, tokens a row stride apart; dS K writes the Q column block of a NaN-filled buffer of that shape, whose
    K and V blocks, pad and guard rows must stay NaN."""
    from posetraj_amd import hip
    Bc, Fr, S, heads, hd = BATCHED
    Cc, rows = heads * hd, Bc * Fr * S
    qkv = ints(rows, 3 * Cc, seed=31)
    qbuf, qoff, ld = guarded(qkv)
    d = qbuf.to(dev)
    x = qkv.double().view(Bc, Fr, S, 3, heads, hd)
    q, k = x[:, :, :, 0].permute(0, 2, 3, 1, 4), x[:, :, :, 1].permute(0, 2, 3, 1, 4)           # [Bc, S, heads, F, hd]
    # S = alpha Q K^T -> [Bc S heads][F, F] fp32
    alpha = 0.25
    ref = alpha * q @ k.transpose(-1, -2)
    exact_precondition(ref, alpha, False)
    before, want, coff, ldc = c_images(ref.reshape(-1, Fr), 1, None, PAD)
    c = before.to(dev)
    p = hip.GemmParams()
    p.A, p.B, p.C = d.data_ptr() + 2 * qoff, d.data_ptr() + 2 * (qoff + Cc), c.data_ptr() + 4 * coff
    p.M, p.N, p.K = Fr, Fr, hd
    p.sa_m, p.sa_k, p.sb_k, p.sb_n, p.sc_m, p.sc_n = S * ld, 1, 1, S * ld, ldc, 1
    p.nb0, p.nb1, p.nb2 = Bc, S, heads
    p.ba0, p.ba1, p.ba2 = Fr * S * ld, ld, hd
    p.bb0, p.bb1, p.bb2 = Fr * S * ld, ld, hd
    p.bc0, p.bc1, p.bc2 = S * heads * Fr * ldc, heads * Fr * ldc, Fr * ldc
    p.alpha, p.out_mode, p.splits = alpha, 1, 1
    launch(hip, p, "pt", dev)
    bad, at = mismatches(c, want)
    report(f"batched Q K^T {ids(BATCHED)} out_mode=1: {bad} elements differ")
    assert bad == 0, at
    # dQ = alpha dS K -> the Q block of [rows, 3 C + 8] fp16
    alpha = 0.5
    ds = ints(Bc * S * heads * Fr, Fr, seed=32)
    sbuf, soff, lds = guarded(ds)
    dsd = sbuf.to(dev)
    ref = alpha * ds.double().view(Bc, S, heads, Fr, Fr) @ k                                    # [Bc, S, heads, F, hd]
    exact_precondition(ref, alpha, True)
    image = torch.full((rows, 3 * Cc), NAN, dtype=torch.float16)
    before, goff, ldg = guarded(image)
    image.view(Bc, Fr, S, 3, heads, hd)[:, :, :, 0] = ref.permute(0, 3, 1, 2, 4).half()
    want, _, _ = guarded(image)
    g = before.to(dev)
    p = hip.GemmParams()
    p.A, p.B, p.C = dsd.data_ptr() + 2 * soff, d.data_ptr() + 2 * (qoff + Cc), g.data_ptr() + 2 * goff
    p.M, p.N, p.K = Fr, hd, Fr
    p.sa_m, p.sa_k, p.sb_k, p.sb_n, p.sc_m, p.sc_n = lds, 1, S * ld, 1, S * ldg, 1
    p.nb0, p.nb1, p.nb2 = Bc, S, heads
    p.ba0, p.ba1, p.ba2 = S * heads * Fr * lds, heads * Fr * lds, Fr * lds
    p.bb0, p.bb1, p.bb2 = Fr * S * ld, ld, hd
    p.bc0, p.bc1, p.bc2 = Fr * S * ldg, ldg, hd
    p.alpha, p.out_mode, p.splits = alpha, 0, 1
    launch(hip, p, "pt", dev)
    bad, at = mismatches(g, want)
    report(f"batched dS K {ids(BATCHED)} out_mode=0 into the Q block: {bad} elements differ")
    assert bad == 0, at


# ------------------------------------------------------------------------------------------------- 2. gathered weight gradients
def gather_geometry(case):
    """-> (Nimg, H, W, OH, OW, KH, KW, stride, pad_h, pad_w) of a GATHERED case"""
    kind, N, H, W, Ci, Co, stride, _ = case
    KH, KW, ph, pw = {"c3": (3, 3, 1, 1), "c1": (1, 1, 0, 0), "t3": (3, 1, 1, 0)}[kind]
    return N, H, W, (H + 2 * ph - KH) // stride + 1, (W + 2 * pw - KW) // stride + 1, KH, KW, stride, ph, pw


def auto_splits(case):
    """What Dense.accumulate asks for: autodiff._split_k over 128 x 128 tiles x taps (the function is pure: no GPU is touched)."""
    from posetraj_amd import autodiff
    _, _, _, _, Ci, Co, _, _ = case
    N, H, W, OH, OW, KH, KW, _, _, _ = gather_geometry(case)
    return autodiff._split_k(-(-Co // 128) * -(-Ci // 128) * KH * KW, N * OH * OW)


def split_choices(case):
    """The split counts a GATHERED case runs with besides 1"""
    s = case[7]
    return [] if s is None else [auto_splits(case) if s == "auto" else s]


@functools.lru_cache(maxsize=None)
def gathered_problem(case):
    """(X [N H W, Ci] fp16 channels-last rows, dY [N OH OW, Co] fp16 rows, the fp64 weight gradient tap-major [T, Co, Ci])"""
    kind, _, _, _, Ci, Co, stride, _ = case
    N, H, W, OH, OW, KH, KW, _, ph, pw = gather_geometry(case)
    seed = 100 * GATHERED.index(case)
    x, dy = ints(N * H * W, Ci, seed=4000 + seed), ints(N * OH * OW, Co, seed=5000 + seed)
    xi = x.double().view(N, H, W, Ci).permute(0, 3, 1, 2)
    gi = dy.double().view(N, OH, OW, Co).permute(0, 3, 1, 2)
    if kind == "t3":                                          # Conv3d (3, 1, 1) over [B, C, F, S, 1], in fp64
        dw = torch.nn.grad.conv3d_weight(xi.unsqueeze(-1), (Co, Ci, 3, 1, 1), gi.unsqueeze(-1), padding=(1, 0, 0))[..., 0]
    else:
        dw = torch.nn.grad.conv2d_weight(xi, (Co, Ci, KH, KW), gi, stride=stride, padding=(ph, pw))
    return x, dy, dw.permute(2, 3, 0, 1).reshape(KH * KW, Co, Ci).contiguous()


def recipe(x, dy, geometry, splits=1, broken=None):
    """The weight gradient [T, Co, Ci] by gemm.hip's own recipe in torch fp32 on the CPU: per tap (the innermost batch level) and per split
    (gemm_splits), K steps of 64 output pixels whose (img, oy, ox) are decomposed once at the split's start (Stager::start, :73-77) and
    then moved by (dimg, doy, dox) with one carry per digit (Stager::next, :114-120); a pixel outside the image or past k_end
    contributes zero (:86-90).  ``broken`` - what the tests must notice: "dox": dox taken as GK % (OW + 1); "carry": the carry from ox into
    oy dropped."""
    N, H, W, OH, OW, KH, KW, stride, ph, pw = geometry
    K, Co, Ci = dy.shape[0], dy.shape[1], x.shape[1]
    xf, dyf = x.float(), dy.float()
    dimg, doy, dox = (GK // OW) // OH, (GK // OW) % OH, GK % (OW + 1 if broken == "dox" else OW)       # gemm.hip:371
    kps, splits = gemm_splits(K, splits)
    out = torch.zeros(KH * KW, Co, Ci, dtype=torch.float32)
    lane = torch.arange(GK)
    for tap in range(KH * KW):
        ky, kx = tap // KW, tap % KW                          # :200
        for s in range(splits):
            k_begin, k_end = s * kps, min((s + 1) * kps, K)
            kk = k_begin + lane
            ox, oy, img = kk % OW, (kk // OW) % OH, kk // OW // OH
            acc = torch.zeros(Co, Ci, dtype=torch.float32)
            for k0 in range(k_begin, k_end, GK):
                iy, ix = oy * stride + ky - ph, ox * stride + kx - pw
                ok = (k0 + lane < k_end) & (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
                src = ((img * H + iy) * W + ix)[ok]
                if broken and bool((src >= xf.shape[0]).any()):               # a broken walk leaves X: the kernel would read the NaN guard
                    acc += NAN
                    src = src.clamp(max=xf.shape[0] - 1)
                acc += dyf[k0 + lane[ok]].t() @ xf[src]
                ox = ox + dox
                cx = ox >= OW
                ox = ox - cx * OW
                oy = oy + doy + (0 if broken == "carry" else cx)
                cy = oy >= OH
                oy = oy - cy * OH
                img = img + dimg + cy
            out[tap] += acc
    return out


@functools.lru_cache(maxsize=1)
def gathered_operands(dev, case):
    x, dy, _ = gathered_problem(case)
    xbuf, xoff, ldx = guarded(x)
    ybuf, yoff, ldy = guarded(dy)
    return xbuf.to(dev), xoff, ldx, ybuf.to(dev), yoff, ldy


def gathered_product(dev, case, out_mode, splits, entry):
    from posetraj_amd import hip
    _, _, _, _, Ci, Co, stride, _ = case
    N, H, W, OH, OW, KH, KW, _, ph, pw = gather_geometry(case)
    T, K = KH * KW, N * OH * OW
    ref = gathered_problem(case)[2]
    exact_precondition(ref, 1.0, False)
    xd, xoff, ldx, yd, yoff, ldy = gathered_operands(dev, case)
    before, want, coff, ldc = c_images(ref.view(T * Co, Ci), out_mode, prefill(T * Co, Ci), 0 if entry == "ptd" else PAD)
    c = before.to(dev)
    p = hip.GemmParams()
    p.A, p.B, p.C = yd.data_ptr() + 2 * yoff, xd.data_ptr() + 2 * xoff, c.data_ptr() + 4 * coff
    p.M, p.N, p.K = Co, Ci, K
    p.sa_m, p.sa_k, p.sb_k, p.sb_n, p.sc_m, p.sc_n = 1, ldy, ldx, 1, ldc, 1
    p.nb0, p.nb1, p.nb2 = 1, 1, T
    p.bc2 = Co * ldc
    p.alpha, p.out_mode, p.splits = 1.0, out_mode, splits
    p.g_H, p.g_W, p.g_OH, p.g_OW, p.g_KH, p.g_KW, p.g_stride, p.g_pad_h, p.g_pad_w, p.g_ld = H, W, OH, OW, KH, KW, stride, ph, pw, ldx
    launch(hip, p, entry, dev)
    return mismatches(c, want)


@pytest.mark.parametrize("case", GATHERED, ids=ids)
def test_gathered_weight_gradients(dev, case):
    """A = dY^T [Co, K], B = X gathered, C in the store's [T][Co][Ci] layout: out_mode 3 in one split; the split cases also out_mode 2
    with the split count of the table.  Every run through pt_ and ptd_."""
    N, H, W, OH, OW, KH, KW, _, _, _ = gather_geometry(case)
    K = N * OH * OW
    if case[0] == "c3" and H == W == 1:
        assert int((gathered_problem(case)[2].abs().amax((1, 2)) > 0).sum()) == 1               # only the centre tap is non-zero
    if case[7] == "auto":
        assert auto_splits(case) > 1
    for out_mode, splits in [(3, 1)] + [(2, s) for s in split_choices(case)]:
        for entry in ("pt", "ptd"):
            bad, at = gathered_product(dev, case, out_mode, splits, entry)
            report(f"gathered {ids(case[:7])} K={K} OHxOW={OH}x{OW} out_mode={out_mode} splits={splits}->{gemm_splits(K, splits)[1]} {entry}: "
                   f"{bad} elements differ")
            assert bad == 0, (out_mode, splits, entry, at)


# ------------------------------------------------------------------------------------------------- 3. Dense on the tape, exact
def wints(*shape, seed):
    """Integer weights in {+-1, +-2}, fp32."""
    g = torch.Generator().manual_seed(seed)
    return ((torch.randint(1, 3, shape, generator=g)) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)).float()


def fp16_integers(*tensors):
    """The precondition of section 3: every value is an integer below 2048, hence an exact fp16 number."""
    for t in tensors:
        assert float(t.abs().max()) < 2048 and bool((t == t.round()).all())


# (name, kind, geom, Ci, Co, stride, pad, residual, more than one split expected)
DENSE = [("conv3x3_res", "conv", (2, 9, 7), 16, 32, 1, 1, True, False),
         ("conv3x3_s2_odd", "conv", (1, 9, 7), 16, 32, 2, 1, False, False),            # pt_zero_insert2x_f16, odd extents
         ("conv3x3_s2_even", "conv", (2, 8, 12), 16, 16, 2, 1, False, False),
         ("conv1x1", "conv", (2, 6, 5), 32, 16, 1, 0, False, False),
         ("temporal", "conv_t3", (2, 5, 12), 16, 24, 1, 1, False, False),
         ("linear_300", "linear", 300, 64, 48, 1, 0, False, False),
         ("linear_14", "linear", 14, 64, 32, 1, 0, False, False),                     # pt_gemv_f16, forward and data gradient
         ("linear_qk", "stack", 700, 96, 40, 1, 0, False, False),
         ("conv3x3_split", "conv", (2, 36, 40), 8, 16, 1, 1, False, True)]            # 2880 pixels: _split_k picks more than one split


def rows_of(t):
    """[N, C, H, W] -> channels-last rows [N H W, C]"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


@functools.lru_cache(maxsize=None)
def dense_problem(name):
    """Inputs as the layer sees them (rows, fp16) and fp64 autograd of F.conv2d / F.conv3d / F.linear over the same values."""
    _, kind, geom, Ci, Co, stride, pad, residual, _ = next(c for c in DENSE if c[0] == name)
    seed = 7000 + 10 * [c[0] for c in DENSE].index(name)
    wshape = {"conv": (Co, Ci, 2 * pad + 1, 2 * pad + 1), "conv_t3": (Co, Ci, 3, 1, 1)}.get(kind, (Co, Ci))
    w, b = wints(*wshape, seed=seed), wints(Co, seed=seed + 1)
    wr, br = w.double().requires_grad_(True), b.double().requires_grad_(True)
    if kind in ("linear", "stack"):
        x = ints(geom, Ci, seed=seed + 2)
        xr = x.double().requires_grad_(True)
        y = F.linear(xr, wr, br)
    else:
        N, H, W = geom
        x = ints(N * H * W, Ci, seed=seed + 2)
        xr = x.double().requires_grad_(True)
        x4 = xr.view(N, H, W, Ci).permute(0, 3, 1, 2)
        y4 = F.conv2d(x4, wr, br, stride=stride, padding=pad) if kind == "conv" else F.conv3d(x4.unsqueeze(-1), wr, br, padding=(1, 0, 0))[..., 0]
        y = rows_of(y4)
    res = ints(*y.shape, seed=seed + 3) if residual else None
    dy = ints(*y.shape, seed=seed + 4)
    out = y if res is None else y + res.double()
    out.backward(dy.double())
    fp16_integers(out.detach(), xr.grad)
    exact_precondition(wr.grad, 1.0, False)
    return dict(w=w, b=b, x=x, res=res, dy=dy, y=out.detach(), dx=xr.grad, dw=wr.grad, db=br.grad)


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("name", [c[0] for c in DENSE])
def test_dense_on_the_tape(dev, AD, monkeypatch, name, det):
    """Forward (pt_igemm_f16 / pt_gemv_f16), data gradient (the transposed, tap-flipped pack; pt_zero_insert2x_f16 for stride 2), weight
    gradient with the split count the project picks and bias gradient (pt_colsum_f16) of a trainable layer: each bit-equal to fp64
    autograd; a second accumulate() gives exactly twice the gradient."""
    _, kind, geom, Ci, Co, stride, pad, residual, split = next(c for c in DENSE if c[0] == name)
    monkeypatch.setattr(AD, "DETERMINISTIC", det)
    pr = dense_problem(name)
    if kind == "stack":
        P = AD.ParamStore({"q": pr["w"][:Co // 2], "k": pr["w"][Co // 2:], "b": pr["b"]}, dev)
        L = AD.Dense(P, "q", "b", stack=("q", "k"))
        grad_w = lambda: P.stacked(("q", "k"), P.grad)
    else:
        P = AD.ParamStore({"w": pr["w"], "b": pr["b"]}, dev)
        L = AD.Dense(P, "w", "b", kind=kind, stride=stride, padding=pad)
        grad_w = lambda: P.gradient("w")
    g = geom if isinstance(geom, tuple) else None
    if split:
        T = pr["w"][0, 0].numel()
        assert AD._split_k(-(-Co // 128) * -(-Ci // 128) * T, pr["dy"].shape[0]) > 1
    tape = AD.Tape()
    xv = AD.Var(pr["x"].to(dev))
    rv = AD.Var(pr["res"].to(dev)) if residual else None
    out = AD.dense(tape, xv, L, geom=g, res=rv)
    dyd = pr["dy"].to(dev)
    out.g = dyd
    y = out.v
    tape.backward()
    torch.cuda.synchronize()
    got = {"y": y, "dx": xv.g, "dw": grad_w(), "db": P.gradient("b")}
    if residual:
        assert torch.equal(rv.g.cpu(), pr["dy"])
    for key, t in got.items():
        bad = int((t.detach().cpu().double().reshape(pr[key].shape) != pr[key]).sum())
        report(f"dense {name} {'det' if det else 'atomics'} {key}: {bad} elements differ")
        assert t.dtype == (torch.float16 if key in ("y", "dx") else torch.float32) and bad == 0, key
    L.accumulate(xv.v, dyd, g)
    torch.cuda.synchronize()
    assert torch.equal(grad_w().cpu().double().reshape(pr["dw"].shape), 2 * pr["dw"]) and torch.equal(P.gradient("b").cpu().double(), 2 * pr["db"])


# (name, geom, C0, C1, Co, k, upsample)
FROZEN = [("upsample2x", (2, 5, 6), 16, 0, 16, 3, True),                # + pt_sumpool2x_f16: a sum of four integers
          ("two_sources_1x1", (2, 6, 5), 64, 32, 32, 1, False),
          ("two_sources_3x3", (2, 6, 5), 64, 32, 32, 3, False)]


@pytest.mark.parametrize("case", FROZEN, ids=lambda c: c[0])
def test_dense_frozen_paths(dev, AD, case):
    """The frozen store's forward and data gradient: nearest-2x upsampling in the gather and two concatenated sources."""
    name, geom, C0, C1, Co, k, upsample = case
    N, H, W = geom
    Ci, pad = C0 + C1, k // 2
    w, b = wints(Co, Ci, k, k, seed=8000 + k), wints(Co, seed=8001)
    x = ints(N * H * W, Ci, seed=8002 + k)
    xr = x.double().requires_grad_(True)
    x4 = xr.view(N, H, W, Ci).permute(0, 3, 1, 2)
    xu = F.interpolate(x4, scale_factor=2.0, mode="nearest") if upsample else x4
    xu.retain_grad()
    y = rows_of(F.conv2d(xu, w.double(), b.double(), padding=pad))
    dy = ints(*y.shape, seed=8003)
    y.backward(dy.double())
    fp16_integers(y.detach(), xr.grad, xu.grad)               # xu.grad: the gradient before pt_sumpool2x_f16 is an fp16 tensor too
    L = AD.Dense(AD.FrozenParams({"w": w, "b": b}, dev), "w", "b", kind="conv", padding=pad)
    tape = AD.Tape()
    x0 = AD.Var(x[:, :C0].contiguous().to(dev))
    x1 = AD.Var(x[:, C0:].contiguous().to(dev)) if C1 else None
    out = AD.dense(tape, x0, L, geom=geom, x1=x1, upsample2x=upsample)
    out.g = dy.to(dev)
    yv = out.v
    tape.backward()
    dx = x0.g if x1 is None else torch.cat([x0.g, x1.g], 1)
    for key, t, want in (("y", yv, y.detach()), ("dx", dx, xr.grad)):
        bad = int((t.cpu().double() != want).sum())
        report(f"dense frozen {name} {key}: {bad} elements differ")
        assert t.dtype == torch.float16 and bad == 0, key


# ------------------------------------------------------------------------------------------------- 4. the refusal
def test_dense_refuses_the_weight_gradient_of_an_upsampling_layer(dev, AD):
    """upsample2x with a trainable store: accumulate() would pair dy's four-fold rows with the un-upsampled x and geometry."""
    P = AD.ParamStore({"w": wints(16, 16, 3, 3, seed=9000), "b": wints(16, seed=9001)}, dev)
    L = AD.Dense(P, "w", "b", kind="conv", padding=1)
    x = AD.Var(ints(2 * 5 * 6, 16, seed=9002).to(dev))
    tape = AD.Tape()
    with pytest.raises(RuntimeError, match="weight gradient of an upsampling layer is not implemented"):
        AD.dense(tape, x, L, geom=(2, 5, 6), upsample2x=True)
    assert L._packs is None and not tape._ops                 # refused before any launch
