"""The attention forward kernels on the MI355X on exact data: pt_attn_spatial_f16 and pt_attn_temporal_f16 (csrc/attn.hip: the spatial
kernel at 3 and 2 query blocks per wave, plain and q_prescaled; the one- / two-block and the long-clip temporal kernels) and pt_attn_f16 /
pt_attn_fwd_lse_f16 (csrc/attn_general.hip: attn_general_kernel<64 | 80 | 128>, attn_d512_kernel), through the raw binding.

Families, bounds and the argument for each are those of tests/attn_exact.py: A (every key counted once: half an fp16 ulp + two fp32
roundings against fp64), B (every query routed to its own key: bit equality), C (integer scores, cexp == 1: half an fp16 ulp + one fp32
rounding per 32-key step against fp64), lse within 2^-18 max(1, |ref|).  tests/test_attn_exact_cpu.py shows on a CPU model of the kernels
that these checks pass a correct kernel and reject a dropped or doubled key, unmasked pad keys, exchanged V rows, shifted query rows, a
skipped re-base and a neighbouring head's keys.

Every call goes through one runner (run()).  q, k, v - or the fused q | k | v - lie in fp16 buffers with 4 NaN guard rows in front and
behind the slab and, in the "padded" runs, a row pitch of needed + 8 whose extra columns hold NaN: a read outside the slab puts a NaN in
the output.  The output (and lse) is allocated the same way (ldo = C + 8, guard rows, 16 guard floats around lse) and pre-filled with a
NaN bit pattern that no arithmetic produces; afterwards every element outside the slab must still hold it, bit for bit, and every element
inside must be finite.  rc == 0 is asserted and the device synchronised; pt_attn_spatial_set_nqb(2) is undone in a `finally`.

One line per run is printed: the case, the pitches, the worst deviation as a fraction of the bound (B: elements that are not bit-equal);
with PT_ATTN_EXACT=<file> it is also appended to that file (profiles/r17/attn_exact.txt is such a run)."""
import pytest
import torch

from tests import attn_exact as X

pytestmark = pytest.mark.gpu

GUARD = 4                             # NaN rows in front of and behind every slab
LSE_GUARD = 16                        # sentinel floats around lse
PAD = 8
SENTINEL16 = 0x7D5A                   # fp16 NaN with a payload: v_cvt_f16_f32 and the MFMAs return 0x7E00 / 0xFE00
SENTINEL32 = 0x7FC5A5A5               # fp32 NaN with a payload
NAN = float("nan")
PADS = ["tight", "padded"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from posetraj_amd import ops
    d = torch.device("cuda:0")
    ops.ensure_ready(d)
    return d


def stream():
    return torch.cuda.current_stream().cuda_stream


def guarded(mats, ld, dev):
    """Column blocks ``mats`` ([rows, cols] fp16 each, side by side) in a NaN-filled [GUARD + rows + GUARD, ld] device buffer -> (buffer,
    address of the slab's [0, 0])."""
    rows = mats[0].shape[0]
    buf = torch.full((rows + 2 * GUARD, ld), NAN, dtype=torch.float16)
    col = 0
    for m in mats:
        assert m.shape[0] == rows
        buf[GUARD:GUARD + rows, col:col + m.shape[1]] = m
        col += m.shape[1]
    assert col <= ld
    buf = buf.to(dev)
    at = buf.data_ptr() + GUARD * ld * 2
    assert buf.data_ptr() % 256 == 0 and at % 16 == 0
    return buf, at


def sentinel_out(rows, ldo, dev):
    buf = torch.full((rows + 2 * GUARD, ldo), SENTINEL16, dtype=torch.int16, device=dev)
    at = buf.data_ptr() + GUARD * ldo * 2
    assert at % 8 == 0
    return buf, at


def slab_of(buf, rows, cols, what):
    """The [rows, cols] inside of a sentinel-filled output: everything around it untouched (bitwise), everything in it written and
    finite.  -> fp16 CPU"""
    got = buf.cpu()
    inside = got[GUARD:GUARD + rows, :cols].clone().contiguous().view(torch.float16)
    got[GUARD:GUARD + rows, :cols] = SENTINEL16
    touched = (got != SENTINEL16).nonzero()
    assert touched.numel() == 0, f"{what}: written outside the slab at (row, column) {(touched[0] - torch.tensor([GUARD, 0])).tolist()}"
    assert bool(torch.isfinite(inside).all()), f"{what}: an element of the slab is not written, or not finite"
    return inside


def run(dev, case, pad, ldo_pad=None):
    """One call of a case.  -> (o [G, Sq, D] fp16, lse [G, Sq] fp32 or None), after the sentinel checks."""
    from posetraj_amd import hip
    L = hip.lib()
    q, k, v = (X.to_rows(case, t) for t in X.problem(case))
    C = case.heads * case.D
    extra = PAD if pad == "padded" else 0
    ldo = C + (extra if ldo_pad is None else ldo_pad)
    out, optr = sentinel_out(q.shape[0], ldo, dev)
    lse = None
    if case.kernel in ("spatial", "temporal"):
        ld = 3 * C + extra
        a, ap = guarded([q, k, v], ld, dev)
        if case.kernel == "spatial":
            try:
                assert L.pt_attn_spatial_set_nqb(case.nqb) == 0
                rc = L.pt_attn_spatial_f16(ap, ld, C, 2 * C, optr, ldo, case.nb, case.Sq, case.heads, case.D, case.scale, case.pre, stream())
            finally:
                L.pt_attn_spatial_set_nqb(3)
        else:
            rc = L.pt_attn_temporal_f16(ap, ld, C, 2 * C, optr, ldo, case.nb, case.Sq, case.pos, case.heads, case.D, case.scale, stream())
    else:
        if case.fused:
            ld = 3 * C + extra
            a, ap = guarded([q, k, v], ld, dev)
            ptrs, lds = (ap, ap + 2 * C, ap + 4 * C), (ld, ld, ld)
        else:                                                     # three buffers, three pitches
            lds = (C + extra, C + 2 * extra, C + 3 * extra)
            a = [guarded([m], n, dev) for m, n in zip((q, k, v), lds)]
            ptrs = tuple(p for _, p in a)
        args = (ptrs[0], lds[0], ptrs[1], lds[1], ptrs[2], lds[2], optr, ldo, case.nb, case.Sq, case.Sk, case.heads, case.D, case.scale)
        if case.lse:
            n = case.nb * case.Sq * case.heads
            lse = torch.full((n + 2 * LSE_GUARD,), SENTINEL32, dtype=torch.int32, device=dev)
            rc = L.pt_attn_fwd_lse_f16(*args, lse.data_ptr() + 4 * LSE_GUARD, stream())
        else:
            rc = L.pt_attn_f16(*args, stream())
    assert rc == 0, L.pt_last_error().decode()
    torch.cuda.synchronize()
    o = X.from_rows(case, slab_of(out, q.shape[0], C, case.id), case.Sq)
    if lse is not None:
        got = lse.cpu()
        inside = got[LSE_GUARD:LSE_GUARD + n].clone().view(torch.float32)
        got[LSE_GUARD:LSE_GUARD + n] = SENTINEL32
        assert bool((got == SENTINEL32).all()), "lse: written outside [nbatch Sq heads]"
        assert bool(torch.isfinite(inside).all()), "lse: an entry is not written, or not finite"
        lse = inside.view(case.nb, case.Sq, case.heads).permute(0, 2, 1).reshape(case.groups, case.Sq).contiguous()
    return o, lse


def check(dev, case, pad, ldo_pad=None):
    X.self_check(case)
    o, lse = run(dev, case, pad, ldo_pad)
    v = X.judge(case, o, lse)
    X.report(f"{case.id} {pad if ldo_pad is None else f'{pad}, ldo = C + {ldo_pad}'}: {v.text}")
    assert v.ok, v.text


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("case", X.spatial_cases(), ids=lambda c: c.id)
def test_spatial(dev, case, pad):
    check(dev, case, pad)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("case", X.general_cases(), ids=lambda c: c.id)
def test_general(dev, case, pad):
    check(dev, case, pad)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("case", X.d512_cases(), ids=lambda c: c.id)
def test_d512(dev, case, pad):
    check(dev, case, pad)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("case", X.temporal_cases(), ids=lambda c: c.id)
def test_temporal(dev, case, pad):
    check(dev, case, pad)


@pytest.mark.parametrize("case", [X.Case("general", "B", 3, 3, 65, 33, 64), X.Case("general", "Am", 3, 3, 65, 33, 80),
                                  X.Case("general", "B", 3, 3, 65, 33, 128, lse=True), X.Case("d512", "B", 3, 1, 129, 33, 512)], ids=lambda c: c.id)
def test_output_pitch_of_c_plus_4(dev, case):
    """pt_attn_f16 / pt_attn_fwd_lse_f16 store 8 bytes at a time: an output pitch of C + 4 is legal."""
    check(dev, case, "padded", ldo_pad=4)
