"""pt_attn_temporal_bwd_f16 for clips of 17 - 32 frames (SVD-XT: 25) on the MI355X: the two-block kernel through the C ABI, the
tape's dispatch, a race screen and the composed training step.

Reference: torch fp64 autograd of softmax(Q K^T / sqrt(d)) V on the CPU over the same fp16-representable inputs; ``rel`` is the
rel-L2 of tests/test_backward_gpu.py.

Bounds.  N(0, 1) inputs: rel(dqkv) <= 1.5e-3, what test_temporal_attention_backward_against_sdpa_autograd asserts for this operator.
dQ, dK and dV separately, in both input regimes (N(0, 1); Q and K scaled by 3 - a peaked softmax): calibrated at run time on code
this file's subject does not touch.  At (2, 16, 7, 2, hd) both the one-block kernel (F <= 16) and the recomputing path
(autodiff._attention_backward) exist; r16 = fused / recompute of their distances to fp64, per block.  For F > 16 the new kernel's
distance per block must be <= 1.25 * max(1, r16) * the recomputing path's distance on the very same inputs (both paths round P
and dS to fp16 once and accumulate in fp32, so the ratio sits near 1; 1.25 is the project's customary margin).

Every distance is printed; with PT_TEMPORAL_BWD_PARITY=<file> it is also appended to that file (profiles/r07/
temporal_bwd_long_parity.txt is such a run)."""
import functools
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = [(1, 17, 5, 1, 64),          # one frame in the second block; 5 tasks: the last workgroup has one live wave
         (2, 25, 7, 2, 64),          # SVD-XT's count; two clips adjacent in memory: a read past frame F - 1 of clip 0 lands in clip 1
         (1, 32, 4, 1, 64),          # both blocks full, no masking
         (1, 25, 3, 1, 128), (2, 31, 2, 3, 128)]                          # the head_dim 128 instance (two waves per workgroup)
CALIBRATION = (2, 16, 7, 2)          # (B, F, S, heads): both of the parent's paths exist here
REGIMES = {"normal": 1.0, "peaked": 3.0}                                 # scale of Q and K
BLOCKS = ("dQ", "dK", "dV")
MARGIN = 1.25


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def report(line: str):
    print(line)
    path = os.environ.get("PT_TEMPORAL_BWD_PARITY")
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


def h16(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half()


@functools.lru_cache(maxsize=None)
def problem(case, regime):
    """(qkv [rows, 3 C] fp16, dout [rows, C] fp16, fp64 gradient [rows, 3 C]) of a case; computed once, never modified."""
    B, Fr, S, heads, hd = case
    Cc = heads * hd
    qkv = h16(B * Fr * S, 3 * Cc, seed=144 + Fr)
    qkv[:, :2 * Cc] = (qkv[:, :2 * Cc].float() * REGIMES[regime]).half()
    dy = h16(B * Fr * S, Cc, seed=145 + Fr)
    xr = qkv.double().requires_grad_(True)
    x5 = xr.view(B, Fr, S, 3, heads, hd)
    q, k, v = (x5[:, :, :, i].permute(0, 2, 3, 1, 4) for i in range(3))                       # [B, S, heads, F, hd]
    p = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(hd), dim=-1)
    y = (p @ v).permute(0, 3, 1, 2, 4).reshape(B * Fr * S, Cc)
    y.backward(dy.double())
    return qkv, dy, xr.grad.detach()


def padded(t, ld, dev):
    """t's rows at pitch ld on the device; the padding columns hold NaN."""
    buf = torch.full((t.shape[0], ld), float("nan"), dtype=torch.float16, device=dev)
    buf[:, :t.shape[1]] = t.to(dev)
    return buf


def run_kernel(dev, case, regime, pad):
    """pt_attn_temporal_bwd_f16 through the raw binding into a NaN-filled gradient buffer -> the whole buffer [rows, ldd]."""
    from posetraj_amd import hip
    B, Fr, S, heads, hd = case
    Cc = heads * hd
    qkv, dy, _ = problem(case, regime)
    ld, ldo, ldd = (3 * Cc + 8, Cc + 8, 3 * Cc + 4) if pad else (3 * Cc, Cc, 3 * Cc)
    a, b = padded(qkv, ld, dev), padded(dy, ldo, dev)
    out = torch.full((qkv.shape[0], ldd), float("nan"), dtype=torch.float16, device=dev)
    rc = hip.lib().pt_attn_temporal_bwd_f16(a.data_ptr(), ld, Cc, 2 * Cc, b.data_ptr(), ldo, out.data_ptr(), ldd, B, Fr, S, heads, hd, hd ** -0.5,
                                            torch.cuda.current_stream().cuda_stream)
    assert rc == 0, hip.lib().pt_last_error().decode()
    torch.cuda.synchronize()
    return out


def recompute(AD, dev, case, regime):
    """The recomputing path on the case's own tight-pitch inputs (no tape)."""
    B, Fr, S, heads, hd = case
    qkv, dy, _ = problem(case, regime)
    return AD._attention_backward(qkv.to(dev), dy.to(dev), heads * hd, heads, hd, Fr, S, (B, Fr * S, S, 1), 1)


def per_block(got, want, Cc):
    return [rel(got[:, i * Cc:(i + 1) * Cc], want[:, i * Cc:(i + 1) * Cc]) for i in range(3)]


_r16 = {}


def r16(AD, dev, hd, regime):
    """fused / recompute distance to fp64 per block at 16 frames: the two paths of the parent commit."""
    if (hd, regime) not in _r16:
        case = CALIBRATION + (hd,)
        Cc = case[3] * hd
        want = problem(case, regime)[2]
        fused = per_block(run_kernel(dev, case, regime, False), want, Cc)
        rec = per_block(recompute(AD, dev, case, regime), want, Cc)
        _r16[(hd, regime)] = [f / r for f, r in zip(fused, rec)]
        report(f"calibration {case} {regime}: one-block kernel " + " ".join(f"{n} {v:.3e}" for n, v in zip(BLOCKS, fused)) + "; recompute " +
               " ".join(f"{n} {v:.3e}" for n, v in zip(BLOCKS, rec)) + "; r16 " + " ".join(f"{v:.3f}" for v in _r16[(hd, regime)]))
    return _r16[(hd, regime)]


def check_blocks(AD, dev, case, regime, got, label):
    """Prints, then asserts, the per-block bound of the header (and the operator's 1.5e-3 in the N(0, 1) regime)."""
    Cc = case[3] * case[4]
    want = problem(case, regime)[2]
    mine = per_block(got, want, Cc)
    rec = per_block(recompute(AD, dev, case, regime), want, Cc)
    ratio = r16(AD, dev, case[4], regime)
    bound = [MARGIN * max(1.0, r) * d for r, d in zip(ratio, rec)]
    total = rel(got[:, :3 * Cc], want)
    report(f"{label} {case} {regime}: dqkv {total:.3e}; " + "; ".join(f"{n} fused {m:.3e} recompute {d:.3e} bound {b:.3e}"
                                                                     for n, m, d, b in zip(BLOCKS, mine, rec, bound)))
    if regime == "normal":
        assert total <= 1.5e-3
    for n, m, b in zip(BLOCKS, mine, bound):
        assert m <= b, (n, m, b)


# ------------------------------------------------------------------------------------------------- a. the kernel against fp64
@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("pad", [False, True], ids=["tight", "padded"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_kernel_against_fp64(dev, AD, case, pad, regime):
    Cc = case[3] * case[4]
    out = run_kernel(dev, case, regime, pad)
    assert bool(torch.isfinite(out[:, :3 * Cc]).all()), "every [Q|K|V] column of every row is written"
    assert bool(torch.isnan(out[:, 3 * Cc:]).all()), "padding columns are not touched"
    check_blocks(AD, dev, case, regime, out, "kernel, padded pitches" if pad else "kernel, tight pitches")


# ------------------------------------------------------------------------------------------------- b. range
def test_frame_range_of_the_entry_point(dev):
    from posetraj_amd import hip
    L = hip.lib()
    hd = 64
    a = torch.zeros((32, 3 * hd), dtype=torch.float16, device=dev)
    b = torch.zeros((32, hd), dtype=torch.float16, device=dev)
    out = torch.empty_like(a)
    call = lambda Fr: L.pt_attn_temporal_bwd_f16(a.data_ptr(), 3 * hd, hd, 2 * hd, b.data_ptr(), hd, out.data_ptr(), 3 * hd, 1, Fr, 1, 1, hd, hd ** -0.5,
                                                 torch.cuda.current_stream().cuda_stream)
    for Fr in (33, 0):
        assert call(Fr) != 0
        msg = L.pt_last_error().decode()
        assert "1..32" in msg and f"{Fr} frames" in msg, msg
    assert call(32) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- c. dispatch
def test_tape_takes_the_fused_kernel_up_to_32_frames(dev, AD, monkeypatch):
    case, regime = (1, 25, 12, 2, 64), "normal"
    B, Fr, S, heads, hd = case
    qkv, dy, _ = problem(case, regime)

    def backward():
        tape = AD.Tape()
        xv = AD.Var(qkv.to(dev))
        o = AD.attn_temporal(tape, xv, B, Fr, S, heads, hd)
        o.g = dy.to(dev)
        tape.backward()
        return xv.g

    def forbidden(*a, **k):
        raise AssertionError("the recomputing path was taken")
    with monkeypatch.context() as m:
        m.setattr(AD, "_attention_backward", forbidden)
        got = backward()
        m.setattr(AD, "TEMPORAL_FLASH_FRAMES", 16)
        with pytest.raises(AssertionError, match="recomputing path"):
            backward()
    check_blocks(AD, dev, case, regime, got, "tape")


# ------------------------------------------------------------------------------------------------- d. race screen
@pytest.mark.parametrize("case", [(2, 25, 7, 2, 64), (2, 31, 2, 3, 128)], ids=lambda c: "x".join(map(str, c)))
def test_runs_agree_bit_for_bit(dev, case):
    """The kernel stages rows through LDS behind a wave barrier: a read ahead of the write would show as a run-to-run difference."""
    outs = [run_kernel(dev, case, "normal", False) for _ in range(5)]
    assert all(torch.equal(outs[0], o) for o in outs[1:])


# ------------------------------------------------------------------------------------------------- e. the composed step
@pytest.mark.parametrize("Fr", [25, 17])
def test_training_step_gradients_with_more_than_16_frames(dev, AD, monkeypatch, Fr):
    """ControlNetTrainer.loss_and_grads (tiny networks, 8 x 8 latent, spatial loss on) vs fp32 autograd over the oracle, at the step
    level tolerances of tests/test_backward_gpu.py's header (all gradients 5e-3, every sizeable tensor 2e-2, losses 1e-3) - and
    against the same step through the recomputing path (TEMPORAL_FLASH_FRAMES = 16), which it may exceed by the margin only."""
    from oracle import train as OT
    from posetraj_amd.training import ControlNetTrainer
    from tests.test_backward_gpu import _compare_grads, _nets
    cn_o, un_o, un, cfg = _nets(dev)
    g = torch.Generator().manual_seed(170 + Fr)
    h = w = 8
    lat = (torch.randn(1, Fr, 4, h, w, generator=g) * 0.18215 * 5).half().float()
    emb = torch.randn(1, 1, 16, generator=g).half().float()
    traj = (torch.rand(1, Fr, 3, h * 8, w * 8, generator=g) * 2 - 1).half().float()
    noise = torch.randn(lat.shape, generator=g)
    sig, rp, ri, mv = torch.tensor([1.3]), torch.tensor([0.7]), Fr // 2 + 1, torch.tensor([127.0])
    ro = OT.training_step_grads(cn_o, un_o, lat, noise, sig, emb, mv, traj, 0.18215, random_p=rp, conditioning_dropout_prob=0.1, ran_idx=ri)
    res = {}
    for name, frames in (("fused", 32), ("recompute", 16)):
        monkeypatch.setattr(AD, "TEMPORAL_FLASH_FRAMES", frames)
        tr = ControlNetTrainer(cfg, cn_o.state_dict(), un, conditioning_dropout_prob=0.1, loss_scale=4096.0)
        r = tr.loss_and_grads(lat, emb, mv, traj, noise=noise, sigmas=sig, random_p=rp, ran_idx=ri)
        rl, rs = abs(r["loss"] / float(ro["loss"]) - 1), abs(r["loss_spatial"] / float(ro["loss_spatial"]) - 1)
        total, worst = _compare_grads(tr.gradients(), ro["grads"], f"training step, {name} ({Fr} frames, {h} x {w} latent)")
        res[name] = (total, worst, rl, rs)
        report(f"training step {Fr} frames, {name}: all gradients {total:.3e}; worst sizeable tensor {worst:.3e}; loss {rl:.1e}; spatial loss {rs:.1e}")
    total, worst, rl, rs = res["fused"]
    assert rl < 1e-3 and rs < 1e-3
    assert total <= 5e-3 and worst <= 2e-2
    assert total <= MARGIN * res["recompute"][0]


def test_one_position_spatial_attention_has_exactly_zero_query_and_key_gradients(dev, AD):
    """What the step test above needs of the mid block of an 8 x 8 latent (S = 1, there with 25 frames): softmax over one key is 1, so
    dQ = dK = 0 exactly and dV = dO - not the rounding residue of dP - sum_d dO O."""
    N, heads, hd = 25, 2, 64
    Cc = heads * hd
    qkv, dy = h16(N, 3 * Cc, seed=180).to(dev), (h16(N, Cc, seed=181) * 64).to(dev)
    tape = AD.Tape()
    xv = AD.Var(qkv)
    o = AD.attn_spatial(tape, xv, N, 1, heads, hd)
    o.g = dy
    tape.backward()
    assert float(xv.g[:, :2 * Cc].abs().max()) == 0.0 and torch.equal(xv.g[:, 2 * Cc:], dy)
