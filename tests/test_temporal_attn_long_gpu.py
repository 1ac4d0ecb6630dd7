"""Temporal attention for clips of 33 - 128 frames on the MI355X: pt_attn_temporal_f16's long-clip kernel and the one-launch backward
ptt_attn_temporal_bwd_long_f16 (include/posetraj_temporal.h) through the C ABI, the entry points' ranges, the tape's dispatch, a race
screen, the networks and the denoising loop at 40 frames.

Inputs, helpers and the fp64 gradients are those of tests/test_temporal_bwd_long_gpu.py (``problem``: fp16-representable Q | K | V
and dO, torch fp64 autograd on the CPU); ``rel`` is its rel-L2.

Forward bound.  Reference: torch fp64 softmax(Q K^T / sqrt(d)) V on the CPU over the same fp16 inputs.  A rounding model of the kernel
is computed here on the CPU (``forward_model``: fp32 scores, exp(s - max) rounded to fp16, fp32 product with V divided by the
unrounded fp32 sum, the output rounded to fp16), and calibrated at run time on code this file's subject does not touch: r32 =
(distance of the two-block kernel at (2, 32, 3, 2, hd)) / (the model's distance there).  The long-clip kernel must satisfy
rel <= 1.25 * max(1, r32) * model per case (1.25: the project's customary margin), and with N(0, 1) inputs also rel < 8e-4, the
operator's bound TOL_ATTN of tests/test_kernels_gpu.py (the model alone sits at 2.0e-4 .. 2.7e-4 on these cases).

Backward bound: that of tests/test_temporal_bwd_long_gpu.py unchanged.  Per block dQ / dK / dV <= 1.25 * max(1, r) * (the recomputing
path's distance to fp64 on the same inputs), r = fused / recompute at (2, 32, 7, 2, hd) where both of the parent's paths exist
(pt_attn_temporal_bwd_f16's two-block kernel and autodiff._attention_backward); with N(0, 1) inputs also rel(dqkv) <= 1.5e-3.

Every distance is printed; with PT_TEMPORAL_LONG_PARITY=<file> it is also appended to that file (profiles/r10/
temporal_long_parity.txt is such a run)."""
import functools
import math
import os

import pytest
import torch

from tests.test_temporal_bwd_long_gpu import BLOCKS, MARGIN, REGIMES, padded, per_block, problem, recompute, rel
from tests.test_temporal_bwd_long_gpu import run_kernel as run_short_backward

pytestmark = pytest.mark.gpu

CASES = [(1, 33, 5, 1, 64),          # one frame in the third block; 5 tasks: the last workgroup has dead waves
         (2, 40, 3, 2, 64),          # two clips adjacent in memory: an unmasked read past frame F - 1 of clip 0 lands in clip 1
         (1, 48, 4, 1, 64),          # every block full, no masking
         (1, 64, 2, 3, 128),         # head_dim 128, heads not a power of two
         (2, 127, 2, 1, 64),         # last block one frame short, at the largest block count
         (1, 128, 3, 1, 128),        # the largest LDS footprint
         (1, 100, 1, 2, 128)]        # S = 1
FWD_CALIBRATION = (2, 32, 3, 2)      # (B, F, S, heads): the parent's two-block forward kernel
BWD_CALIBRATION = (2, 32, 7, 2)      # both of the parent's backward paths exist here
TOL_ATTN = 8e-4                      # tests/test_kernels_gpu.py
IDS = lambda c: "x".join(map(str, c))


def report(line: str):
    print(line)
    path = os.environ.get("PT_TEMPORAL_LONG_PARITY")
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


def stream():
    return torch.cuda.current_stream().cuda_stream


def heads_view(case, qkv):
    """[rows, 3 C] -> Q, K, V as [B, S, heads, F, hd]."""
    B, Fr, S, heads, hd = case
    x5 = qkv.view(B, Fr, S, 3, heads, hd)
    return tuple(x5[:, :, :, i].permute(0, 2, 3, 1, 4) for i in range(3))


def rows_view(case, y):
    """[B, S, heads, F, hd] -> [rows, C]."""
    B, Fr, S, heads, hd = case
    return y.permute(0, 3, 1, 2, 4).reshape(B * Fr * S, heads * hd)


@functools.lru_cache(maxsize=None)
def forward_reference(case, regime):
    """fp64 softmax(Q K^T / sqrt(d)) V over the case's fp16 inputs -> [rows, C]; computed once, never modified."""
    q, k, v = heads_view(case, problem(case, regime)[0].double())
    return rows_view(case, torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(case[4]), dim=-1) @ v)


@functools.lru_cache(maxsize=None)
def forward_model(case, regime):
    """The kernels' rounding points on the CPU: fp32 scores, P = exp(s - max) rounded to fp16, fp32 P V divided by the fp32 sum of
    the unrounded P, the output rounded to fp16 -> [rows, C] fp16."""
    q, k, v = heads_view(case, problem(case, regime)[0].float())
    s = (q @ k.transpose(-1, -2)) * (case[4] ** -0.5)
    p = torch.exp(s - s.amax(dim=-1, keepdim=True))
    o = (p.half().float() @ v) / p.sum(dim=-1, keepdim=True)
    return rows_view(case, o.half())


def run_forward(dev, case, regime, pad):
    """pt_attn_temporal_f16 through the raw binding into a NaN-filled output -> the whole buffer [rows, ldo]."""
    from posetraj_amd import hip
    B, Fr, S, heads, hd = case
    Cc = heads * hd
    qkv = problem(case, regime)[0]
    ld, ldo = (3 * Cc + 8, Cc + 8) if pad else (3 * Cc, Cc)
    a = padded(qkv, ld, dev)
    out = torch.full((qkv.shape[0], ldo), float("nan"), dtype=torch.float16, device=dev)
    rc = hip.lib().pt_attn_temporal_f16(a.data_ptr(), ld, Cc, 2 * Cc, out.data_ptr(), ldo, B, Fr, S, heads, hd, hd ** -0.5, stream())
    assert rc == 0, hip.lib().pt_last_error().decode()
    torch.cuda.synchronize()
    return out


def run_backward(dev, case, regime, pad):
    """ptt_attn_temporal_bwd_long_f16 through the raw binding into a NaN-filled gradient buffer -> the whole buffer [rows, ldd]."""
    from posetraj_amd import hip
    B, Fr, S, heads, hd = case
    Cc = heads * hd
    qkv, dy, _ = problem(case, regime)
    ld, ldo, ldd = (3 * Cc + 8, Cc + 8, 3 * Cc + 4) if pad else (3 * Cc, Cc, 3 * Cc)
    a, b = padded(qkv, ld, dev), padded(dy, ldo, dev)
    out = torch.full((qkv.shape[0], ldd), float("nan"), dtype=torch.float16, device=dev)
    rc = hip.lib().ptt_attn_temporal_bwd_long_f16(a.data_ptr(), ld, Cc, 2 * Cc, b.data_ptr(), ldo, out.data_ptr(), ldd, B, Fr, S, heads, hd,
                                                  hd ** -0.5, stream())
    assert rc == 0, hip.lib().pt_last_error().decode()
    torch.cuda.synchronize()
    return out


_r32_fwd, _r32_bwd = {}, {}


def r32_forward(dev, hd, regime):
    """(two-block forward kernel's distance to fp64) / (the model's) at 32 frames."""
    if (hd, regime) not in _r32_fwd:
        case = FWD_CALIBRATION + (hd,)
        want = forward_reference(case, regime)
        kernel, model = rel(run_forward(dev, case, regime, False), want), rel(forward_model(case, regime), want)
        _r32_fwd[(hd, regime)] = kernel / model
        report(f"forward calibration {case} {regime}: two-block kernel {kernel:.3e}; model {model:.3e}; r32 {kernel / model:.3f}")
    return _r32_fwd[(hd, regime)]


def r32_backward(AD, dev, hd, regime):
    """fused / recompute distance to fp64 per block at 32 frames: the two paths of the parent commit."""
    if (hd, regime) not in _r32_bwd:
        case = BWD_CALIBRATION + (hd,)
        Cc = case[3] * hd
        want = problem(case, regime)[2]
        fused = per_block(run_short_backward(dev, case, regime, False), want, Cc)
        rec = per_block(recompute(AD, dev, case, regime), want, Cc)
        _r32_bwd[(hd, regime)] = [f / r for f, r in zip(fused, rec)]
        report(f"backward calibration {case} {regime}: two-block kernel " + " ".join(f"{n} {v:.3e}" for n, v in zip(BLOCKS, fused)) + "; recompute " +
               " ".join(f"{n} {v:.3e}" for n, v in zip(BLOCKS, rec)) + "; r32 " + " ".join(f"{v:.3f}" for v in _r32_bwd[(hd, regime)]))
    return _r32_bwd[(hd, regime)]


def check_blocks(AD, dev, case, regime, got, label):
    """Prints, then asserts, the per-block bound of the header (and the operator's 1.5e-3 in the N(0, 1) regime)."""
    Cc = case[3] * case[4]
    want = problem(case, regime)[2]
    mine = per_block(got, want, Cc)
    rec = per_block(recompute(AD, dev, case, regime), want, Cc)
    ratio = r32_backward(AD, dev, case[4], regime)
    bound = [MARGIN * max(1.0, r) * d for r, d in zip(ratio, rec)]
    total = rel(got[:, :3 * Cc], want)
    report(f"{label} {case} {regime}: dqkv {total:.3e}; " + "; ".join(f"{n} fused {m:.3e} recompute {d:.3e} bound {b:.3e}"
                                                                     for n, m, d, b in zip(BLOCKS, mine, rec, bound)))
    if regime == "normal":
        assert total <= 1.5e-3
    for n, m, b in zip(BLOCKS, mine, bound):
        assert m <= b, (n, m, b)


# ------------------------------------------------------------------------------------------------- a. forward against fp64
@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("pad", [False, True], ids=["tight", "padded"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_against_fp64(dev, case, pad, regime):
    Cc = case[3] * case[4]
    out = run_forward(dev, case, regime, pad)
    assert bool(torch.isfinite(out[:, :Cc]).all()), "every output column of every row is written"
    assert bool(torch.isnan(out[:, Cc:]).all()), "padding columns are not touched"
    want = forward_reference(case, regime)
    mine, model = rel(out[:, :Cc], want), rel(forward_model(case, regime), want)
    bound = MARGIN * max(1.0, r32_forward(dev, case[4], regime)) * model
    report(f"forward, {'padded' if pad else 'tight'} pitches {case} {regime}: kernel {mine:.3e} model {model:.3e} bound {bound:.3e}")
    if regime == "normal":
        assert mine < TOL_ATTN
    assert mine <= bound, (mine, bound)


# ------------------------------------------------------------------------------------------------- b. backward against fp64 autograd
@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("pad", [False, True], ids=["tight", "padded"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_backward_against_fp64(dev, AD, case, pad, regime):
    Cc = case[3] * case[4]
    out = run_backward(dev, case, regime, pad)
    assert bool(torch.isfinite(out[:, :3 * Cc]).all()), "every [Q|K|V] column of every row is written"
    assert bool(torch.isnan(out[:, 3 * Cc:]).all()), "padding columns are not touched"
    check_blocks(AD, dev, case, regime, out, "backward, padded pitches" if pad else "backward, tight pitches")


# ------------------------------------------------------------------------------------------------- c. ranges
def test_frame_and_head_ranges_of_the_entry_points(dev):
    """Every refusal is a host-side check before any launch."""
    from posetraj_amd import hip
    L = hip.lib()

    def buffers(Fr, hd):
        rows = max(Fr, 1)
        return (torch.zeros((rows, 3 * hd), dtype=torch.float16, device=dev), torch.zeros((rows, hd), dtype=torch.float16, device=dev),
                torch.empty((rows, 3 * hd), dtype=torch.float16, device=dev))

    def forward(Fr, hd=64):
        a, _, _ = buffers(Fr, hd)
        o = torch.empty((a.shape[0], hd), dtype=torch.float16, device=dev)
        return L.pt_attn_temporal_f16(a.data_ptr(), 3 * hd, hd, 2 * hd, o.data_ptr(), hd, 1, Fr, 1, 1, hd, hd ** -0.5, stream())

    def backward(fn, Fr, hd=64):
        a, b, g = buffers(Fr, hd)
        return fn(a.data_ptr(), 3 * hd, hd, 2 * hd, b.data_ptr(), hd, g.data_ptr(), 3 * hd, 1, Fr, 1, 1, hd, hd ** -0.5, stream())

    assert forward(128) == 0
    for Fr in (129, 0):
        assert forward(Fr) != 0
        msg = L.pt_last_error().decode()
        assert "1..128" in msg and f"{Fr} frames" in msg, msg
    for Fr in (32, 129):
        assert backward(L.ptt_attn_temporal_bwd_long_f16, Fr) != 0
        msg = L.pt_last_error().decode()
        assert "ptt_attn_temporal_bwd_long_f16" in msg and "33..128" in msg and f"{Fr} frames" in msg, msg
    assert backward(L.ptt_attn_temporal_bwd_long_f16, 40, hd=80) != 0
    msg = L.pt_last_error().decode()
    assert "ptt_attn_temporal_bwd_long_f16" in msg and "head_dim 80" in msg, msg
    assert backward(L.pt_attn_temporal_bwd_f16, 33) != 0
    msg = L.pt_last_error().decode()
    assert "1..32" in msg and "33 frames" in msg, msg
    assert backward(L.ptt_attn_temporal_bwd_long_f16, 33) == 0 and backward(L.ptt_attn_temporal_bwd_long_f16, 128, hd=128) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- d. dispatch
def tape_backward(AD, dev, case, regime="normal"):
    B, Fr, S, heads, hd = case
    qkv, dy, _ = problem(case, regime)
    tape = AD.Tape()
    xv = AD.Var(qkv.to(dev))
    o = AD.attn_temporal(tape, xv, B, Fr, S, heads, hd)
    o.g = dy.to(dev)
    tape.backward()
    return xv.g


def test_tape_takes_the_long_kernel_when_the_switch_is_on(dev, AD, monkeypatch):
    case = (1, 40, 12, 2, 64)

    def forbidden(*a, **k):
        raise AssertionError("the recomputing path was taken")
    with monkeypatch.context() as m:
        m.setattr(AD, "_attention_backward", forbidden)
        m.setattr(AD, "TEMPORAL_LONG_BACKWARD", True)
        got = tape_backward(AD, dev, case)
        m.setattr(AD, "TEMPORAL_LONG_BACKWARD", False)
        with pytest.raises(AssertionError, match="recomputing path"):
            tape_backward(AD, dev, case)
    check_blocks(AD, dev, case, "normal", got, "tape")


def test_tape_keeps_the_two_block_kernel_at_25_frames(dev, AD, monkeypatch):
    from posetraj_amd import hip
    C = hip.checked()
    calls = {"short": 0, "long": 0}
    short, long_ = C.pt_attn_temporal_bwd_f16, C.ptt_attn_temporal_bwd_long_f16

    class Counting:
        """The checked library with the two temporal backward entry points counted."""
        def __getattr__(self, name):
            return getattr(C, name)

        def pt_attn_temporal_bwd_f16(self, *a):
            calls["short"] += 1
            return short(*a)

        def ptt_attn_temporal_bwd_long_f16(self, *a):
            calls["long"] += 1
            return long_(*a)

    counting = Counting()
    monkeypatch.setattr(AD, "TEMPORAL_LONG_BACKWARD", True)
    monkeypatch.setattr(AD.hip, "checked", lambda: counting)
    g = tape_backward(AD, dev, (1, 25, 12, 2, 64))
    assert calls == {"short": 1, "long": 0} and bool(torch.isfinite(g).all())
    tape_backward(AD, dev, (1, 40, 12, 2, 64))
    assert calls == {"short": 1, "long": 1}


# ------------------------------------------------------------------------------------------------- e. race screen
@pytest.mark.parametrize("case", [(2, 40, 3, 2, 64), (2, 127, 2, 1, 64)], ids=IDS)
def test_runs_agree_bit_for_bit(dev, case):
    """Both kernels stage rows through LDS behind wave barriers (the backward twice into the same slab): a read ahead of a write would
    show as a run-to-run difference."""
    fwd = [run_forward(dev, case, "normal", False) for _ in range(5)]
    assert all(torch.equal(fwd[0], o) for o in fwd[1:])
    bwd = [run_backward(dev, case, "normal", False) for _ in range(5)]
    assert all(torch.equal(bwd[0], o) for o in bwd[1:])


# ------------------------------------------------------------------------------------------------- f. networks
FRAMES = 40


def test_unet_forward_with_controlnet_residuals_at_40_frames(dev):
    """The tiny U-Net of tests/test_backward_gpu.py on an 8 x 8 latent, residuals from the oracle ControlNet: within 1e-3 rel-L2 of
    the fp32 oracle."""
    from tests import parity as P
    from tests.test_backward_gpu import _nets
    cn_o, un_o, un, _ = _nets(dev)
    i = P.tiny_inputs(seed=190, B=2, F=FRAMES, h=8, w=8, xdim=16)
    with torch.no_grad():
        down_o, mid_o = cn_o(i["sample"], i["t"], i["ehs"], i["ids"], controlnet_cond=i["cond"], return_dict=False)
        y_o = un_o(i["sample"], i["t"], i["ehs"], down_o, mid_o, return_dict=False, added_time_ids=i["ids"])[0]
    y = un(i["sample"].half().to(dev), i["t"].to(dev), i["ehs"].half().to(dev), [d.half().to(dev) for d in down_o], mid_o.half().to(dev),
           return_dict=False, added_time_ids=i["ids"].to(dev))[0]
    assert tuple(y.shape) == tuple(y_o.shape) == (2, FRAMES, 4, 8, 8)
    r = P.rel_l2(y, y_o)
    report(f"U-Net forward, {FRAMES} frames, 8 x 8 latent: rel-L2 to the fp32 oracle {r:.3e}")
    assert bool(torch.isfinite(y).all()) and r < 1e-3, r


def test_training_step_gradients_at_40_frames(dev, AD, monkeypatch):
    """ControlNetTrainer.loss_and_grads (tiny networks, 8 x 8 latent, spatial loss on) vs fp32 autograd over the oracle, at the step
    level tolerances of tests/test_backward_gpu.py's header (all gradients 5e-3, every sizeable tensor 2e-2, losses 1e-3) - and
    against the same step through the recomputing path (TEMPORAL_LONG_BACKWARD off), which it may exceed by the margin only.  Then
    deterministic=True twice: equal gradients."""
    from oracle import train as OT
    from posetraj_amd.training import ControlNetTrainer
    from tests.test_backward_gpu import _compare_grads, _nets
    Fr = FRAMES
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
    for name, on in (("fused", True), ("recompute", False)):
        monkeypatch.setattr(AD, "TEMPORAL_LONG_BACKWARD", on)
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
    monkeypatch.setattr(AD, "TEMPORAL_LONG_BACKWARD", True)
    grads = []
    for _ in range(2):
        tr = ControlNetTrainer(cfg, cn_o.state_dict(), un, conditioning_dropout_prob=0.1, loss_scale=4096.0, deterministic=True)
        tr.loss_and_grads(lat, emb, mv, traj, noise=noise, sigmas=sig, random_p=rp, ran_idx=ri)
        grads.append({k: v.clone() for k, v in tr.gradients().items()})
    assert sorted(grads[0]) == sorted(grads[1]) and all(torch.equal(grads[0][k], grads[1][k]) for k in grads[0])


# ------------------------------------------------------------------------------------------------- g. pipeline
def test_denoise_at_40_frames_graph_equals_eager(dev):
    """denoise on the tiny networks, 40 frames, 2 steps: the captured graph with overlapped streams equals the eager launches bit for
    bit (as tests/test_model_gpu.py asserts at 14 frames) and the result is finite."""
    from posetraj_amd import EulerDiscreteScheduler, StableVideoDiffusionPipelineControlNet, SVD_SCHEDULER_CONFIG
    from tests import parity as P
    cn_o, unet_o = P.build_oracle_nets(seed=12)
    cn_h, unet_h = P.build_hip_nets(cn_o, unet_o, dev)
    pipe = StableVideoDiffusionPipelineControlNet(unet=unet_h, controlnet=cn_h, scheduler=EulerDiscreteScheduler(**SVD_SCHEDULER_CONFIG))
    g = torch.Generator().manual_seed(340)
    lat = (torch.randn(1, FRAMES, 4, 8, 8, generator=g) * 700).to(dev)
    mode = torch.randn(1, 4, 8, 8, generator=g).half()
    il = torch.cat([torch.zeros_like(mode), mode]).to(dev)
    e = torch.randn(1, 1, 64, generator=g).half()
    emb = torch.cat([torch.zeros_like(e), e]).to(dev)
    c1 = (torch.rand(1, FRAMES, 3, 64, 64, generator=g) * 2 - 1).half()
    cond = torch.cat([c1, c1]).to(dev)
    out_g = pipe.denoise(lat, il, emb, cond, num_inference_steps=2, use_graph=True, overlap_streams=True)
    out_e = pipe.denoise(lat, il, emb, cond, num_inference_steps=2, use_graph=False, overlap_streams=False)
    assert tuple(out_g.shape) == (1, FRAMES, 4, 8, 8) and bool(torch.isfinite(out_g).all())
    assert torch.equal(out_g, out_e)
