"""SURVEY 8(f)4 on the MI355X: the training step's reverse pass - pt_gemm_f16, the kernels of csrc/norm_bwd.hip, pointwise_bwd.hip and optim.hip, the tape
primitives of posetraj_amd/autodiff.py and ControlNetTrainer - through the C ABI against torch autograd on the CPU (fp32, over
the same fp16-representable inputs) and against the reference-run fixture tests/golden/train_grads.npz.

Tolerances.  Kernel level: fp16 operands, fp32 accumulation, one fp16 rounding of each output -> rel-L2 <= 1e-3 (weight
gradients are fp32 outputs: <= 3e-4).  Step level: every activation gradient is stored in fp16 along a reverse path as deep as
the forward, so a parameter gradient carries the forward's rounding noise (1e-3 class) twice over; asserted:
global gradient (all parameters concatenated) rel-L2 <= 5e-3 against fp32 autograd, per parameter <= 2e-2 for tensors whose
gradient norm is not negligible, losses as in the forward test."""
import contextlib
import io
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def AD():
    from posetraj_amd import autodiff
    return autodiff


def h16(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half()


# ------------------------------------------------------------------------------------------------- pt_gemm_f16
@pytest.mark.parametrize("M,N,K,ta,tb", [(128, 128, 64, 0, 0), (100, 72, 50, 0, 1), (257, 130, 333, 1, 0), (14, 14, 64, 0, 1), (14, 64, 14, 1, 0),
                                         (64, 64, 2880, 1, 0), (300, 64, 200, 1, 1), (1, 5, 7, 0, 0), (320, 320, 4096, 1, 0)])
def test_gemm_all_transposes(dev, AD, M, N, K, ta, tb):
    """C = A B with A stored [M, K] or [K, M], B stored [K, N] or [N, K]; ragged sizes take the scalar tails."""
    A, B = h16(M, K, seed=1), h16(K, N, seed=2)
    want = A.float() @ B.float()
    a = (A.t().contiguous() if ta else A).to(dev)
    b = (B.t().contiguous() if tb else B).to(dev)
    c = torch.empty((M, N), dtype=torch.float32, device=dev)
    AD.gemm((a, 0), (b, 0), (c, 0), M, N, K, (1, M) if ta else (K, 1), (1, K) if tb else (N, 1), (N, 1), out_mode=1)
    assert rel(c, want) < 2e-6 * math.sqrt(K) + 1e-6
    c16 = torch.empty((M, N), dtype=torch.float16, device=dev)
    AD.gemm((a, 0), (b, 0), (c16, 0), M, N, K, (1, M) if ta else (K, 1), (1, K) if tb else (N, 1), (N, 1), alpha=0.5)
    assert rel(c16, 0.5 * want) < 5e-4
    if K >= 512:                                              # split-K accumulates with atomics into a pre-filled fp32 buffer
        c = torch.ones((M, N), dtype=torch.float32, device=dev)
        AD.gemm((a, 0), (b, 0), (c, 0), M, N, K, (1, M) if ta else (K, 1), (1, K) if tb else (N, 1), (N, 1), out_mode=2, splits=7)
        assert rel(c - 1, want) < 1e-5


def test_gemm_three_level_batches_inside_a_fused_projection(dev, AD):
    """Q K^T of (clip, position, head) batches addressed in place inside a [rows, 3 C] projection, tokens a row stride apart
    (the temporal attention's addressing) - against an explicit gather."""
    Bc, Fr, S, heads, hd = 2, 5, 6, 3, 16
    Cc = heads * hd
    qkv = h16(Bc * Fr * S, 3 * Cc, seed=3)
    d = qkv.to(dev)
    out = torch.empty((Bc * S * heads, Fr, Fr), dtype=torch.float32, device=dev)
    ld = 3 * Cc
    AD.gemm((d, 0), (d, Cc), (out, 0), Fr, Fr, hd, (S * ld, 1), (1, S * ld), (Fr, 1), nb=(Bc, S, heads), ba=(Fr * S * ld, ld, hd),
            bb=(Fr * S * ld, ld, hd), bc=(S * heads * Fr * Fr, heads * Fr * Fr, Fr * Fr), alpha=0.25, out_mode=1)
    x = qkv.float().view(Bc, Fr, S, 3, heads, hd)
    q, k = x[:, :, :, 0].permute(0, 2, 3, 1, 4), x[:, :, :, 1].permute(0, 2, 3, 1, 4)          # [B, S, heads, F, hd]
    want = 0.25 * q @ k.transpose(-1, -2)
    assert rel(out.view(Bc, S, heads, Fr, Fr), want) < 1e-5


@pytest.mark.parametrize("Ci,Co,N,H,W,k,stride,pad", [(16, 32, 2, 9, 7, 3, 1, 1), (8, 24, 3, 10, 12, 3, 2, 1), (3, 16, 2, 8, 8, 3, 1, 1), (64, 64, 1, 5, 6, 1, 1, 0),
                                                      (320, 320, 2, 16, 16, 3, 1, 1)])
def test_conv_weight_gradient_against_autograd(dev, AD, Ci, Co, N, H, W, k, stride, pad):
    """Dense.accumulate (pt_gemm_f16 with the convolution gather, split-K atomics into the [Co, Ci, kh, kw] tensor) and the
    bias gradient (pt_colsum_f16) vs torch autograd; Ci = 3 is the condition encoder's padded-to-8 input."""
    x = h16(N, Ci, H, W, seed=4)
    w = torch.randn(Co, Ci, k, k, generator=torch.Generator().manual_seed(5)).half().float().requires_grad_(True)
    bias = torch.zeros(Co, requires_grad=True)
    y = F.conv2d(x.float(), w, bias, stride=stride, padding=pad)
    dy = h16(*y.shape, seed=6)
    y.backward(dy.float())
    P = AD.ParamStore({"w": w.detach(), "b": bias.detach()}, dev)
    L = AD.Dense(P, "w", "b", kind="conv", stride=stride, padding=pad)
    cp = (Ci + 7) // 8 * 8
    xcl = torch.zeros(N, H, W, cp, dtype=torch.float16)
    xcl[..., :Ci] = x.permute(0, 2, 3, 1)
    dycl = dy.permute(0, 2, 3, 1).contiguous().view(-1, Co)
    for _ in range(2):                                        # gradients accumulate
        L.accumulate(xcl.view(-1, cp).to(dev), dycl.to(dev), (N, H, W))
    assert rel(P.gradient("w"), 2 * w.grad) < 3e-4
    assert rel(P.gradient("b"), 2 * bias.grad) < 3e-4


def test_linear_and_temporal_conv_weight_gradients(dev, AD):
    M, K, N = 700, 96, 40
    x, dy = h16(M, K, seed=7), h16(M, N, seed=8)
    P = AD.ParamStore({"q": torch.zeros(N // 2, K), "k": torch.zeros(N // 2, K), "t": torch.zeros(24, 16, 3, 1, 1), "tb": torch.zeros(24)}, dev)
    L = AD.Dense(P, "q", None, stack=("q", "k"))
    L.accumulate(x.to(dev), dy.to(dev), None)
    want = dy.float().t() @ x.float()
    assert rel(P.gradient("q"), want[:N // 2]) < 3e-4 and rel(P.gradient("k"), want[N // 2:]) < 3e-4
    # Conv3d (3,1,1) over [B, C, F, h, w] == (3 x 1) convolution over the image (F, S)
    Bc, Fr, S, Ci, Co = 2, 5, 12, 16, 24
    xt = h16(Bc, Ci, Fr, S, 1, seed=9)
    w = torch.randn(Co, Ci, 3, 1, 1, generator=torch.Generator().manual_seed(10)).requires_grad_(True)
    y = F.conv3d(xt.float(), w, None, padding=(1, 0, 0))
    dyt = h16(*y.shape, seed=11)
    y.backward(dyt.float())
    Lt = AD.Dense(P, "t", "tb", kind="conv_t3")
    to_rows = lambda t: t[..., 0].permute(0, 2, 3, 1).contiguous().view(Bc * Fr * S, -1)
    Lt.accumulate(to_rows(xt).to(dev), to_rows(dyt).to(dev), (Bc, Fr, S))
    assert rel(P.gradient("t"), w.grad) < 3e-4
    assert rel(P.gradient("tb"), dyt.float().sum((0, 2, 3, 4))) < 3e-4


# ------------------------------------------------------------------------------------------------- norms
@pytest.mark.parametrize("C0,C1,rows_per_sample,n_samples,silu", [(64, 0, 50, 3, True), (320, 0, 144, 2, True), (64, 32, 37, 2, True), (640, 640, 16, 1, False),
                                                                  (320, 0, 4 * 36, 1, True)])
def test_groupnorm_backward_against_autograd(dev, AD, C0, C1, rows_per_sample, n_samples, silu):
    Ct = C0 + C1
    rows = rows_per_sample * n_samples
    x = h16(rows, Ct, seed=12, scale=1.5) + 0.3
    gm = (1 + 0.2 * torch.randn(Ct, generator=torch.Generator().manual_seed(13))).half()
    bt = (0.2 * torch.randn(Ct, generator=torch.Generator().manual_seed(14))).half()
    dy = h16(rows, Ct, seed=15)
    xr, gr, br = x.float().requires_grad_(True), gm.float().requires_grad_(True), bt.float().requires_grad_(True)
    y = F.group_norm(xr.view(n_samples, rows_per_sample, Ct).permute(0, 2, 1), 32, gr, br, 1e-5)
    y = F.silu(y) if silu else y
    y.backward(dy.float().view(n_samples, rows_per_sample, Ct).permute(0, 2, 1))
    P = AD.ParamStore({"n.weight": gm.float(), "n.bias": bt.float()}, dev)
    A = AD.Affine(P, "n")
    tape = AD.Tape()
    x0 = AD.Var(x[:, :C0].contiguous().to(dev))
    x1 = AD.Var(x[:, C0:].contiguous().to(dev)) if C1 else None
    out = AD.groupnorm(tape, x0, A, rows_per_sample=rows_per_sample, n_samples=n_samples, eps=1e-5, silu=silu, x1=x1)
    assert rel(out.v, y.detach().permute(0, 2, 1).reshape(rows, Ct)) < 1e-3
    out.g = dy.to(dev)
    tape.backward()
    got = x0.g if x1 is None else torch.cat([x0.g, x1.g], 1)
    assert rel(got, xr.grad) < 1e-3
    assert rel(P.gradient("n.weight"), gr.grad) < 5e-4 and rel(P.gradient("n.bias"), br.grad) < 5e-4


@pytest.mark.parametrize("M,Cc", [(100, 64), (257, 320), (33, 1280)])
def test_layernorm_backward_against_autograd(dev, AD, M, Cc):
    x, dy = h16(M, Cc, seed=16, scale=2.0) + 0.5, h16(M, Cc, seed=17)
    gm = (1 + 0.2 * torch.randn(Cc, generator=torch.Generator().manual_seed(18))).half()
    bt = (0.2 * torch.randn(Cc, generator=torch.Generator().manual_seed(19))).half()
    xr, gr, br = x.float().requires_grad_(True), gm.float().requires_grad_(True), bt.float().requires_grad_(True)
    F.layer_norm(xr, (Cc,), gr, br, 1e-5).backward(dy.float())
    P = AD.ParamStore({"n.weight": gm.float(), "n.bias": bt.float()}, dev)
    tape = AD.Tape()
    xv = AD.Var(x.to(dev))
    out = AD.layernorm(tape, xv, AD.Affine(P, "n"))
    out.g = dy.to(dev)
    tape.backward()
    assert rel(xv.g, xr.grad) < 1e-3
    assert rel(P.gradient("n.weight"), gr.grad) < 5e-4 and rel(P.gradient("n.bias"), br.grad) < 5e-4


# ------------------------------------------------------------------------------------------------- element-wise / reductions
def test_elementwise_backward_kernels(dev, AD):
    from posetraj_amd import hip, ops
    L, st = hip.lib(), ops._stream()
    M, I = 77, 64
    h, dy = h16(M, 2 * I, seed=20, scale=2.0), h16(M, I, seed=21)
    hr = h.float().requires_grad_(True)
    val, gate = hr.chunk(2, dim=-1)
    y = val * F.gelu(gate)
    y.backward(dy.float())
    tape = AD.Tape()
    hv = AD.Var(h.to(dev))
    out = AD.geglu(tape, hv)
    assert rel(out.v, y.detach()) < 6e-4
    out.g = dy.to(dev)
    tape.backward()
    assert rel(hv.g, hr.grad) < 6e-4
    # silu
    x = h16(1000, seed=22, scale=3.0)
    xr = x.float().requires_grad_(True)
    F.silu(xr).backward(dy.float().reshape(-1)[:1000])
    tape = AD.Tape()
    xv = AD.Var(x.to(dev))
    o = AD.silu(tape, xv)
    o.g = dy.reshape(-1)[:1000].contiguous().to(dev)
    tape.backward()
    assert rel(xv.g, xr.grad) < 6e-4
    # blend + its weight's gradient, add_rowvec + the row vector's gradient
    a, b, g = h16(60, 64, seed=23), h16(60, 64, seed=24), h16(60, 64, seed=25)
    P = AD.ParamStore({"m": torch.tensor([0.3])}, dev)
    mr, ar, br_ = torch.tensor([0.3], requires_grad=True), a.float().requires_grad_(True), b.float().requires_grad_(True)
    al = torch.sigmoid(mr)
    (al * ar + (1 - al) * br_).backward(g.float())
    tape = AD.Tape()
    av, bv = AD.Var(a.to(dev)), AD.Var(b.to(dev))
    o = AD.blend(tape, av, bv, AD.Mix(P, "m"))
    o.g = g.to(dev)
    tape.backward()
    assert rel(av.g, ar.grad) < 6e-4 and rel(bv.g, br_.grad) < 6e-4 and rel(P.gradient("m"), mr.grad) < 1e-3
    vec = h16(5, 64, seed=26)
    vr = vec.float().requires_grad_(True)
    (a.float() + vr.repeat_interleave(12, 0)).backward(g.float())
    tape = AD.Tape()
    vv = AD.Var(vec.to(dev))
    o = AD.add_rowvec(tape, AD.Var(a.to(dev)), vv, 12)
    assert rel(o.v, a.float() + vec.float().repeat_interleave(12, 0)) < 5e-4
    o.g = g.to(dev)
    tape.backward()
    assert rel(vv.g, vr.grad) < 6e-4
    # softmax rows and its backward
    R, n = 37, 75
    S = torch.randn(R, n, generator=torch.Generator().manual_seed(27)) * 3
    dP = torch.randn(R, n, generator=torch.Generator().manual_seed(28))
    Sr = S.clone().requires_grad_(True)
    Pw = torch.softmax(Sr, -1)
    Pg = torch.empty((R, n), dtype=torch.float16, device=dev)
    Sd, dPd = S.to(dev), dP.to(dev)
    hip.check(L.pt_softmax_rows(Sd.data_ptr(), R, n, n, Pg.data_ptr(), n, st))
    assert rel(Pg, Pw.detach()) < 5e-4
    Pw.backward(dP)
    dS = torch.empty((R, n), dtype=torch.float16, device=dev)
    hip.check(L.pt_softmax_bwd_rows(Pg.data_ptr(), n, dPd.data_ptr(), n, R, n, dS.data_ptr(), n, st))
    assert rel(dS, Sr.grad) < 1.5e-3
    # 2x2 block sums, zero interleave
    du = h16(2, 6, 8, 16, seed=29)
    dx = torch.empty((2, 3, 4, 16), dtype=torch.float16, device=dev)
    dud = du.to(dev)
    hip.check(L.pt_sumpool2x_f16(dud.data_ptr(), 2, 3, 4, 16, dx.data_ptr(), st))
    assert rel(dx, du.float().view(2, 3, 2, 4, 2, 16).sum((2, 4))) < 5e-4
    dyz = h16(2, 3, 4, 8, seed=30)
    z = torch.empty((2, 5, 8, 8), dtype=torch.float16, device=dev)
    dyzd = dyz.to(dev)
    hip.check(L.pt_zero_insert2x_f16(dyzd.data_ptr(), 2, 3, 4, 5, 8, 8, z.data_ptr(), st))
    want = torch.zeros(2, 5, 8, 8)
    want[:, ::2, ::2] = dyz.float()
    assert torch.equal(z.float().cpu(), want)


@pytest.fixture(scope="module")
def blend_case():
    """The AlphaBlender shapes of ``test_elementwise_backward_kernels`` (3840 elements: 15 blocks of the weight-gradient reduction,
    mix 0.3) and the gradients of ``alpha a + (1 - alpha) b`` under autograd."""
    a, b, g = h16(60, 64, seed=23), h16(60, 64, seed=24), h16(60, 64, seed=25)
    mr, ar, br_ = torch.tensor([0.3], requires_grad=True), a.float().requires_grad_(True), b.float().requires_grad_(True)
    al = torch.sigmoid(mr)
    y = al * ar + (1 - al) * br_
    y.backward(g.float())
    return a, b, g, y.detach(), ar.grad, br_.grad, mr.grad


def _forbidden(*args, **kw):
    raise AssertionError("must not be called in this mode")


def test_blend_with_the_weight_in_device_memory(dev, AD, blend_case, monkeypatch):
    """``device_scalars`` (what ``use_graph=True`` runs): pt_lerp_f16_dev / pt_dot_diff_dev / pt_scale_f16_dev read sigmoid(mix) from
    ``ParamStore.alphas``; the host never fetches the scalar.  Tolerances: those of the host mode above."""
    a, b, g, y, da, db, dm = blend_case
    P = AD.ParamStore({"m": torch.tensor([0.3])}, dev)
    P.device_scalars = True
    P.refresh_alphas()
    monkeypatch.setattr(P, "scalar", _forbidden)
    tape = AD.Tape()
    av, bv = AD.Var(a.to(dev)), AD.Var(b.to(dev))
    o = AD.blend(tape, av, bv, AD.Mix(P, "m"))
    o.g = g.to(dev)
    tape.backward()
    got = rel(o.v, y), rel(av.g, da), rel(bv.g, db), rel(P.gradient("m"), dm)
    print("blend, device scalars: forward %.2e, da %.2e, db %.2e, dmix %.2e" % got)
    assert got[0] < 6e-4 and got[1] < 6e-4 and got[2] < 6e-4 and got[3] < 1e-3
    assert o.g is None


def test_lerp_host_and_device_alpha_agree_bit_for_bit(dev):
    """pt_lerp_f16 (alpha a launch argument) and pt_lerp_f16_dev (the same fp32 value in device memory) are two instances of one
    kernel body: identical outputs.  n: one 8-element chunk; 257 chunks (a second block with one live lane); the AlphaBlender's."""
    from posetraj_amd import hip, ops
    L, st = hip.lib(), ops._stream()
    for n in (8, 8 * 257, 8 * 3840):
        a, b = h16(n, seed=31).to(dev), h16(n, seed=32).to(dev)
        for alpha in (0.0, 0.3, 1.0):
            alpha_dev = torch.tensor([alpha], dtype=torch.float32, device=dev)
            host, devm = (torch.full((n,), float("nan"), dtype=torch.float16, device=dev) for _ in range(2))
            hip.check(L.pt_lerp_f16(a.data_ptr(), b.data_ptr(), alpha, n, host.data_ptr(), st))
            hip.check(L.pt_lerp_f16_dev(a.data_ptr(), b.data_ptr(), alpha_dev.data_ptr(), n, devm.data_ptr(), st))
            assert torch.equal(host.view(torch.int16), devm.view(torch.int16)), (n, alpha)
            al = float(alpha_dev.item())
            assert rel(host, al * a.float() + (1.0 - al) * b.float()) < 5e-4, (n, alpha)


def test_blend_over_a_frozen_store(dev, AD, blend_case, monkeypatch):
    """The frozen U-Net's AlphaBlender: data gradients only - no weight-gradient launch, ``gradient`` never asked for."""
    from posetraj_amd import hip
    a, b, g, y, da, db, _ = blend_case
    P = AD.FrozenParams({"m": torch.tensor([0.3])}, dev)
    monkeypatch.setattr(P, "gradient", _forbidden)
    real, launched = hip.checked(), []

    class Recording:
        def __getattr__(self, name):
            launched.append(name)
            return getattr(real, name)

    monkeypatch.setattr(hip, "checked", lambda: Recording())
    tape = AD.Tape()
    av, bv = AD.Var(a.to(dev)), AD.Var(b.to(dev))
    o = AD.blend(tape, av, bv, AD.Mix(P, "m"))
    o.g = g.to(dev)
    tape.backward()
    got = rel(o.v, y), rel(av.g, da), rel(bv.g, db)
    print("blend, frozen store: forward %.2e, da %.2e, db %.2e; launches %s" % (got + (launched,)))
    assert got[0] < 6e-4 and got[1] < 6e-4 and got[2] < 6e-4
    assert "pt_lerp_f16" in launched and not any(n.startswith("pt_dot_diff") or n.endswith("_dev") for n in launched)


@pytest.mark.parametrize("shared", [False, True])
def test_rows_backward_and_add_rows(dev, AD, shared):
    """``rows``' backward - at once, and deferred then joined by ``add_rows`` - adds the gradient into rows ``r0:r1`` of ``x.g``: of a
    zero fill when there is none yet, else of a CLONE - the tensor that was there is also another variable's gradient and keeps its
    values.  Into zeros the sum is exact; onto a gradient it is one fp16 rounding of a sum of two fp16 numbers: 5e-4; the rows outside
    the slice are exact."""
    x, dy, g0 = h16(6 * 8, 16, seed=70).to(dev), h16(8, 16, seed=71).to(dev), h16(6 * 8, 16, seed=72).to(dev)
    r0, r1 = 16, 24
    want = g0.float() if shared else torch.zeros(48, 16, device=dev)
    want[r0:r1] += dy.float()
    kept = g0.clone()
    for defer in (None, []):
        tape = AD.Tape()
        xv, other = AD.Var(x), AD.Var(x)
        if shared:
            xv.g = other.g = g0
        o = AD.rows(tape, xv, r0, r1, defer=defer)
        assert o.v.data_ptr() == x[r0:r1].data_ptr()
        o.g = dy
        tape.backward()
        if defer is not None:
            assert xv.g is (g0 if shared else None) and len(defer) == 1 and defer[0][:3] == (xv, r0, r1) and defer[0][3] is dy
            AD.add_rows(*defer[0])
        assert xv.g is not g0 and xv.g.shape == x.shape
        assert rel(xv.g[r0:r1], want[r0:r1]) < 5e-4 if shared else torch.equal(xv.g[r0:r1], dy)
        assert torch.equal(xv.g[:r0].float(), want[:r0]) and torch.equal(xv.g[r1:].float(), want[r1:])
        if shared:
            assert other.g is g0 and torch.equal(g0, kept)      # never modified in place
    quiet = AD.Var(x, need=False)
    AD.add_rows(quiet, r0, r1, dy)
    assert quiet.g is None


def test_edm_loss_backward_adamw_and_norm(dev):
    from posetraj_amd import hip, ops
    L, st = hip.lib(), ops._stream()
    Bc, Fr, HW = 1, 3, 20
    g = torch.Generator().manual_seed(31)
    pred = torch.randn(Bc, Fr, HW, 4, generator=g).half()
    noisy, target = torch.randn(Bc, Fr, 4, HW, generator=g), torch.randn(Bc, Fr, 4, HW, generator=g)
    sig = torch.tensor([1.7])
    pr = pred.float().requires_grad_(True)
    c_out, c_skip, w = -sig / (sig ** 2 + 1) ** 0.5, 1 / (sig ** 2 + 1), (1 + sig ** 2) / sig ** 2
    den = pr.permute(0, 1, 3, 2) * c_out + c_skip * noisy
    (w * (den - target) ** 2).reshape(Bc, -1).mean(1).mean().backward()
    out = torch.empty((Bc * Fr * HW, 8), dtype=torch.float16, device=dev)
    pd, nd, td, sd = pred.to(dev), noisy.to(dev), target.to(dev), sig.to(dev)
    hip.check(L.pt_edm_loss_bwd(pd.data_ptr(), 0, 4, nd.data_ptr(), td.data_ptr(), sd.data_ptr(), Bc, Fr, HW, 1024.0, out.data_ptr(), st))
    assert rel(out[:, :4].float() / 1024, pr.grad.reshape(-1, 4)) < 6e-4 and float(out[:, 4:].abs().max()) == 0.0
    # AdamW: three steps against torch.optim.AdamW, gradients scaled like a loss-scaled reverse pass
    n = 5000
    p0 = torch.randn(n, generator=g)
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([ref], lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8)
    p, m, v = p0.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    for step in range(1, 4):
        gr = torch.randn(n, generator=g) * 0.1
        ref.grad = gr.clone()
        opt.step()
        gs = (gr * 256).to(dev)
        hip.check(L.pt_adamw_f32(p.data_ptr(), gs.data_ptr(), m.data_ptr(), v.data_ptr(), n, 1e-3, 0.9, 0.999, 1e-8, 1e-2, step, 1 / 256.0, st))
        assert float((p.cpu() - ref.detach()).abs().max()) < 2e-6
    acc = torch.zeros(1, dtype=torch.float64, device=dev)
    hip.check(L.pt_sumsq_f32(gs.data_ptr(), n, acc.data_ptr(), st))
    assert abs(float(acc) / float((gs.double() ** 2).sum()) - 1) < 1e-9
    gs[17] = float("inf")
    acc.zero_()
    hip.check(L.pt_sumsq_f32(gs.data_ptr(), n, acc.data_ptr(), st))
    assert not math.isfinite(float(acc))


def test_pack_refresh_from_the_fp32_master_equals_a_fresh_pack(dev, AD):
    """After an optimizer step the layers rewrite their fp16 operands in place with pt_pack_weight_f32 (forward pack and the
    transposed, tap-flipped data-gradient pack): bit-identical to packing the updated master from scratch."""
    g = torch.Generator().manual_seed(50)
    sd = {"lin.weight": torch.randn(72, 40, generator=g), "lin.bias": torch.randn(72, generator=g),
          "conv.weight": torch.randn(48, 24, 3, 3, generator=g), "conv.bias": torch.randn(48, generator=g),
          "cin.weight": torch.randn(16, 3, 3, 3, generator=g), "cin.bias": torch.randn(16, generator=g),
          "one.weight": torch.randn(40, 72, 1, 1, generator=g), "one.bias": torch.randn(40, generator=g),
          "t3.weight": torch.randn(32, 16, 3, 1, 1, generator=g), "t3.bias": torch.randn(32, generator=g),
          "q.weight": torch.randn(16, 24, generator=g), "k.weight": torch.randn(16, 24, generator=g), "v.weight": torch.randn(16, 24, generator=g)}
    P = AD.ParamStore(sd, dev)
    layers = [AD.Dense(P, "lin.weight", "lin.bias"), AD.Dense(P, "conv.weight", "conv.bias", kind="conv", padding=1),
              AD.Dense(P, "cin.weight", "cin.bias", kind="conv", padding=1), AD.Dense(P, "one.weight", "one.bias"),
              AD.Dense(P, "conv.weight", "conv.bias", kind="conv", padding=1, stride=2), AD.Dense(P, "t3.weight", "t3.bias", kind="conv_t3"),
              AD.Dense(P, "q.weight", None, stack=("q.weight", "k.weight", "v.weight"))]
    first = [L.packs() for L in layers]
    ptrs = [(f.w.data_ptr(), t.w.data_ptr()) for f, t in first]
    P.flat.mul_(1.5).add_(0.25)                                   # "an optimizer step"
    P.version += 1
    for L, pp in zip(layers, ptrs):
        f, t = L.packs()
        assert (f.w.data_ptr(), t.w.data_ptr()) == pp             # refreshed in place
        fresh = AD.Dense(P, L.wname, L.bname, kind=L.kind, stride=L.stride, padding=L.padding, stack=L.stack)
        fresh.P = AD.FrozenParams({k: P.value(k).clone() for k in P.names}, dev)       # the torch packing path
        f2, t2 = fresh.packs()
        assert torch.equal(f.w, f2.w) and torch.equal(t.w, t2.w), L.wname
        assert (f.bias is None and f2.bias is None) or torch.equal(f.bias, f2.bias)
    gm = P.half_view("lin.bias")
    assert torch.equal(gm, P.value("lin.bias").half())


@pytest.mark.parametrize("M,K,N", [(1, 1280, 320), (14, 64, 256), (2, 16, 64), (16, 768, 1280)])
def test_few_row_linear_layers(dev, AD, M, K, N):
    from posetraj_amd.packing import pack_linear
    x, w, b, r = h16(M, K, seed=51), h16(N, K, seed=52, scale=K ** -0.5), h16(N, seed=53), h16(M, N, seed=54)
    pw = pack_linear(w.float(), b.float(), dev)
    xd, rd = x.to(dev), r.to(dev)
    assert AD._few_rows(xd, pw)
    want = x.float() @ w.float().t() + b.float()
    assert rel(AD.gemv(xd, pw), want) < 5e-4
    assert rel(AD.gemv(xd, pw, rd), want + r.float()) < 5e-4


# ------------------------------------------------------------------------------------------------- tape primitives: dense
def _conv_case(dev, AD, kind, N, H, W, Ci, Co, stride=1, pad=1, upsample=False, C1=0, res=False):
    g = torch.Generator().manual_seed(40)
    x = torch.randn(N, Ci + C1, H, W, generator=g).half()
    k = 1 if pad == 0 else 3
    w = (torch.randn(Co, Ci + C1, k, k, generator=g) / math.sqrt((Ci + C1) * k * k)).half().float()
    b = (torch.randn(Co, generator=g) * 0.1).half().float()
    xr = x.float().requires_grad_(True)
    xin = F.interpolate(xr, scale_factor=2.0, mode="nearest") if upsample else xr
    y = F.conv2d(xin, w, b, stride=stride, padding=pad)
    r = torch.randn(*y.shape, generator=g).half() if res else None
    rr = None if r is None else r.float().requires_grad_(True)
    y = y if r is None else y + rr
    dy = torch.randn(*y.shape, generator=g).half()
    y.backward(dy.float())
    P = AD.FrozenParams({"w": w, "b": b}, dev)
    L = AD.Dense(P, "w", "b", kind="conv", stride=stride, padding=pad)
    cl = lambda t: t.permute(0, 2, 3, 1).contiguous().view(-1, t.shape[1])
    tape = AD.Tape()
    x0 = AD.Var(cl(x[:, :Ci]).to(dev))
    x1 = AD.Var(cl(x[:, Ci:]).to(dev)) if C1 else None
    rv = None if r is None else AD.Var(cl(r).to(dev))
    out = AD.dense(tape, x0, L, geom=(N, H, W), res=rv, x1=x1, upsample2x=upsample)
    assert rel(out.v, cl(y.detach())) < 6e-4
    out.g = cl(dy).to(dev)
    tape.backward()
    got = x0.g if x1 is None else torch.cat([x0.g, x1.g], 1)
    assert rel(got, cl(xr.grad)) < 8e-4
    if rv is not None:
        assert rel(rv.g, cl(rr.grad)) < 1e-6


def test_dense_data_gradients(dev, AD):
    """3 x 3 stride 1 (+ residual), stride 2 (even and odd extents), nearest-2x-upsample + conv, 1 x 1 over two concatenated
    sources (the up blocks' shortcut), 3 x 3 over... one source after a two-source norm."""
    _conv_case(dev, AD, "conv", 2, 9, 7, 32, 64, res=True)
    _conv_case(dev, AD, "conv", 2, 8, 12, 32, 32, stride=2)
    _conv_case(dev, AD, "conv", 1, 9, 7, 16, 32, stride=2)
    _conv_case(dev, AD, "conv", 2, 5, 6, 32, 32, upsample=True)
    _conv_case(dev, AD, "conv", 2, 6, 5, 64, 32, pad=0, C1=32)


def test_dense_linear_and_temporal_data_gradients(dev, AD):
    g = torch.Generator().manual_seed(41)
    M, K, N = 300, 64, 160
    x, dy = torch.randn(M, K, generator=g).half(), torch.randn(M, N, generator=g).half()
    w = (torch.randn(N, K, generator=g) / 8).half().float()
    L = AD.Dense(AD.FrozenParams({"w": w}, dev), "w")
    tape = AD.Tape()
    xv = AD.Var(x.to(dev))
    o = AD.dense(tape, xv, L)
    o.g = dy.to(dev)
    tape.backward()
    assert rel(o.v, x.float() @ w.t()) < 6e-4 and rel(xv.g, dy.float() @ w) < 8e-4
    Bc, Fr, S, Ci, Co = 2, 5, 12, 32, 64
    xt = torch.randn(Bc, Ci, Fr, S, 1, generator=g).half()
    wt = (torch.randn(Co, Ci, 3, 1, 1, generator=g) / 10).half().float()
    xr = xt.float().requires_grad_(True)
    y = F.conv3d(xr, wt, None, padding=(1, 0, 0))
    dyt = torch.randn(*y.shape, generator=g).half()
    y.backward(dyt.float())
    to_rows = lambda t: t[..., 0].permute(0, 2, 3, 1).contiguous().view(Bc * Fr * S, -1)
    Lt = AD.Dense(AD.FrozenParams({"t": wt}, dev), "t", kind="conv_t3")
    tape = AD.Tape()
    xv = AD.Var(to_rows(xt).to(dev))
    o = AD.dense(tape, xv, Lt, geom=(Bc, Fr, S))
    o.g = to_rows(dyt).to(dev)
    tape.backward()
    assert rel(o.v, to_rows(y.detach())) < 6e-4 and rel(xv.g, to_rows(xr.grad)) < 8e-4


# ------------------------------------------------------------------------------------------------- tape primitives: attention
@pytest.mark.parametrize("flash", [True, False])
@pytest.mark.parametrize("N,S,heads,hd", [(3, 64, 2, 64), (2, 180, 1, 64), (2, 50, 2, 128), (1, 1, 1, 64), (2, 333, 3, 64), (1, 720, 2, 128)])
def test_spatial_attention_backward_against_sdpa_autograd(dev, AD, monkeypatch, N, S, heads, hd, flash):
    """flash: pt_attn_fwd_lse_f16 + the two-pass flash backward pt_attn_bwd_f16 (what the trainer runs); else the recomputing
    path through pt_gemm_f16 and the softmax row kernels (kept for head sizes the flash kernels do not cover)."""
    monkeypatch.setattr(AD, "FLASH_BACKWARD", flash)
    Cc = heads * hd
    qkv = h16(N * S, 3 * Cc, seed=42)
    dy = h16(N * S, Cc, seed=43)
    xr = qkv.float().requires_grad_(True)
    q, k, v = (t.reshape(N, S, heads, hd).transpose(1, 2) for t in xr.view(N * S, 3, Cc).unbind(1))
    y = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(N * S, Cc)
    y.backward(dy.float())
    monkeypatch.setattr(AD, "ATTN_SCORE_BYTES", heads * S * S * 4 * 2)                        # two frames per chunk: the chunk loop runs
    tape = AD.Tape()
    xv = AD.Var(qkv.to(dev))
    o = AD.attn_spatial(tape, xv, N, S, heads, hd)
    assert rel(o.v, y.detach()) < 8e-4
    o.g = dy.to(dev)
    tape.backward()
    assert rel(xv.g, xr.grad) < 1.5e-3


@pytest.mark.parametrize("flash", [True, False])
@pytest.mark.parametrize("Bc,Fr,S,heads,hd", [(1, 14, 20, 2, 64), (2, 4, 9, 1, 64), (1, 1, 16, 2, 64), (1, 7, 6, 1, 128), (2, 16, 33, 3, 64), (1, 14, 2880, 5, 64),
                                              (1, 25, 12, 2, 64)])
def test_temporal_attention_backward_against_sdpa_autograd(dev, AD, monkeypatch, Bc, Fr, S, heads, hd, flash):
    """flash: pt_attn_temporal_bwd_f16 (one wave per position and head, F <= 16; one frame: the exact shortcut); else, and for
    longer clips (25 frames), the recomputing path through pt_gemm_f16."""
    monkeypatch.setattr(AD, "FLASH_BACKWARD", flash)
    Cc = heads * hd
    qkv = h16(Bc * Fr * S, 3 * Cc, seed=44)
    dy = h16(Bc * Fr * S, Cc, seed=45)
    xr = qkv.float().requires_grad_(True)
    x5 = xr.view(Bc, Fr, S, 3, heads, hd)
    q, k, v = (x5[:, :, :, i].permute(0, 2, 3, 1, 4) for i in range(3))                      # [B, S, heads, F, hd]
    y = F.scaled_dot_product_attention(q, k, v).permute(0, 3, 1, 2, 4).reshape(Bc * Fr * S, Cc)
    y.backward(dy.float())
    tape = AD.Tape()
    xv = AD.Var(qkv.to(dev))
    o = AD.attn_temporal(tape, xv, Bc, Fr, S, heads, hd)
    assert rel(o.v, y.detach()) < 8e-4
    o.g = dy.to(dev)
    tape.backward()
    assert rel(xv.g, xr.grad) < 1.5e-3


def test_pipelined_training_kernels_are_deterministic(dev, AD):
    """Race screen for the kernels that stage tiles through LDS under a prefetch (pt_gemm_f16 without split-K, both passes of
    pt_attn_bwd_f16, pt_attn_fwd_lse_f16): a too-early LDS overwrite shows as a run-to-run difference - five runs each over
    several tiles per workgroup must agree bit for bit."""
    from posetraj_amd import hip, ops
    L = hip.lib()
    for M, N, K in ((300, 200, 1000), (304, 200, 1000)):                     # the general loader (M % 8 != 0) and the branch-free one
        a, b = h16(K, M, seed=60).to(dev), h16(K, N, seed=61).to(dev)         # both operands transposed-read
        outs = []
        for _ in range(5):
            c = torch.empty((M, N), dtype=torch.float16, device=dev)
            AD.gemm((a, 0), (b, 0), (c, 0), M, N, K, (1, M), (N, 1), (N, 1))
            outs.append(c)
        assert all(torch.equal(outs[0], o) for o in outs[1:])
        assert rel(outs[0], a.float().T @ b.float()) < 2e-3
    Nf, S, heads, hd = 3, 333, 2, 64
    Cc = heads * hd
    qkv, dy = h16(Nf * S, 3 * Cc, seed=62).to(dev), h16(Nf * S, Cc, seed=63).to(dev)
    res = []
    for _ in range(5):
        tape = AD.Tape()
        xv = AD.Var(qkv)
        o = AD.attn_spatial(tape, xv, Nf, S, heads, hd)
        o.g = dy
        tape.backward()
        res.append((o.v, xv.g))
    assert all(torch.equal(res[0][0], r[0]) and torch.equal(res[0][1], r[1]) for r in res[1:])


# ------------------------------------------------------------------------------------------------- the whole step
def _nets(dev):
    from oracle import init as OI, nets as ON
    from posetraj_amd import UNetSpatioTemporalConditionControlNetModel
    from tests.golden.make_golden import TRAIN_CE, TRAIN_CFG
    with contextlib.redirect_stdout(io.StringIO()):
        cn_o = OI.seeded_init_(ON.ControlNetSDVModel(**TRAIN_CFG, conditioning_embedding_out_channels=TRAIN_CE), seed=81)
        un_o = OI.seeded_init_(ON.UNetSpatioTemporalConditionControlNetModel(**TRAIN_CFG), seed=82)
    with torch.no_grad():
        for m in (cn_o, un_o):
            for prm in m.parameters():
                prm.copy_(prm.half().float())
    un = UNetSpatioTemporalConditionControlNetModel(**TRAIN_CFG).load_state_dict(un_o.state_dict(), dev, keep_source=True)
    cfg = dict(TRAIN_CFG, conditioning_embedding_out_channels=TRAIN_CE, down_block_types=un.config.down_block_types)
    return cn_o, un_o, un, cfg


def _compare_grads(got: dict, want: dict, label: str):
    names = sorted(want)
    gw = torch.cat([want[k].reshape(-1).double() for k in names])
    gg = torch.cat([got[k].reshape(-1).double().cpu() for k in names])
    total = float((gg - gw).norm() / gw.norm())
    big = float(gw.norm()) / math.sqrt(len(names))
    worst, worst_name = 0.0, ""
    for k in names:
        nw = float(want[k].norm())
        if nw < 0.05 * big:
            continue
        r = rel(got[k], want[k])
        if r > worst:
            worst, worst_name = r, k
    dead = [k for k in names if float(want[k].abs().max()) == 0.0]
    assert all(float(got[k].abs().max()) == 0.0 for k in dead), "parameters with exactly zero gradient under autograd must stay zero"
    print(f"{label}: all {len(names)} parameter gradients rel-L2 {total:.2e}; worst sizeable tensor {worst:.2e} ({worst_name}); {len(dead)} exactly-zero tensors")
    return total, worst


def test_training_step_gradients_against_the_reference_run(dev, golden):
    """ControlNetTrainer.loss_and_grads vs the gradients the reference script's own statements produced (fp32,
    tests/golden/train_grads.npz: `accelerator.backward(loss)` captured inside `optimizer.step()`), then one AdamW step vs the
    parameters after the script's `optimizer.step()`."""
    from oracle import train as OT
    from posetraj_amd.training import ControlNetTrainer
    from tests.golden.make_golden import GRAD_FULL, GRAD_SUBSAMPLE
    g = golden("train_grads")
    cn_o, un_o, un, cfg = _nets(dev)
    lr, b1, b2, wd, eps = (float(v) for v in g["adam"])
    tr = ControlNetTrainer(cfg, cn_o.state_dict(), un, learning_rate=lr, adam_beta1=b1, adam_beta2=b2, adam_weight_decay=wd, adam_epsilon=eps,
                           conditioning_dropout_prob=0.1, loss_scale=4096.0)
    t = lambda n: torch.from_numpy(g[n])
    r = tr.loss_and_grads(t("latents"), t("emb"), torch.tensor([127.0]), t("traj"), noise=t("noise"), sigmas=t("sigmas"), random_p=t("random_p"),
                          ran_idx=int(g["ran_idx"]))
    rl, rs = abs(r["loss"] / float(g["loss"]) - 1), abs(r["loss_spatial"] / float(g["loss_spatial"]) - 1)
    print(f"loss {r['loss']:.6f} vs {float(g['loss']):.6f} ({rl:.1e}); spatial ({rs:.1e})")
    assert rl < 1e-3 and rs < 1e-3
    grads = tr.gradients()
    names = [str(n) for n in g["names"]]
    sample = lambda x: (x.reshape(-1) if x.numel() <= GRAD_FULL else x.reshape(-1)[::GRAD_SUBSAMPLE]).float().cpu().numpy()
    got = np.concatenate([sample(grads[k]) for k in names])
    rg = float(np.linalg.norm(got - g["grad_samples"]) / np.linalg.norm(g["grad_samples"]))
    gn = np.array([float(grads[k].norm()) for k in names])
    print(f"stored gradient values rel-L2 {rg:.2e}; per-parameter norms: max relative deviation among the sizeable ones "
          f"{np.abs(gn / np.maximum(g['grad_norm'], 1e-30) - 1)[g['grad_norm'] > 0.05 * g['grad_norm'].max()].max():.2e}")
    assert rg < 1.1e-3                                         # measured 8.65e-4 (r05): the stated 1.25 x measured
    # full gradients against fp32 autograd over the oracle (itself pinned to the same fixture on the CPU)
    ro = OT.training_step_grads(cn_o, un_o, t("latents"), t("noise"), t("sigmas"), t("emb"), torch.tensor([127.0]), t("traj"), 0.18215,
                                random_p=t("random_p"), conditioning_dropout_prob=0.1, ran_idx=int(g["ran_idx"]))
    total, worst = _compare_grads(grads, ro["grads"], "training step (4 frames, 8 x 8 latent)")
    assert total < 1.2e-3 and worst < 3.0e-3                   # measured 9.3 - 9.5e-4 / 2.3 - 2.4e-3 (r04, r05) x 1.25
    assert math.isfinite(tr.grad_norm())
    assert tr.optimizer_step() is True and tr.optimizer_steps == 1
    after = tr.state_dict()
    got_after = np.concatenate([sample(after[k]) for k in names])
    # AdamW's first step moves every parameter by lr * g / (|g| + eps) ~ +-lr: a sign flip of a near-zero gradient costs 2 lr
    d = np.abs(got_after - g["after_samples"])
    print(f"parameters after optimizer.step(): max |diff| {d.max():.2e} (lr {lr:.0e}); {float((d > 0.1 * lr).mean()) * 100:.2f} % differ by more than lr / 10")
    assert d.max() <= 2.0 * lr * 1.01 and float((d > 0.1 * lr).mean()) < 0.02
    assert float(tr.params.grad.abs().max()) == 0.0                                            # optimizer.zero_grad()


def test_camera_twin_training_step_against_oracle_autograd(dev):
    """The camera ControlNet's step (scripts/train_svd_traj_VIPSeg_14_cam_concat.py:1393,1409: `camera_cond=cam_parameter`, no
    spatial loss): cc_projection over [features | R|T] trains with everything else; gradients vs fp32 autograd over the oracle."""
    from oracle import init as OI, nets as ON, train as OT
    from posetraj_amd import UNetSpatioTemporalConditionControlNetModel
    from posetraj_amd.training import ControlNetTrainer
    from tests.golden.make_golden import TRAIN_CE, TRAIN_CFG
    with contextlib.redirect_stdout(io.StringIO()):
        cn_o = OI.seeded_init_(ON.ControlNetSDVModel(**TRAIN_CFG, conditioning_embedding_out_channels=TRAIN_CE, camera=True), seed=91)
        un_o = OI.seeded_init_(ON.UNetSpatioTemporalConditionControlNetModel(**TRAIN_CFG), seed=92)
    with torch.no_grad():
        for m in (cn_o, un_o):
            for prm in m.parameters():
                prm.copy_(prm.half().float())
    un = UNetSpatioTemporalConditionControlNetModel(**TRAIN_CFG).load_state_dict(un_o.state_dict(), dev, keep_source=True)
    cfg = dict(TRAIN_CFG, conditioning_embedding_out_channels=TRAIN_CE, down_block_types=un.config.down_block_types, camera=True)
    tr = ControlNetTrainer(cfg, cn_o.state_dict(), un, conditioning_dropout_prob=None, loss_scale=4096.0)
    g = torch.Generator().manual_seed(93)
    Fr, h, w = 4, 8, 8
    lat = (torch.randn(1, Fr, 4, h, w, generator=g) * 0.18215 * 5).half().float()
    emb = torch.randn(1, 1, 16, generator=g).half().float()
    traj = (torch.rand(1, Fr, 3, h * 8, w * 8, generator=g) * 2 - 1).half().float()
    cam = (torch.randn(1, Fr, 12, generator=g) * 0.5).half().float()
    noise, sig = torch.randn(lat.shape, generator=g), torch.tensor([0.9])
    r = tr.loss_and_grads(lat, emb, torch.tensor([127.0]), traj, noise=noise, sigmas=sig, use_spatial=False, camera_cond=cam)
    ro = OT.training_step_grads(cn_o, un_o, lat, noise, sig, emb, torch.tensor([127.0]), traj, 0.18215, use_spatial=False, camera_cond=cam)
    assert r["loss_spatial"] is None and abs(r["loss"] / float(ro["loss"]) - 1) < 5e-4
    grads = tr.gradients()
    total, worst = _compare_grads(grads, ro["grads"], "camera twin (4 frames, 8 x 8 latent, no spatial loss)")
    assert total < 1.2e-3 and worst < 3.0e-3                   # measured 9.3 - 9.5e-4 / 2.3 - 2.4e-3 (r04, r05) x 1.25
    k = "controlnet_cond_embedding.cc_projection.weight"
    assert float(ro["grads"][k].norm()) > 0 and rel(grads[k], ro["grads"][k]) < 1e-2 and rel(grads[k.replace("weight", "bias")], ro["grads"][k.replace("weight", "bias")]) < 1e-2
    assert tr.optimizer_step() is True
    f, t = tr.controlnet.cc.packs()                                                           # refreshed in place: padding columns stay zero
    assert float(f.w[:, cn_o.controlnet_cond_embedding.cc_projection.weight.shape[1]:].abs().max()) == 0.0
    with pytest.raises(ValueError):
        ControlNetTrainer(dict(cfg, camera=False), {k: v for k, v in cn_o.state_dict().items() if "cc_projection" not in k}, un).loss_and_grads(
            lat, emb, torch.tensor([127.0]), traj, camera_cond=cam)


@pytest.mark.parametrize("Fr,h,w", [(2, 16, 16), (14, 8, 8)])
def test_training_step_gradients_at_full_width(dev, Fr, h, w):
    """The same comparison at the FULL model widths (U-Net 1.52 B frozen, ControlNet 0.68 B trainable, head_dim 64 everywhere;
    2 frames at a 16 x 16 latent, and the training clip's own 14 frames at 8 x 8 - the composed step with the one-wave temporal
    attention backward at F = 14, VERDICT r04 #2b): ControlNetTrainer vs fp32 autograd over the oracle on the host (~20 GB there)."""
    from oracle import train as OT
    from posetraj_amd import UNetSpatioTemporalConditionControlNetModel
    from posetraj_amd.training import ControlNetTrainer
    from tests import parity as P
    cn_o, un_o = P.build_oracle_nets(7, cfg=P.SVD_CFG, ce=P.SVD_CE)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():                                      # zero-convs that have left zero: every gradient is live
        for k, p in cn_o.named_parameters():
            if k.startswith(("controlnet_down_blocks", "controlnet_mid_block", "controlnet_cond_embedding.conv_out")):
                p.copy_((torch.randn(p.shape, generator=g) * 0.02).half().float())
    un = UNetSpatioTemporalConditionControlNetModel(**P.SVD_CFG).load_state_dict(un_o.state_dict(), dev, keep_source=True)
    cfg = dict(P.SVD_CFG, conditioning_embedding_out_channels=P.SVD_CE, down_block_types=un.config.down_block_types)
    tr = ControlNetTrainer(cfg, cn_o.state_dict(), un, conditioning_dropout_prob=0.1, loss_scale=4096.0)
    lat = (torch.randn(1, Fr, 4, h, w, generator=g) * 0.18215 * 5).half().float()
    emb = torch.randn(1, 1, P.SVD_CFG["cross_attention_dim"], generator=g).half().float()
    traj = (torch.rand(1, Fr, 3, h * 8, w * 8, generator=g) * 2 - 1).half().float()
    noise = torch.randn(lat.shape, generator=g)
    sig, rp = torch.tensor([1.3]), torch.tensor([0.7])
    ri = Fr // 2 + 1 if Fr > 2 else 1
    r = tr.loss_and_grads(lat, emb, torch.tensor([127.0]), traj, noise=noise, sigmas=sig, random_p=rp, ran_idx=ri)
    ro = OT.training_step_grads(cn_o, un_o, lat, noise, sig, emb, torch.tensor([127.0]), traj, 0.18215, random_p=rp, conditioning_dropout_prob=0.1, ran_idx=ri)
    print(f"full-width training step ({Fr} frames, {h} x {w}): loss {r['loss']:.6f} vs {float(ro['loss']):.6f} ({abs(r['loss'] / float(ro['loss']) - 1):.1e})")
    assert abs(r["loss"] / float(ro["loss"]) - 1) < 5e-4
    total, worst = _compare_grads(tr.gradients(), ro["grads"], f"full-width training step ({Fr} frames, {h} x {w} latent)")
    # measured (2 frames, 16 x 16) 0.96 - 1.06e-3 / 2.5 - 2.6e-3 on two boxes; (14 frames, 8 x 8) 7.2e-4 / 1.7e-3: 1.25 x the largest
    assert total < 1.33e-3 and worst < 3.25e-3


def test_training_loop_reduces_the_loss_and_handles_overflow(dev, golden):
    """A few optimizer steps on ONE fixed batch (same draws) must lower its loss; gradient accumulation over two identical
    micro-batches gives the single-batch gradient; an overflowing loss scale skips the step and halves the scale."""
    from posetraj_amd.training import ControlNetTrainer
    g = golden("train_grads")
    cn_o, un_o, un, cfg = _nets(dev)
    t = lambda n: torch.from_numpy(g[n])
    draws = dict(noise=t("noise"), sigmas=t("sigmas"), random_p=t("random_p"), ran_idx=int(g["ran_idx"]))
    batch = (t("latents"), t("emb"), torch.tensor([127.0]), t("traj"))
    tr = ControlNetTrainer(cfg, cn_o.state_dict(), un, learning_rate=2e-4, conditioning_dropout_prob=0.1, loss_scale=4096.0)
    losses = [tr.step(*batch, **draws)["loss"] for _ in range(6)]
    print("loss over 6 AdamW steps on one batch:", " ".join(f"{v:.5f}" for v in losses))
    assert losses[-1] < losses[0] * 0.97 and tr.optimizer_steps == 6
    # the same four steps with torch.optim.AdamW over fp32 autograd of the oracle: the loss TRAJECTORY must agree (after step 1
    # every parameter has moved by about lr, whichever way a negligible gradient's sign fell)
    from oracle import train as OT
    opt = torch.optim.AdamW(cn_o.parameters(), lr=2e-4, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8)
    ref = []
    for _ in range(4):
        ro = OT.training_step_grads(cn_o, un_o, batch[0], draws["noise"], draws["sigmas"], batch[1], batch[2], batch[3], 0.18215,
                                    random_p=draws["random_p"], conditioning_dropout_prob=0.1, ran_idx=draws["ran_idx"])
        ref.append(float(ro["loss"]))
        for k, prm in cn_o.named_parameters():
            prm.grad = ro["grads"][k]
        opt.step()
    print("the oracle's (torch.optim.AdamW, fp32):     ", " ".join(f"{v:.5f}" for v in ref))
    assert max(abs(a / b - 1) for a, b in zip(losses, ref)) < 4e-3            # measured 1.7e-3
    cn_o, un_o, un, cfg = _nets(dev)                           # fresh parameters for the remaining checks
    one = ControlNetTrainer(cfg, cn_o.state_dict(), un, conditioning_dropout_prob=0.1, loss_scale=4096.0)
    one.loss_and_grads(*batch, **draws)
    two = ControlNetTrainer(cfg, cn_o.state_dict(), un, conditioning_dropout_prob=0.1, loss_scale=4096.0, gradient_accumulation_steps=2)
    assert two.step(*batch, **draws)["stepped"] is None
    two.loss_and_grads(*batch, **draws)
    total, worst = _compare_grads(two.gradients(), {k: v.cpu() for k, v in one.gradients().items()}, "two accumulated half-weight micro-batches vs one batch")
    assert total < 1e-3 and worst < 5e-3
    hot = ControlNetTrainer(cfg, cn_o.state_dict(), un, conditioning_dropout_prob=0.1, loss_scale=2.0 ** 40)
    before = hot.state_dict()
    out = hot.step(*batch, **draws)
    assert out["stepped"] is False and hot.skipped_steps == 1 and hot.loss_scale == 2.0 ** 39
    after = hot.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)


def test_training_step_as_a_hipgraph_equals_the_eager_step(dev, golden):
    """``ControlNetTrainer(use_graph=True)`` (round 6): forward + backward captured once per (spatial frame index, loss scale, shapes) and
    replayed.  Step for step - losses, gradients before the optimizer - a graphed trainer must equal an eager one that reads the
    AlphaBlender weights from device memory too (``device_scalars=True``: the same launches, only their enqueueing differs) up to the
    order of fp32 atomics, over steps that change ``ran_idx`` (a second graph), the inputs (static buffers refilled) and - through an
    overflowing loss scale - the scale (graphs re-captured); and stay within rounding of the default trainer (host-side sigmoid)."""
    from posetraj_amd.training import ControlNetTrainer
    g = golden("train_grads")
    cn_o, un_o, un, cfg = _nets(dev)
    t = lambda n: torch.from_numpy(g[n])
    batch = (t("latents"), t("emb"), torch.tensor([127.0]), t("traj"))
    F = batch[0].shape[1]
    gen = torch.Generator().manual_seed(21)
    kw = dict(learning_rate=2e-4, conditioning_dropout_prob=0.1, loss_scale=4096.0)
    eager = ControlNetTrainer(cfg, cn_o.state_dict(), un, device_scalars=True, **kw)
    graph = ControlNetTrainer(cfg, cn_o.state_dict(), un, use_graph=True, **kw)
    host = ControlNetTrainer(cfg, cn_o.state_dict(), un, **kw)
    replays = 0

    def close(got, want):                                      # rel-L2 over all parameters together, and the worst sizeable tensor
        num = sum(float((got[k].double() - want[k].double()).pow(2).sum()) for k in want)
        den = sum(float(want[k].double().pow(2).sum()) for k in want)
        big = max(float(want[k].double().norm()) for k in want)
        worst = max(float((got[k].double() - want[k].double()).norm() / want[k].double().norm()) for k in want
                    if float(want[k].double().norm()) > 1e-3 * big)
        return (num / den) ** 0.5, worst

    for step in range(7):
        lat = batch[0] if step < 4 else (batch[0] * (1.0 + 0.1 * step)).half().float()          # new inputs through the static buffers
        draws = dict(noise=torch.randn(lat.shape, generator=gen), sigmas=torch.tensor([0.7 + 0.3 * step]), random_p=torch.tensor([0.9]),
                     ran_idx=(step * 3) % F if step != 3 else 0)                                  # step 3 re-uses the graph of step 0
        outs = []
        for tr in (eager, graph, host):
            o = tr.loss_and_grads(lat, *batch[1:], **draws)
            grads = {k: v.clone() for k, v in tr.gradients().items()}
            o["grad_norm"] = tr.grad_norm()
            o["stepped"] = tr.optimizer_step(o["grad_norm"])
            outs.append((o, grads))
        (oe, ge), (og, gg), (oh, gh) = outs
        replays += int(og["graph_replay"])
        assert og["graph_replay"] == (step >= 1) and not oe["graph_replay"]
        # the same launches in the same order on the same data: what differs between two runs is the order of the fp32 atomics inside the
        # weight-gradient and reduction kernels (two EAGER trainers differ by that much as well: measured below)
        # (after a few AdamW steps the two parameter sets have drifted apart by the sign of noise-level gradients: the bounds widen with the step;
        # a capture that dropped or mis-ordered a launch is off by O(1), not by 1e-3)
        assert abs(oe["loss"] / og["loss"] - 1) < 5e-4 * (1 + step), (step, oe["loss"], og["loss"])
        total, worst = close(gg, ge)
        assert total < 1.5e-3 * (1 + 0.5 * step) and worst < 2e-2, (step, total, worst)   # (step 0, both eager: 4.8e-4 / 1.3e-3)
        assert abs(oe["loss"] / oh["loss"] - 1) < 2e-3
        total, worst = close(ge, gh)
        assert total < 3e-3 * (1 + step), (step, total)                                          # (the two parameter sets drift apart by rounding, step by step)
    assert replays == 6 and len(graph._graphs) >= 3
    # an overflow: the step is skipped, the scale halves, and the next step's graphs are captured for the new scale
    for tr in (eager, graph):
        tr.loss_scale = 2.0 ** 40
    draws = dict(noise=torch.randn(batch[0].shape, generator=gen), sigmas=torch.tensor([1.1]), random_p=torch.tensor([0.9]), ran_idx=0)
    oe, og = eager.step(*batch, **draws), graph.step(*batch, **draws)
    assert oe["stepped"] is False and og["stepped"] is False and graph.loss_scale == eager.loss_scale == 2.0 ** 39
    for tr in (eager, graph):
        tr.loss_scale = 4096.0
    oe, og = eager.step(*batch, **draws), graph.step(*batch, **draws)
    assert oe["stepped"] and og["stepped"] and abs(oe["loss"] / og["loss"] - 1) < 2e-3
    with pytest.raises(ValueError):
        ControlNetTrainer(cfg, cn_o.state_dict(), un, use_graph=True, gradient_accumulation_steps=2)


def test_checkpoint_resume_and_lr_schedule(dev, golden, tmp_path):
    """``accelerator.save_state`` / ``load_state`` (reference ``:1464-1466``, ``:1241``): a trainer restored from a checkpoint
    continues like the one that wrote it (parameters, AdamW moments, step count, loss-scale state); the ``controlnet/`` folder
    is what ``ControlNetSDVModel.from_pretrained`` reads; a warm-up schedule drives AdamW's rate per taken step."""
    from posetraj_amd import ControlNetSDVModel, train_state
    from posetraj_amd.training import ControlNetTrainer
    g = golden("train_grads")
    cn_o, un_o, un, cfg = _nets(dev)
    t = lambda n: torch.from_numpy(g[n])
    draws = dict(noise=t("noise"), sigmas=t("sigmas"), random_p=t("random_p"), ran_idx=int(g["ran_idx"]))
    batch = (t("latents"), t("emb"), torch.tensor([127.0]), t("traj"))
    sd0 = {k: v.clone() for k, v in cn_o.state_dict().items()}
    lr = 2e-4
    sched = train_state.get_scheduler("constant_with_warmup", num_warmup_steps=2)
    a = ControlNetTrainer(cfg, sd0, un, learning_rate=lr, conditioning_dropout_prob=0.1, loss_scale=4096.0, growth_interval=2, lr_scheduler=sched)
    a.step(*batch, **draws)
    first = a.state_dict()
    assert a.last_lr == 0.0 and all(torch.equal(first[k].cpu(), sd0[k].float()) for k in sd0)       # lambda(0) = 0: AdamW moved nothing
    a.step(*batch, **draws)
    assert a.last_lr == lr / 2 and a.loss_scale == 8192.0 and a._clean == 0                          # grew after two clean steps
    ck = str(tmp_path / "checkpoint-2")
    a.save_state(ck)
    assert sorted(os.listdir(ck)) == ["controlnet", "optimizer.safetensors", "trainer_state.json"]
    a.step(*batch, **draws)
    assert a.last_lr == lr
    b = ControlNetTrainer(cfg, sd0, un, learning_rate=lr, conditioning_dropout_prob=0.1, loss_scale=4096.0, growth_interval=2, lr_scheduler=sched)
    stored = b.load_state(ck)
    assert stored["optimizer_steps"] == 2 and b.optimizer_steps == 2 and b.loss_scale == 8192.0 and b._clean == 0
    assert stored["hyperparameters"]["learning_rate"] == lr
    b.step(*batch, **draws)
    assert b.last_lr == lr and b.optimizer_steps == 3
    pa, pb = a.state_dict(), b.state_dict()
    # same parameters, moments and gradient (up to the order of the fp32 atomic sums): the third step must land in the same place
    worst = max(float((pa[k] - pb[k]).abs().max()) for k in pa)
    diff = math.sqrt(sum(float((pa[k] - pb[k]).double().pow(2).sum()) for k in pa))
    moved = math.sqrt(sum(float((pa[k].cpu() - first[k].cpu()).double().pow(2).sum()) for k in pa))
    print(f"resumed vs continuous run after the third step: |diff| {diff:.2e} of |moved| {moved:.2e}, max element diff {worst:.2e} (lr {lr:g})")
    assert diff < 1e-2 * moved and worst <= 2 * lr       # a near-zero gradient's sign may fall either way under fp32 atomics
    # the moments, over the whole store (a tensor whose gradient is rounding noise has noise for moments: no per-tensor bound)
    for buf_a, buf_b in ((a.optimizer.exp_avg, b.optimizer.exp_avg), (a.optimizer.exp_avg_sq, b.optimizer.exp_avg_sq)):
        assert float((buf_a - buf_b).double().norm() / buf_a.double().norm()) < 1e-3
    # the controlnet/ folder is a diffusers-format model of the parameters at save time
    m = ControlNetSDVModel.from_pretrained(ck, subfolder="controlnet", device=dev, keep_source=True)
    c = ControlNetTrainer(dict(m.config), m.state_dict(), un, learning_rate=lr)
    b2 = ControlNetTrainer(cfg, sd0, un, learning_rate=lr)
    b2.load_state(ck)
    pc, pb2 = c.state_dict(), b2.state_dict()
    assert set(pc) == set(pb2)
    assert max(float((pc[k] - pb2[k]).abs().max()) for k in pc) < 1e-3       # from_pretrained keeps an fp16 source copy
    a.save_pretrained(str(tmp_path / "final"))
    assert sorted(os.listdir(tmp_path / "final")) == ["config.json", "diffusion_pytorch_model.safetensors"]
    with pytest.raises(RuntimeError, match="accumulation cycle"):
        two = ControlNetTrainer(cfg, sd0, un, gradient_accumulation_steps=2, loss_scale=4096.0)
        two.step(*batch, **draws)
        two.save_state(str(tmp_path / "mid"))


# ------------------------------------------------------------------------------------------------- data parallel (two ranks, one GPU)
def _dp_worker(rank, world, port, q):
    import os
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        dev = torch.device("cuda:0")
        probe = torch.ones(4, device=dev) * (rank + 1)
        try:
            dist.all_reduce(probe)
        except Exception as e:                                  # this build's gloo cannot reduce device tensors
            q.put((rank, "unsupported", repr(e)[:200]))
            return
        from posetraj_amd.training import ControlNetTrainer
        g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_grads.npz"))
        cn_o, un_o, un, cfg = _nets(dev)
        sd = cn_o.state_dict()
        if rank == 1:                                           # rank 1 starts from other weights: the broadcast must overwrite them
            sd = {k: v + 0.01 for k, v in sd.items()}
        tr = ControlNetTrainer(cfg, sd, un, conditioning_dropout_prob=0.1, loss_scale=4096.0, bucket_mb=1)
        t = lambda n: torch.from_numpy(g[n])
        draws = dict(noise=t("noise") * (1.0 if rank == 0 else -1.0), sigmas=t("sigmas") * (1.0 + rank), random_p=t("random_p"), ran_idx=int(g["ran_idx"]))
        batch = (t("latents"), t("emb"), torch.tensor([127.0]), t("traj"))
        out = None
        for _ in range(2):                                      # step 1 learns the gradient-producing set, step 2 overlaps
            tr.params.zero_grad(); tr._micro, tr._accum_scale = 0, None
            out = tr.loss_and_grads(*batch, **draws)
        grads = {k: v.float().cpu().numpy() for k, v in tr.gradients().items()}            # numpy: pickled by value through the queue
        q.put((rank, "ok", dict(world=tr.world, early=tr.buckets.launched_early, nbuckets=len(tr.buckets.bounds),
                                 w0=float(tr.params.value("conv_in.weight").double().sum()), grads=grads, loss=out["loss"])))
    finally:
        dist.destroy_process_group()


def test_data_parallel_gradient_exchange_two_ranks_one_gpu(dev, golden):
    """ControlNetTrainer under torch.distributed with two ranks (both on this GPU, gloo moving the buckets): parameters follow
    rank 0, the synchronised gradients are the MEAN of the two ranks' own gradients (each rank draws a different sigma / noise),
    and from the second step on the buckets leave while the reverse pass is still running."""
    import socket
    import torch.multiprocessing as mp
    from posetraj_amd.training import ControlNetTrainer
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in range(2):
            r, status, payload = q.get(timeout=240)
            res[r] = (status, payload)
    finally:
        for p in procs:
            p.join(60)
            if p.is_alive():
                p.kill()
    if any(v[0] == "unsupported" for v in res.values()):
        pytest.skip(f"gloo cannot all-reduce device tensors here: {[v[1] for v in res.values() if v[0] == 'unsupported'][0]}")
    a, b = res[0][1], res[1][1]
    for d in (a, b):
        d["grads"] = {k: torch.from_numpy(v) for k, v in d["grads"].items()}
    assert a["world"] == b["world"] == 2 and a["w0"] == b["w0"]                               # rank 1 received rank 0's parameters
    assert a["early"] > 0 and a["early"] <= a["nbuckets"]
    assert all(torch.equal(a["grads"][k], b["grads"][k]) for k in a["grads"])                 # both ranks hold the same averaged gradients
    # reference: each rank's own gradient from a single-process trainer, averaged on the host
    g = golden("train_grads")
    t = lambda n: torch.from_numpy(g[n])
    cn_o, un_o, un, cfg = _nets(dev)
    own = []
    for rank in range(2):
        tr = ControlNetTrainer(cfg, cn_o.state_dict(), un, conditioning_dropout_prob=0.1, loss_scale=4096.0)
        tr.loss_and_grads(t("latents"), t("emb"), torch.tensor([127.0]), t("traj"), noise=t("noise") * (1.0 if rank == 0 else -1.0),
                          sigmas=t("sigmas") * (1.0 + rank), random_p=t("random_p"), ran_idx=int(g["ran_idx"]))
        own.append({k: v.float().cpu() for k, v in tr.gradients().items()})
    mean = {k: 0.5 * (own[0][k] + own[1][k]) for k in own[0]}
    total, worst = _compare_grads(a["grads"], mean, "two ranks' averaged gradients vs the host average of two single-rank runs")
    assert total < 1e-3 and worst < 5e-3
