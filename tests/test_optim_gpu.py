"""``optim.AdamW.step`` / ``optim.AdamW8bit.step`` on the device: each is ONE launch of the entry point, with the argument list, that
``ControlNetTrainer.optimizer_step`` and the 8-bit state's ``step`` issued before the optimizer had an object of its own.  Both sides
run the same kernel on the same values and the kernels have no atomics, so every comparison is ``torch.equal``."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BETAS, EPS, WD = (0.9, 0.999), 1e-8, 1e-2
STEPS = [(2e-4, 1 / 256.0, 1.0), (1.5e-4, 1 / 512.0, 2 / 11), (1e-4, 1 / 256.0, 3 / 12)]      # lr, inv_scale, 1 - EMA decay of steps 1, 2, 3


def _sd():
    """23 053 elements: two parameters with 8-bit state and a short last block (4200 = 16 x 256 + 104, 4752 = 18 x 256 + 144), one of
    whole blocks, two under 4096 elements (fp32 moments) and a scalar."""
    g = torch.Generator().manual_seed(0)
    return {"conv_in.weight": torch.randn(6, 5, 3, 3, generator=g), "conv_in.bias": torch.randn(6, generator=g),
            "odd.conv.weight": torch.randn(33, 16, 3, 3, generator=g), "big.conv.weight": torch.randn(32, 48, 3, 3, generator=g),
            "big.proj.weight": torch.randn(70, 60, generator=g), "mid.mix_factor": torch.tensor([0.25])}


@pytest.mark.parametrize("ema", ["none", "fused", "separate"])
@pytest.mark.parametrize("kind", ["adamw", "adamw8bit"])
def test_step_is_the_launch_the_trainer_used_to_issue(kind, ema):
    from posetraj_amd import hip, ops, optim
    from posetraj_amd.autodiff import ParamStore
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    sd = _sd()
    P, Q = ParamStore(sd, dev), ParamStore(sd, dev)             # P: through the optimizer object; Q: the entry points called by hand
    assert P.numel == Q.numel and 20000 < P.numel < 40000
    for S in (P, Q):
        S.flat16.zero_()                                        # (torch.empty: the 8-bit pass never writes the padding between parameters)
    hyper = dict(lr=STEPS[0][0], betas=BETAS, eps=EPS, weight_decay=WD)
    opt = (optim.AdamW8bit if kind == "adamw8bit" else optim.AdamW)(P, **hyper)
    assert opt.kind == kind
    A = optim.AdamW8bit(Q, **hyper) if kind == "adamw8bit" else None      # Q's 8-bit buffers, plan and table; its step() is not called
    m, v = (None, None) if A is not None else (torch.zeros_like(Q.flat), torch.zeros_like(Q.flat))
    if A is not None:
        kinds = {s[0]: s[4] for s in A.plan["segments"]}
        assert kinds == {"conv_in.weight": 0, "conv_in.bias": 0, "odd.conv.weight": 1, "big.conv.weight": 1, "big.proj.weight": 1, "mid.mix_factor": 0}
    shadow_p, shadow_q = (None, None) if ema == "none" else (P.flat.clone(), Q.flat.clone())
    L = hip.checked()
    g = torch.Generator().manual_seed(7)
    for i, (lr, inv_scale, omd) in enumerate(STEPS):
        step = i + 1
        grad = torch.randn(P.numel, generator=g) * 256.0
        P.grad.copy_(grad); Q.grad.copy_(grad)
        # -- the optimizer object
        if ema == "fused":
            opt.step(lr, step, inv_scale, shadow_p, omd)
        else:
            opt.step(lr, step, inv_scale)
            if ema == "separate":
                L.pt_ema_update_f32(shadow_p.data_ptr(), P.flat.data_ptr(), P.numel, omd, ops._stream())
        # -- by hand
        fused = ema == "fused"
        if A is not None:
            plan = A.plan
            L.pto_adamw8_f32(Q.flat.data_ptr(), Q.grad.data_ptr(), A._ptr(A.state1), A._ptr(A.state2), A._ptr(A.absmax1),
                             A._ptr(A.absmax2), A.qmap1.data_ptr(), A.qmap2.data_ptr(), A._ptr(A.exp_avg),
                             A._ptr(A.exp_avg_sq), A._segments, len(plan["segments"]), plan["n_work"], Q.numel, plan["n_blocks"],
                             plan["n_f32_alloc"], lr, BETAS[0], BETAS[1], EPS, WD, step, inv_scale, Q.flat16.data_ptr(), 1,
                             shadow_q.data_ptr() if fused else None, omd if fused else 0.0, ops._stream())
        else:
            adamw = (Q.flat.data_ptr(), Q.grad.data_ptr(), m.data_ptr(), v.data_ptr(), Q.numel, lr, BETAS[0],
                     BETAS[1], EPS, WD, step, inv_scale, Q.flat16.data_ptr(), 1)
            if fused:
                L.pt_adamw_ema_f32(*adamw, shadow_q.data_ptr(), omd, ops._stream())
            else:
                L.pt_adamw_fused_f32(*adamw, ops._stream())
        if ema == "separate":
            L.pt_ema_update_f32(shadow_q.data_ptr(), Q.flat.data_ptr(), Q.numel, omd, ops._stream())
        torch.cuda.synchronize()
        assert torch.equal(P.flat, Q.flat) and torch.equal(P.flat16, Q.flat16) and torch.equal(P.grad, Q.grad), (kind, ema, step)
        assert all(float(P.raw(P.grad, k).abs().max()) == 0.0 for k in P.names)                   # zeroed by the pass
        assert all(torch.equal(P.raw(P.flat16, k), P.raw(P.flat, k).half()) for k in P.names)     # the mirror of the new parameters
        if A is not None:
            for name in ("state1", "state2", "absmax1", "absmax2", "exp_avg", "exp_avg_sq"):
                assert torch.equal(getattr(opt, name), getattr(A, name)), (kind, ema, step, name)
        else:
            assert torch.equal(opt.exp_avg, m) and torch.equal(opt.exp_avg_sq, v), (kind, ema, step)
        if shadow_p is not None:
            assert torch.equal(shadow_p, shadow_q), (kind, ema, step)
    assert not torch.equal(P.flat, ParamStore(sd, dev).flat)                                      # the steps moved the parameters ...
    if A is not None:
        assert float(opt.absmax1.abs().max()) > 0 and not bool((opt.state1 == opt.zero_codes[0]).all())      # ... and the state
    else:
        assert float(opt.exp_avg.abs().max()) > 0 and float(opt.exp_avg_sq.abs().max()) > 0
    if shadow_p is not None:
        assert not torch.equal(shadow_p, P.flat)
