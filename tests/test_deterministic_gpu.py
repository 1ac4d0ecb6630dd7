"""``ControlNetTrainer(deterministic=True)`` on the MI355X: the two-stage reductions of include/posetraj_det.h (``ptd_*``), kernel by
kernel, and the training step built on them.

Kernel level.  Each ``ptd_`` reduction is launched ``REPEATS`` times on one input, at the shapes where the atomic form is known to
differ from run to run (tests/test_grad_checkpoint_gpu.py's header) and with more than one partial per output - asserted from the
size query - and every launch must reproduce the first BITWISE.  The result is also held against the atomic entry point's and against
an fp64 torch reference, with the tolerances the existing tests of those entry points state (tests/test_backward_gpu.py: activation
gradients rel-L2 <= 1e-3, norm parameter gradients <= 5e-4, weight / bias gradients <= 3e-4, the blend weight <= 1e-3, the sum of
squares 1e-9).  How many of the atomic entry point's repeats differed is printed, not asserted: it shows the shape discriminates.

Trainer level.  The tiny networks on the inputs of tests/golden/train_grads.npz, the two-step pattern of
tests/test_grad_checkpoint_gpu.py (a fresh trainer's first step, an optimizer step at learning rate 0, a second step with all four
side streams live), inside ``torch.use_deterministic_algorithms(True)`` so that a nondeterministic torch op would raise.  Equalities
are ``torch.equal``."""
import contextlib
import math
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

REPEATS = 20


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def h16(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from posetraj_amd import hip, ops
    return hip.lib(), ops._stream()


def repeats(run, what):
    """``run(det)`` -> tuple of result tensors.  The deterministic form ``REPEATS`` times: all equal to the first (asserted); the atomic
    form as often: how many differ from ITS first (printed).  Returns the first result of each."""
    det = [run(True) for _ in range(REPEATS)]
    torch.cuda.synchronize()
    for r in det[1:]:
        assert all(torch.equal(a, b) for a, b in zip(det[0], r)), f"{what}: a deterministic launch differs from the first"
    atomic = [run(False) for _ in range(REPEATS)]
    torch.cuda.synchronize()
    differ = sum(1 for r in atomic[1:] if not all(torch.equal(a, b) for a, b in zip(atomic[0], r)))
    print(f"{what}: {REPEATS} ptd_ launches bitwise equal; the atomic entry point differed from its first result in {differ} of {REPEATS - 1} repeats")
    return det[0], atomic[0]


def ws_of(floats, dev):
    return torch.empty(max(int(floats), 2), dtype=torch.float32, device=dev)


# ------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("C0,C1,rows", [(64, 0, 256), (320, 0, 256), (64, 32, 256), (64, 0, 200)], ids=["c64", "c320", "two-source", "ragged-slab"])
def test_groupnorm_backward(dev, lib, C0, C1, rows):
    """rows_per_sample = 256, one sample, 32 groups (320 channels: a group straddles the two strips); two sources; 200 rows = three
    slabs of 64 and one of 8.  dgamma / dbeta accumulate on top of a non-zero buffer."""
    L, st = lib
    Ct, groups, eps = C0 + C1, 32, 1e-5
    x = h16(rows, Ct, seed=12, scale=1.5) + 0.3
    gm = (1 + 0.2 * torch.randn(Ct, generator=torch.Generator().manual_seed(13))).half()
    bt = (0.2 * torch.randn(Ct, generator=torch.Generator().manual_seed(14))).half()
    dy = h16(rows, Ct, seed=15)
    xr, gr, br = x.double().requires_grad_(True), gm.double().requires_grad_(True), bt.double().requires_grad_(True)
    F.silu(F.group_norm(xr.view(1, rows, Ct).permute(0, 2, 1), groups, gr, br, eps)).backward(dy.double().view(1, rows, Ct).permute(0, 2, 1))
    need = L.ptd_groupnorm_bwd_ws_floats(Ct, groups, rows, 1, 1)
    strips = (Ct + 255) // 256
    slabs = need // (strips * groups * 2 + 2 * Ct)
    assert need == slabs * (strips * groups * 2 + 2 * Ct) and slabs > 1
    x0, x1 = x[:, :C0].contiguous().to(dev), (x[:, C0:].contiguous().to(dev) if C1 else None)
    gd, bd, dyd = gm.to(dev), bt.to(dev), dy.to(dev)
    base = torch.linspace(-1, 1, 2 * Ct, device=dev)

    def run(det):
        dx0 = torch.empty((rows, C0), dtype=torch.float16, device=dev)
        dx1 = torch.empty((rows, C1), dtype=torch.float16, device=dev) if C1 else None
        stat = torch.empty(4 * groups, dtype=torch.float32, device=dev)
        par = base.clone()
        args = (x0.data_ptr(), x1.data_ptr() if C1 else None, C0, C1, groups, rows, 1, eps, gd.data_ptr(), bd.data_ptr(), 1, dyd.data_ptr(), dx0.data_ptr(),
                dx1.data_ptr() if C1 else None, par.data_ptr(), par.data_ptr() + 4 * Ct, stat.data_ptr())
        if det:
            ws = ws_of(need, dev)
            assert L.ptd_groupnorm_bwd(*args, ws.data_ptr(), need, st) == 0, L.pt_last_error()
        else:
            assert L.pt_groupnorm_bwd(*args, st) == 0, L.pt_last_error()
        return (dx0 if dx1 is None else torch.cat([dx0, dx1], 1)), par - base, stat

    det, atomic = repeats(run, f"groupnorm backward {C0}+{C1} channels, {rows} rows ({slabs} slabs x {strips} strips)")
    for name, got in (("ptd", det), ("pt", atomic)):
        assert rel(got[0], xr.grad) < 1e-3, name
        assert rel(got[1][:Ct], gr.grad) < 5e-4 and rel(got[1][Ct:], br.grad) < 5e-4, name
    assert rel(det[0], atomic[0]) < 1e-3 and rel(det[1], atomic[1]) < 5e-4


@pytest.mark.parametrize("rows,nseg,Cc", [(256, 1, 64), (256, 1, 128), (256, 1, 100), (256, 3, 64)], ids=["c64", "c128", "ragged-c100", "3-segments"])
def test_column_sums(dev, lib, rows, nseg, Cc):
    L, st = lib
    ld = (Cc + 7) // 8 * 8
    dy = h16(rows * nseg, ld, seed=41)
    want = dy.double().view(nseg, rows, ld)[:, :, :Cc].sum(1)
    need = L.ptd_colsum_ws_floats(rows, nseg, Cc)
    assert need % (nseg * Cc) == 0 and need // (nseg * Cc) > 1
    dyd = dy.to(dev)
    base = torch.linspace(-3, 3, nseg * Cc, device=dev).view(nseg, Cc)

    def run(det):
        out = base.clone()
        if det:
            ws = ws_of(need, dev)
            assert L.ptd_colsum_f16(dyd.data_ptr(), rows, nseg, Cc, ld, out.data_ptr(), ws.data_ptr(), need, st) == 0, L.pt_last_error()
        else:
            assert L.pt_colsum_f16(dyd.data_ptr(), rows, nseg, Cc, ld, out.data_ptr(), st) == 0, L.pt_last_error()
        return (out - base,)

    det, atomic = repeats(run, f"column sums {nseg} x {rows} rows x {Cc} columns ({need // (nseg * Cc)} slabs)")
    assert rel(det[0], want) < 3e-4 and rel(atomic[0], want) < 3e-4 and rel(det[0], atomic[0]) < 3e-4


@pytest.mark.parametrize("Cc", [320, 1280], ids=["narrow-320", "wave-per-row-1280"])
def test_layernorm_backward_parameter_gradients(dev, lib, Cc):
    L, st = lib
    M, eps = 1000, 1e-5
    x, dy = h16(M, Cc, seed=16, scale=2.0) + 0.5, h16(M, Cc, seed=17)
    gm = (1 + 0.2 * torch.randn(Cc, generator=torch.Generator().manual_seed(18))).half()
    xr, gr, br = x.double().requires_grad_(True), gm.double().requires_grad_(True), torch.zeros(Cc, dtype=torch.float64, requires_grad=True)
    F.layer_norm(xr, (Cc,), gr, br, eps).backward(dy.double())
    need = L.ptd_layernorm_bwd_ws_floats(M, Cc)
    assert need % (2 * Cc) == 0 and need // (2 * Cc) > 1
    xd, dyd, gd = x.to(dev), dy.to(dev), gm.to(dev)
    base = torch.linspace(-1, 1, 2 * Cc, device=dev)

    def run(det):
        dx = torch.empty_like(xd)
        par = base.clone()
        rowstat = torch.empty(2 * M, dtype=torch.float32, device=dev)
        args = (xd.data_ptr(), M, Cc, gd.data_ptr(), eps, dyd.data_ptr(), dx.data_ptr(), par.data_ptr(), par.data_ptr() + 4 * Cc, rowstat.data_ptr())
        if det:
            ws = ws_of(need, dev)
            assert L.ptd_layernorm_bwd(*args, ws.data_ptr(), need, st) == 0, L.pt_last_error()
        else:
            assert L.pt_layernorm_bwd(*args, st) == 0, L.pt_last_error()
        return dx, par - base

    det, atomic = repeats(run, f"layernorm backward [{M}, {Cc}] ({need // (2 * Cc)} partials)")
    for got in (det, atomic):
        assert rel(got[0], xr.grad) < 1e-3 and rel(got[1][:Cc], gr.grad) < 5e-4 and rel(got[1][Cc:], br.grad) < 5e-4
    print(f"dx of the two forms bitwise equal: {torch.equal(det[0], atomic[0])}")     # (it never crossed workgroups)
    assert rel(det[0], atomic[0]) < 1e-3 and rel(det[1], atomic[1]) < 5e-4


@pytest.mark.parametrize("device_scalar", [False, True], ids=["host-scale", "device-alpha"])
def test_dot_diff(dev, lib, device_scalar):
    L, st = lib
    n = 65536
    dy, a, b = h16(n, seed=51), h16(n, seed=52), h16(n, seed=53)
    alpha = 1.0 / (1.0 + math.exp(-0.3))
    want = alpha * (1 - alpha) * float((dy.double() * (a.double() - b.double())).sum())
    need = L.ptd_dot_diff_ws_floats(n)
    assert need > 1
    dyd, ad, bd = dy.to(dev), a.to(dev), b.to(dev)
    al = torch.tensor([alpha], dtype=torch.float32, device=dev)

    def run(det):
        out = torch.full((1,), 0.25, dtype=torch.float32, device=dev)
        ws = ws_of(need, dev)
        head = (dyd.data_ptr(), ad.data_ptr(), bd.data_ptr(), n)
        if device_scalar:
            rc = L.ptd_dot_diff_dev(*head, al.data_ptr(), out.data_ptr(), ws.data_ptr(), need, st) if det else L.pt_dot_diff_dev(*head, al.data_ptr(), out.data_ptr(), st)
        else:
            rc = L.ptd_dot_diff(*head, alpha * (1 - alpha), out.data_ptr(), ws.data_ptr(), need, st) if det else L.pt_dot_diff(*head, alpha * (1 - alpha), out.data_ptr(), st)
        assert rc == 0, L.pt_last_error()
        return (out - 0.25,)

    det, atomic = repeats(run, f"dot_diff n = {n} ({need} partials)")
    assert abs(float(det[0]) / want - 1) < 1e-3 and abs(float(atomic[0]) / want - 1) < 1e-3 and abs(float(det[0]) / float(atomic[0]) - 1) < 1e-3


def test_sum_of_squares(dev, lib):
    L, st = lib
    n = 1_000_003
    g = torch.randn(n, generator=torch.Generator().manual_seed(61)) * 37.0
    want = float((g.double() ** 2).sum())
    need = L.ptd_sumsq_ws_floats(n)
    assert need % 2 == 0 and need // 2 > 1
    gd = g.to(dev)

    def run(det):
        acc = torch.zeros(1, dtype=torch.float64, device=dev)
        ws = ws_of(need, dev)
        rc = L.ptd_sumsq_f32(gd.data_ptr(), n, acc.data_ptr(), ws.data_ptr(), need, st) if det else L.pt_sumsq_f32(gd.data_ptr(), n, acc.data_ptr(), st)
        assert rc == 0, L.pt_last_error()
        return (acc,)

    det, atomic = repeats(run, f"sumsq n = {n} ({need // 2} partials)")
    assert abs(float(det[0]) / want - 1) < 1e-9 and abs(float(atomic[0]) / want - 1) < 1e-9
    gd[17] = float("inf")
    assert not math.isfinite(float(run(True)[0]))


class _Sizes:
    """``hip.checked()`` with the results of the ``*_ws_floats`` queries kept."""

    def __init__(self, real):
        self.real, self.sizes = real, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if not name.endswith("_ws_floats"):
            return fn

        def query(*a):
            self.sizes.append((name, fn(*a)))
            return self.sizes[-1][1]
        return query


@pytest.mark.parametrize("K", [2048, 1100], ids=["K2048", "K1100-ragged-last-split"])
def test_split_k_weight_gradient_of_a_linear_layer(dev, K, monkeypatch):
    """``autodiff.gemm`` in accumulate mode, Co = Ci = 32, four splits (K = 1100: three of 320 and one of 140), on top of a non-zero C."""
    from posetraj_amd import autodiff as AD, hip
    Co = Ci = 32
    x, dy = h16(K, Ci, seed=7), h16(K, Co, seed=8)
    want = dy.double().t() @ x.double()
    xd, dyd = x.to(dev), dy.to(dev)
    base = torch.linspace(-2, 2, Co * Ci, device=dev).view(Co, Ci)
    spy = _Sizes(hip.checked())
    monkeypatch.setattr(hip, "checked", lambda: spy)

    def run(det):
        monkeypatch.setattr(AD, "DETERMINISTIC", det)
        c = base.clone()
        AD.gemm((dyd, 0), (xd, 0), (c, 0), Co, Ci, K, (1, Co), (Ci, 1), (Ci, 1), out_mode=2, splits=4)
        return (c - base,)

    det, atomic = repeats(run, f"split-K linear weight gradient 32 x 32, K = {K}")
    assert len(spy.sizes) == REPEATS and all(s == ("ptd_gemm_ws_floats", 4 * Co * Ci) for s in spy.sizes)          # four partials per output
    assert rel(det[0], want) < 3e-4 and rel(atomic[0], want) < 3e-4 and rel(det[0], atomic[0]) < 3e-4


def test_split_k_weight_gradient_of_a_gathered_convolution(dev, monkeypatch):
    """``Dense.accumulate`` of a 3 x 3 convolution, 4 images of 16 x 16, Co = Ci = 32: the gathered product over 1024 pixels in two
    splits, nine taps, into a non-zero gradient; the bias gradient's column sums with it."""
    from posetraj_amd import autodiff as AD, hip
    N, H, W, Ci, Co = 4, 16, 16, 32, 32
    x = h16(N, Ci, H, W, seed=4)
    w = torch.randn(Co, Ci, 3, 3, generator=torch.Generator().manual_seed(5)).half().double().requires_grad_(True)
    bias = torch.zeros(Co, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x.double(), w, bias, padding=1)
    dy = h16(*y.shape, seed=6)
    y.backward(dy.double())
    P = AD.ParamStore({"w": w.detach().float(), "b": bias.detach().float()}, dev)
    layer = AD.Dense(P, "w", "b", kind="conv", stride=1, padding=1)
    xd = x.permute(0, 2, 3, 1).contiguous().view(-1, Ci).to(dev)
    dyd = dy.permute(0, 2, 3, 1).contiguous().view(-1, Co).to(dev)
    base = torch.linspace(-1, 1, P.numel, device=dev)
    spy = _Sizes(hip.checked())
    monkeypatch.setattr(hip, "checked", lambda: spy)

    def run(det):
        monkeypatch.setattr(AD, "DETERMINISTIC", det)
        P.grad.copy_(base)
        layer.accumulate(xd, dyd, (N, H, W))
        g = P.grad - base
        return P.shaped(P.raw(g, "w"), "w").contiguous(), P.raw(g, "b").clone()

    det, atomic = repeats(run, "split-K 3 x 3 convolution weight gradient, 4 x 16 x 16 pixels, 32 -> 32 channels")
    gemm_sizes = [v for k, v in spy.sizes if k == "ptd_gemm_ws_floats"]
    assert len(gemm_sizes) == REPEATS and all(v == 2 * 9 * Co * Ci for v in gemm_sizes)                            # two partials per output
    for got in (det, atomic):
        assert rel(got[0], w.grad) < 3e-4 and rel(got[1], bias.grad) < 3e-4
    assert rel(det[0], atomic[0]) < 3e-4


# ------------------------------------------------------------------------------------------------- the training step
KW = dict(learning_rate=0.0, conditioning_dropout_prob=0.1, loss_scale=4096.0)


@contextlib.contextmanager
def strict_torch():
    """``torch.use_deterministic_algorithms(True)`` for the span of the steps: a nondeterministic torch op raises."""
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn)


def flat_grads(tr):
    g = tr.gradients()
    return torch.cat([g[k].reshape(-1) for k in tr.params.names])


@pytest.fixture(scope="module")
def nets(dev):
    from tests.test_backward_gpu import _nets
    return _nets(dev)


@pytest.fixture(scope="module")
def data(golden):
    g = golden("train_grads")
    t = lambda n: torch.from_numpy(g[n])
    batch = (t("latents"), t("emb"), torch.tensor([127.0]), t("traj"))
    draws = dict(noise=t("noise"), sigmas=t("sigmas"), random_p=t("random_p"), ran_idx=int(g["ran_idx"]))
    return g, batch, draws


def _two_steps(nets, data, **kw):
    """tests/test_grad_checkpoint_gpu.py's pattern: a fresh trainer's first step, an optimizer step that moves nothing, a second step
    with every side stream live.  Per phase: the result dict, the whole gradient, ``gradients()`` by name."""
    from posetraj_amd.training import ControlNetTrainer
    cn_o, un_o, un, cfg = nets
    _, batch, draws = data
    tr = ControlNetTrainer(cfg, cn_o.state_dict(), un, **dict(KW, **kw))
    phases = []
    with strict_torch():
        for phase in range(2):
            r = tr.loss_and_grads(*batch, **draws)
            phases.append(dict(out=r, flat=flat_grads(tr).cpu(), grads={k: v.cpu() for k, v in tr.gradients().items()}))
            if phase == 0:
                assert tr.optimizer_step() is True and float(tr.params.grad.abs().max()) == 0.0
    assert tr._sp_stream is not None and tr._side is not None and tr._enc_stream is not None and tr._pk_stream is not None
    return phases


@pytest.fixture(scope="module")
def runs(nets, data):
    """Computed once, shared, not modified."""
    return {"a": _two_steps(nets, data, deterministic=True), "b": _two_steps(nets, data, deterministic=True),
            True: _two_steps(nets, data, deterministic=True, gradient_checkpointing=True),
            "all": _two_steps(nets, data, deterministic=True, gradient_checkpointing="all"), "plain": _two_steps(nets, data)}


def test_two_fresh_trainers_agree_bit_for_bit(runs):
    first = runs["a"][0]["flat"]
    assert float(first.abs().max()) > 0 and bool(torch.isfinite(first).all())
    for key in ("a", "b"):
        for p in range(2):
            assert torch.equal(runs[key][p]["flat"], first), f"trainer {key}, step {p + 1}"
            a, b = runs[key][p]["out"], runs["plain"][p]["out"]
            assert a["loss"] == b["loss"] and a["loss_spatial"] == b["loss_spatial"] and a["loss_temporal"] == b["loss_temporal"]
    print(f"plain trainer, same inputs: whole gradient rel-L2 to the deterministic one {rel(runs['plain'][0]['flat'], first):.3e} (step 1), "
          f"{rel(runs['plain'][1]['flat'], first):.3e} (step 2); its two steps {rel(runs['plain'][1]['flat'], runs['plain'][0]['flat']):.3e} apart")


@pytest.mark.parametrize("mode", [True, "all"], ids=["controlnet", "all"])
def test_checkpointed_gradients_equal_the_plain_deterministic_ones(runs, mode):
    for p in range(2):
        assert torch.equal(runs[mode][p]["flat"], runs["a"][p]["flat"]), f"gradient_checkpointing={mode!r}, step {p + 1}"
        assert runs[mode][p]["out"]["loss"] == runs["a"][p]["out"]["loss"]


def test_gradients_against_the_reference_run(runs, nets, data):
    """The bounds of tests/test_backward_gpu.py::test_training_step_gradients_against_the_reference_run: stored samples of the reference
    script's own backward < 1.1e-3; fp32 autograd over the oracle < 1.2e-3 in all, < 3.0e-3 for the worst sizeable tensor."""
    from oracle import train as OT
    from tests.golden.make_golden import GRAD_FULL, GRAD_SUBSAMPLE
    from tests.test_backward_gpu import _compare_grads
    g, batch, draws = data
    cn_o, un_o, _, _ = nets
    r, grads = runs["a"][0]["out"], runs["a"][0]["grads"]
    assert abs(r["loss"] / float(g["loss"]) - 1) < 1e-3 and abs(r["loss_spatial"] / float(g["loss_spatial"]) - 1) < 1e-3
    sample = lambda x: (x.reshape(-1) if x.numel() <= GRAD_FULL else x.reshape(-1)[::GRAD_SUBSAMPLE]).float().numpy()
    got = np.concatenate([sample(grads[str(n)]) for n in g["names"]])
    rg = float(np.linalg.norm(got - g["grad_samples"]) / np.linalg.norm(g["grad_samples"]))
    ro = OT.training_step_grads(cn_o, un_o, batch[0], draws["noise"], draws["sigmas"], batch[1], batch[2], batch[3], 0.18215,
                                random_p=draws["random_p"], conditioning_dropout_prob=0.1, ran_idx=draws["ran_idx"])
    total, worst = _compare_grads(grads, ro["grads"], "deterministic step")
    print(f"deterministic step: stored gradient values rel-L2 {rg:.2e}")
    assert rg < 1.1e-3
    assert total < 1.2e-3 and worst < 3.0e-3


def test_accumulation_over_two_different_micro_batches(nets, data):
    from posetraj_amd.training import ControlNetTrainer
    cn_o, un_o, un, cfg = nets
    _, batch, draws = data
    gen = torch.Generator().manual_seed(7)
    second = dict(noise=torch.randn(batch[0].shape, generator=gen), sigmas=torch.tensor([0.6]), random_p=torch.tensor([0.95]),
                  ran_idx=(draws["ran_idx"] + 1) % batch[0].shape[1])
    batch2 = ((batch[0] * 0.9).half().float(),) + batch[1:]
    got = []
    with strict_torch():
        for _ in range(2):
            tr = ControlNetTrainer(cfg, cn_o.state_dict(), un, deterministic=True, gradient_accumulation_steps=2, **KW)
            assert tr.step(*batch, **draws)["stepped"] is None
            one = flat_grads(tr).cpu()
            tr.loss_and_grads(*batch2, **second)
            got.append(flat_grads(tr).cpu())
            assert not torch.equal(one, got[-1]) and tr.optimizer_step() is True
    assert torch.equal(got[0], got[1])


def test_camera_twin_without_the_spatial_loss(dev):
    from oracle import init as OI, nets as ON
    from posetraj_amd import UNetSpatioTemporalConditionControlNetModel
    from posetraj_amd.training import ControlNetTrainer
    from tests.golden.make_golden import TRAIN_CE, TRAIN_CFG
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        cn_o = OI.seeded_init_(ON.ControlNetSDVModel(**TRAIN_CFG, conditioning_embedding_out_channels=TRAIN_CE, camera=True), seed=91)
        un_o = OI.seeded_init_(ON.UNetSpatioTemporalConditionControlNetModel(**TRAIN_CFG), seed=92)
    with torch.no_grad():
        for m in (cn_o, un_o):
            for prm in m.parameters():
                prm.copy_(prm.half().float())
    un = UNetSpatioTemporalConditionControlNetModel(**TRAIN_CFG).load_state_dict(un_o.state_dict(), dev, keep_source=True)
    cfg = dict(TRAIN_CFG, conditioning_embedding_out_channels=TRAIN_CE, down_block_types=un.config.down_block_types, camera=True)
    g = torch.Generator().manual_seed(93)
    Fr, h, w = 4, 8, 8
    lat = (torch.randn(1, Fr, 4, h, w, generator=g) * 0.18215 * 5).half().float()
    emb = torch.randn(1, 1, 16, generator=g).half().float()
    traj = (torch.rand(1, Fr, 3, h * 8, w * 8, generator=g) * 2 - 1).half().float()
    cam = (torch.randn(1, Fr, 12, generator=g) * 0.5).half().float()
    noise, sig = torch.randn(lat.shape, generator=g), torch.tensor([0.9])
    got = []
    with strict_torch():
        for _ in range(2):
            tr = ControlNetTrainer(cfg, cn_o.state_dict(), un, deterministic=True, learning_rate=0.0, conditioning_dropout_prob=None, loss_scale=4096.0)
            r = tr.loss_and_grads(lat, emb, torch.tensor([127.0]), traj, noise=noise, sigmas=sig, use_spatial=False, camera_cond=cam)
            assert r["loss_spatial"] is None
            got.append((r["loss"], flat_grads(tr).cpu()))
    assert got[0][0] == got[1][0] and float(got[0][1].abs().max()) > 0 and torch.equal(got[0][1], got[1][1])


def test_two_optimizer_steps_with_ema_and_8bit_adam(nets, data):
    from posetraj_amd.training import ControlNetTrainer
    cn_o, un_o, un, cfg = nets
    _, batch, draws = data
    got = []
    with strict_torch():
        for _ in range(2):
            tr = ControlNetTrainer(cfg, cn_o.state_dict(), un, deterministic=True, use_ema=True, use_8bit_adam=True, **dict(KW, learning_rate=2e-4))
            norms = []
            for _ in range(2):
                o = tr.step(*batch, **draws)
                assert o["stepped"] is True
                norms.append(o["grad_norm"])
            got.append((tr.params.flat.cpu(), tr.ema.shadow.cpu(), norms))
    assert not torch.equal(got[0][0], got[0][1])                   # (the parameters moved away from the shadow)
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]) and got[0][2] == got[1][2]
    assert all(math.isfinite(v) and v > 0 for v in got[0][2])


def test_resume_equals_the_uninterrupted_run(nets, data):
    from posetraj_amd.training import ControlNetTrainer
    cn_o, un_o, un, cfg = nets
    _, batch, draws = data
    kw = dict(KW, learning_rate=2e-4, deterministic=True)
    with strict_torch():
        whole = ControlNetTrainer(cfg, cn_o.state_dict(), un, **kw)
        assert whole.step(*batch, **draws)["stepped"] is True and whole.step(*batch, **draws)["stepped"] is True
        first = ControlNetTrainer(cfg, cn_o.state_dict(), un, **kw)
        assert first.step(*batch, **draws)["stepped"] is True
        second = ControlNetTrainer(cfg, cn_o.state_dict(), un, **kw)
        with tempfile.TemporaryDirectory() as d:
            first.save_state(d)
            second.load_state(d)
        assert second.optimizer_steps == 1 and second.step(*batch, **draws)["stepped"] is True
    assert not torch.equal(whole.params.flat, first.params.flat)
    assert torch.equal(whole.params.flat, second.params.flat)


def test_the_default_trainer_calls_no_ptd_entry(nets, data, monkeypatch):
    """``deterministic=False``: not one ``ptd_`` entry point is asked for, and the sequence of entry points the step calls is the
    deterministic trainer's with every ``ptd_x`` read as ``pt_x`` (its size queries aside) - the flag changes which form of a
    reduction runs and nothing else about the step."""
    from posetraj_amd import hip
    from posetraj_amd.training import ControlNetTrainer
    cn_o, un_o, un, cfg = nets
    _, batch, draws = data
    real, names = hip.checked(), []

    class Recording:
        def __getattr__(self, name):
            names.append(name)
            return getattr(real, name)

    monkeypatch.setattr(hip, "checked", lambda: Recording())
    seqs = {}
    for det in (False, True):
        tr = ControlNetTrainer(cfg, cn_o.state_dict(), un, deterministic=det, **KW)
        del names[:]
        out = tr.step(*batch, **draws)
        assert out["stepped"] is True
        seqs[det] = list(names)
    assert not any(n.startswith("ptd_") for n in seqs[False])
    used = {n for n in seqs[True] if n.startswith("ptd_")}
    print("ptd_ entry points of one deterministic step:", sorted(used))
    assert used >= {"ptd_gemm_f16", "ptd_colsum_f16", "ptd_groupnorm_bwd", "ptd_layernorm_bwd", "ptd_dot_diff", "ptd_sumsq_f32"}, used
    mapped = [("pt_" + n[4:]) if n.startswith("ptd_") else n for n in seqs[True] if not (n.startswith("ptd_") and n.endswith("_ws_floats"))]
    assert mapped == seqs[False] and len(seqs[False]) > 500


def test_the_keyword_refuses_the_captured_step(nets):
    from posetraj_amd.training import ControlNetTrainer
    cn_o, un_o, un, cfg = nets
    with pytest.raises(ValueError, match="deterministic"):
        ControlNetTrainer(cfg, cn_o.state_dict(), un, deterministic=True, use_graph=True)
    assert ControlNetTrainer(cfg, cn_o.state_dict(), un).deterministic is False
