"""``ControlNetTrainer(gradient_checkpointing=...)`` on the MI355X: the tiny networks of tests/golden/make_golden.py (``TRAIN_CFG`` /
``TRAIN_CE``) on the inputs of tests/golden/train_grads.npz (4 frames, 8 x 8 latent), in the three modes ``False`` / ``True`` / ``"all"``.

What must hold.  The forward of a checkpointed step is the same launches: both losses are EQUAL (``==``).  The recomputation runs the
forward kernels again, which are bit-reproducible - checked directly, tensor by tensor, in
``test_recomputed_segments_equal_the_dropped_ones_bit_for_bit`` - and the reverse pass visits the same closures in the same order: the
gradients can differ from the ``False`` trainer's only the way two ``False`` runs differ from each other, by the order of the
backward's fp32 atomics.  That noise floor is measured here - the largest whole-gradient rel-L2 between repeated ``False`` steps of
fresh trainers - and a checkpointed mode must lie within ``max(4 x floor, 1e-6)`` of a ``False`` run: 4 because both sides are draws
of the same noise, 1e-6 the scale of fp32 summation order.

The floor is not small on these networks, and it is not one number per run.  Measured over sixteen steps (ten ``False``, three of
each mode): the whole gradients fall into a few discrete distances - 4.5e-4, 1.6e-5, 1e-7, 1e-8 .. 1e-9 - in combination, the
checkpointed runs spread over them like the plain ones.  Two sources were reproduced in isolation, 100 repeats on one input each:
``pt_groupnorm_bwd`` at ``rows_per_sample = F S = 256``, one sample (the temporal residual block's norms: several workgroups
``atomicAdd`` a sample's four statistics, the fp16 ``dx`` computed from them differed bitwise in 90 repeats; at the spatial shapes in
none), and ``pt_colsum_f16`` at 256 rows per segment (fp32 sums differed in 36 and 100 repeats at 64 and 128 columns; their fp16
cast, the time-embedding gradient, in none on that input).  The 4.5e-4 step reaches 370 of 406 parameters, the 1.6e-5 step the
time-embedding layers first.  A floor from three repeats therefore misses the 4.5e-4 step in about one run in four, and would then
fail a correct checkpointed run that shows it: ``REPEATS`` fresh ``False`` trainers, two steps each, are pooled instead (the two
steps compute the same gradient: the optimizer step between them runs at learning rate 0), which leaves that chance below 1e-3.
When the step is seen the bound is 1.8e-3: it guards against a dropped or doubled gradient, not against one fp16 ulp - the
bit-for-bit test does that.  Accumulation and the camera twin measure their own floors on their own configurations.

Every trainer takes two steps: the first of a fresh trainer (the spatial pass still shares the main stream while the packs are
built), then - behind an optimizer step at learning rate 0, which moves no parameter but sets the pack stream going - one with all
four side streams live, where the spatial pass's recomputation runs on the spatial stream."""
import contextlib
import io
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MODES = (False, True, "all")
KW = dict(learning_rate=0.0, conditioning_dropout_prob=0.1, loss_scale=4096.0)
REPEATS = 8           # False trainers behind a floor: the 4.5e-4 step showed in 6 of 16 steps, so 8 x 2 pooled steps miss it with
#                       probability 0.625 ** 16 + 0.375 ** 16 = 5e-4 (and then only a checkpointed run that shows it fails)


def rel(a, b):
    return float((a - b).norm() / b.norm())


def bound(floor):
    return max(4.0 * floor, 1e-6)


def floor_of(flats):
    """Largest distance between any two of the repeated plain gradients."""
    return max(rel(a, b) for i, a in enumerate(flats) for b in flats[:i])


def flat_grads(tr):
    g = tr.gradients()
    return torch.cat([g[k].reshape(-1) for k in tr.params.names]).double().cpu()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


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


def _two_steps(nets, data, mode):
    """A fresh trainer's first step, an optimizer step that moves nothing, a second step: per phase the result dict, the whole
    gradient, ``gradients()`` by name and the ``grad_ready`` sequence."""
    from posetraj_amd.training import ControlNetTrainer
    cn_o, un_o, un, cfg = nets
    _, batch, draws = data
    tr = ControlNetTrainer(cfg, cn_o.state_dict(), un, gradient_checkpointing=mode, **KW)
    seq = []
    tr.params.on_grad_ready = seq.append
    phases = []
    for phase in range(2):
        del seq[:]
        r = tr.loss_and_grads(*batch, **draws)
        phases.append(dict(out=r, flat=flat_grads(tr), grads={k: v.cpu() for k, v in tr.gradients().items()}, seq=list(seq)))
        if phase == 0:
            before = tr.params.flat.clone()
            assert tr.optimizer_step() is True
            assert torch.equal(before, tr.params.flat) and float(tr.params.grad.abs().max()) == 0.0
    assert tr._sp_stream is not None and tr._side is not None and tr._enc_stream is not None and tr._pk_stream is not None
    return phases


@pytest.fixture(scope="module")
def runs(nets, data):
    """Computed once, shared, not modified: ``REPEATS`` ``False`` trainers (the noise floor, pooled over their two steps), one trainer
    per checkpointed mode."""
    plain = [_two_steps(nets, data, False) for _ in range(REPEATS)]
    pool = [q[p]["flat"] for q in plain for p in range(2)]
    floor = floor_of(pool)
    res = {False: plain[0], True: _two_steps(nets, data, True), "all": _two_steps(nets, data, "all"), "pool": pool}
    for q in plain[1:]:                                         # (only the whole gradients of the repeats are kept)
        for ph in q:
            ph.pop("grads")
    return res, floor


@pytest.fixture(scope="module")
def oracle(nets, data):
    from oracle import train as OT
    cn_o, un_o, _, _ = nets
    _, batch, draws = data
    return OT.training_step_grads(cn_o, un_o, batch[0], draws["noise"], draws["sigmas"], batch[1], batch[2], batch[3], 0.18215,
                                  random_p=draws["random_p"], conditioning_dropout_prob=0.1, ran_idx=draws["ran_idx"])


@pytest.mark.parametrize("mode", [True, "all"], ids=["controlnet", "all"])
def test_losses_are_equal_in_every_mode(runs, mode):
    res, _ = runs
    for p in range(2):
        a, b = res[mode][p]["out"], res[False][p]["out"]
        print(f"step {p + 1}, gradient_checkpointing={mode!r}: loss {a['loss']!r} vs {b['loss']!r}; spatial {a['loss_spatial']!r} vs {b['loss_spatial']!r}")
        assert a["loss"] == b["loss"] and a["loss_spatial"] == b["loss_spatial"] and a["loss_temporal"] == b["loss_temporal"]


@pytest.mark.parametrize("mode", [True, "all"], ids=["controlnet", "all"])
def test_gradients_within_the_noise_floor_of_the_plain_step(runs, mode):
    res, floor = runs
    for p in range(2):
        d = rel(res[mode][p]["flat"], res[False][p]["flat"])
        each = sorted(rel(res[mode][p]["flat"], q) for q in res["pool"])
        print(f"step {p + 1}: floor ({len(res['pool'])} False steps) {floor:.3e}; gradient_checkpointing={mode!r} vs False {d:.3e}; bound {bound(floor):.3e}; "
              f"nearest False step {each[0]:.3e}; all: {' '.join(f'{v:.1e}' for v in each)}")
    for p in range(2):
        assert rel(res[mode][p]["flat"], res[False][p]["flat"]) <= bound(floor)


@pytest.mark.parametrize("mode", [True, "all"], ids=["controlnet", "all"])
def test_gradients_against_the_reference_run(runs, data, oracle, mode):
    """The bounds tests/test_backward_gpu.py::test_training_step_gradients_against_the_reference_run states: stored samples of the
    reference script's own backward < 1.1e-3, fp32 autograd over the oracle < 1.2e-3 in all, < 3.0e-3 for the worst sizeable tensor."""
    from tests.golden.make_golden import GRAD_FULL, GRAD_SUBSAMPLE
    from tests.test_backward_gpu import _compare_grads
    g, _, _ = data
    res, _ = runs
    for p in range(2):
        r, grads = res[mode][p]["out"], res[mode][p]["grads"]
        assert abs(r["loss"] / float(g["loss"]) - 1) < 1e-3 and abs(r["loss_spatial"] / float(g["loss_spatial"]) - 1) < 1e-3
        sample = lambda x: (x.reshape(-1) if x.numel() <= GRAD_FULL else x.reshape(-1)[::GRAD_SUBSAMPLE]).float().numpy()
        got = np.concatenate([sample(grads[str(n)]) for n in g["names"]])
        rg = float(np.linalg.norm(got - g["grad_samples"]) / np.linalg.norm(g["grad_samples"]))
        total, worst = _compare_grads(grads, oracle["grads"], f"gradient_checkpointing={mode!r}, step {p + 1}")
        print(f"gradient_checkpointing={mode!r}, step {p + 1}: stored gradient values rel-L2 {rg:.2e}")
        assert rg < 1.1e-3
        assert total < 1.2e-3 and worst < 3.0e-3


def test_grad_ready_sequence_is_the_same_in_every_mode(runs):
    res, _ = runs
    for p in range(2):
        want = res[False][p]["seq"]
        assert len(want) > 50 and len(set(want)) == len(want)              # each name once per micro-batch
        for mode in (True, "all"):
            assert res[mode][p]["seq"] == want


def test_accumulation_over_two_different_micro_batches(nets, data):
    """Two different micro-batches into one gradient; the floor is this configuration's own (``REPEATS`` ``False`` trainers)."""
    from posetraj_amd.training import ControlNetTrainer
    cn_o, un_o, un, cfg = nets
    _, batch, draws = data
    gen = torch.Generator().manual_seed(7)
    F = batch[0].shape[1]
    second = dict(noise=torch.randn(batch[0].shape, generator=gen), sigmas=torch.tensor([0.6]), random_p=torch.tensor([0.95]),
                  ran_idx=(draws["ran_idx"] + 1) % F)
    batch2 = ((batch[0] * 0.9).half().float(),) + batch[1:]
    got = {}
    for mode in (False,) * REPEATS + (True, "all"):
        tr = ControlNetTrainer(cfg, cn_o.state_dict(), un, gradient_checkpointing=mode, gradient_accumulation_steps=2, **KW)
        assert tr.step(*batch, **draws)["stepped"] is None
        tr.loss_and_grads(*batch2, **second)
        got.setdefault(mode, []).append(flat_grads(tr))
        assert tr.optimizer_step() is True
    floor = floor_of(got[False])
    for mode in (True, "all"):
        d = rel(got[mode][0], got[False][0])
        print(f"two accumulated micro-batches: gradient_checkpointing={mode!r} vs False {d:.3e}; floor ({REPEATS} False trainers) {floor:.3e}; "
              f"bound {bound(floor):.3e}; nearest False trainer {min(rel(got[mode][0], q) for q in got[False]):.3e}")
    for mode in (True, "all"):
        assert rel(got[mode][0], got[False][0]) <= bound(floor)


def test_camera_twin_at_17_frames(dev):
    """``camera=True``, ``use_spatial=False``, ``"all"``, 17 frames: the two-block temporal attention backward runs inside recomputed
    segments.  At an 8 x 8 latent, the smallest the four-level networks take (three halvings; the frozen decoder's skip connections
    do not line up below it).  The floor is this configuration's own (``REPEATS`` ``False`` trainers)."""
    from oracle import init as OI, nets as ON
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
    g = torch.Generator().manual_seed(94)
    Fr, h, w = 17, 8, 8
    lat = (torch.randn(1, Fr, 4, h, w, generator=g) * 0.18215 * 5).half().float()
    emb = torch.randn(1, 1, 16, generator=g).half().float()
    traj = (torch.rand(1, Fr, 3, h * 8, w * 8, generator=g) * 2 - 1).half().float()
    cam = (torch.randn(1, Fr, 12, generator=g) * 0.5).half().float()
    noise, sig = torch.randn(lat.shape, generator=g), torch.tensor([0.9])
    got = []
    for mode in (False,) * REPEATS + ("all",):
        tr = ControlNetTrainer(cfg, cn_o.state_dict(), un, gradient_checkpointing=mode, learning_rate=0.0, conditioning_dropout_prob=None,
                               loss_scale=4096.0)
        r = tr.loss_and_grads(lat, emb, torch.tensor([127.0]), traj, noise=noise, sigmas=sig, use_spatial=False, camera_cond=cam)
        assert r["loss_spatial"] is None
        got.append((r["loss"], flat_grads(tr)))
    plain = [f for _, f in got[:REPEATS]]
    floor, d = floor_of(plain), rel(got[-1][1], got[0][1])
    print(f"camera twin, 17 frames: \"all\" vs False {d:.3e}; floor ({REPEATS} False trainers) {floor:.3e}; bound {bound(floor):.3e}; "
          f"nearest False trainer {min(rel(got[-1][1], q) for q in plain):.3e}")
    assert all(l == got[0][0] for l, _ in got) and float(got[0][1].norm()) > 0
    assert d <= bound(floor)


def test_peak_memory_falls_with_every_mode(dev, nets):
    """14 frames at a 32 x 32 latent, where the tiny networks' activations outweigh their parameters: the high-water mark of one
    ``loss_and_grads`` (after a warm-up step that builds the packs and the streams) must fall strictly from ``False`` to ``True`` to
    ``"all"``.  By how much is a measurement, printed."""
    from posetraj_amd.training import ControlNetTrainer
    cn_o, un_o, un, cfg = nets
    g = torch.Generator().manual_seed(95)
    Fr, h, w = 14, 32, 32
    lat = (torch.randn(1, Fr, 4, h, w, generator=g) * 0.18215 * 5).half().float()
    emb = torch.randn(1, 1, 16, generator=g).half().float()
    traj = (torch.rand(1, Fr, 3, h * 8, w * 8, generator=g) * 2 - 1).half().float()
    draws = dict(noise=torch.randn(lat.shape, generator=g), sigmas=torch.tensor([0.9]), random_p=torch.tensor([0.7]), ran_idx=5)
    peak, loss = {}, {}
    for mode in MODES:
        tr = ControlNetTrainer(cfg, cn_o.state_dict(), un, gradient_checkpointing=mode, **KW)
        assert tr.step(lat, emb, torch.tensor([127.0]), traj, **draws)["stepped"] is True
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        loss[mode] = tr.loss_and_grads(lat, emb, torch.tensor([127.0]), traj, **draws)["loss"]
        torch.cuda.synchronize()
        peak[mode] = torch.cuda.max_memory_allocated()
        print(f"gradient_checkpointing={mode!r}: peak {peak[mode] / 2 ** 20:.1f} MiB over one loss_and_grads ({(peak[mode] - base) / 2 ** 20:.1f} MiB above "
              f"the {base / 2 ** 20:.1f} MiB held before it)")
        del tr
    assert loss[True] == loss[False] and loss["all"] == loss[False]
    assert peak["all"] < peak[True] < peak[False]


def test_values_the_keyword_refuses(nets):
    from posetraj_amd.training import ControlNetTrainer
    cn_o, un_o, un, cfg = nets
    for bad in ("controlnet", 1, None, "ALL"):
        with pytest.raises(ValueError, match="gradient_checkpointing"):
            ControlNetTrainer(cfg, cn_o.state_dict(), un, gradient_checkpointing=bad)
    for mode in (True, "all"):
        with pytest.raises(ValueError, match="use_graph"):
            ControlNetTrainer(cfg, cn_o.state_dict(), un, gradient_checkpointing=mode, use_graph=True)
    assert ControlNetTrainer(cfg, cn_o.state_dict(), un, use_graph=True).gradient_checkpointing is False


def test_ema_and_8bit_adam_step_under_checkpointing(nets, data):
    """The optimizer side knows nothing of the mode: an ``"all"`` trainer with ``use_ema`` and ``use_8bit_adam`` takes its steps, its
    first loss equal to the ``False`` trainer's, and a state saved in one mode loads into another."""
    import tempfile
    from posetraj_amd.training import ControlNetTrainer
    cn_o, un_o, un, cfg = nets
    _, batch, draws = data
    kw = dict(KW, learning_rate=2e-4, use_ema=True, use_8bit_adam=True)
    a = ControlNetTrainer(cfg, cn_o.state_dict(), un, gradient_checkpointing="all", **kw)
    b = ControlNetTrainer(cfg, cn_o.state_dict(), un, **kw)
    oa, ob = a.step(*batch, **draws), b.step(*batch, **draws)
    assert oa["stepped"] is True and ob["stepped"] is True and oa["loss"] == ob["loss"]
    oa = a.step(*batch, **draws)
    assert oa["stepped"] is True and math.isfinite(oa["loss"]) and a.ema.optimization_step == 2
    with tempfile.TemporaryDirectory() as d:
        a.save_state(d)
        b.load_state(d)
    assert b.optimizer_steps == 2 and torch.equal(a.params.flat, b.params.flat)


PRIMITIVES = ("dense", "groupnorm", "layernorm", "silu", "geglu", "add", "add_rowvec", "blend", "attn_spatial", "attn_temporal")


def test_recomputed_segments_equal_the_dropped_ones_bit_for_bit(nets, data, monkeypatch):
    """What the whole scheme rests on, checked directly and independently of the reverse pass's noise: in a real ``"all"`` step with
    every side stream live, each segment's function runs exactly twice, and the second run - in the reverse pass, on whichever stream
    reverses it - reproduces the output of EVERY primitive of the first (``torch.equal``: the segment's result and all its
    intermediates).  Covers each residual block and transformer of the ControlNet and of the decoder in both passes."""
    from posetraj_amd import autodiff as AD
    from posetraj_amd.training import ControlNetTrainer
    cn_o, un_o, un, cfg = nets
    _, batch, draws = data
    tr = ControlNetTrainer(cfg, cn_o.state_dict(), un, gradient_checkpointing="all", **KW)
    assert tr.step(*batch, **draws)["stepped"] is True          # packs and streams exist: the next step uses all four
    current, segments = [None], []
    for name in PRIMITIVES:
        def spy(*a, _f=getattr(AD, name), **k):
            out = _f(*a, **k)
            if current[0] is not None:
                current[0].append(out.v)
            return out
        monkeypatch.setattr(AD, name, spy)
    real = AD.checkpoint

    def checkpoint(tape, fn):
        calls = []
        segments.append(calls)

        def traced(t):
            current[0] = []
            out = fn(t)
            calls.append(current[0] + [out.v])
            current[0] = None
            return out
        return real(tape, traced)
    monkeypatch.setattr(AD, "checkpoint", checkpoint)
    r = tr.loss_and_grads(*batch, **draws)
    torch.cuda.synchronize()
    n_cn = sum(len(b.resnets) + len(b.attns) for b in tr.controlnet.down) + len(tr.controlnet.mid)
    n_dec = sum(len(b.resnets) + len(b.attns) for b in tr.decoder.up)
    assert math.isfinite(r["loss"]) and len(segments) == n_cn + 2 * n_dec
    tensors = 0
    for calls in segments:
        assert len(calls) == 2 and len(calls[0]) == len(calls[1]) > 10
        for a, b in zip(*calls):
            assert a.data_ptr() != b.data_ptr() or a.numel() == 0
            assert torch.equal(a, b)
        tensors += len(calls[0])
    print(f"{len(segments)} segments, {tensors} primitive outputs each computed twice: all bit-identical")
