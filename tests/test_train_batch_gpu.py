"""Batches of clips per training step on the MI355X (``ControlNetTrainer`` at ``per_gpu_batch_size`` > 1): the two kernels of
include/posetraj_batch.h exactly, on integer data, against index arithmetic; the step on the tiny networks of
tests/golden/make_golden.py (``TRAIN_CFG`` / ``TRAIN_CE``; 4 frames on an 8 x 8 latent, so S = 64, 16, 4, 1 over the levels) against
fp32 autograd over the oracle, with inputs that differ per clip; the per-clip spatial loss; equal clips; no leak
between clips; the trainer's modes at two clips; one clip untouched.

B = 3 wherever the context index matters: 64 mod 3 = 16 mod 3 = 4 mod 3 = 1, so the context class of a position shifts from clip to
clip, and S = 1 gives j = b - `s mod B` or `b` cannot pass all levels.

Bounds against fp32 autograd.  Losses: 1e-3, the one-clip step's.  Gradients of clips WITHOUT conditioning dropout: the one-clip
step's (tests/test_backward_gpu.py: whole gradient 1.2e-3, worst sizeable tensor 3.0e-3; measured here 9.4e-4 - 1.02e-3 / 2.2 - 2.4e-3).
With dropout draws that hit one clip and not another (one clip loses embedding and image latent, one the image latent alone, one
nothing) the batch measures above them - and so does the
UNCHANGED one-clip step on those clips alone: 2.66e-3 / 6.6e-3 and 2.86e-3 / 8.8e-3 for the clip that lost both, 1.76e-3 / 4.0e-3
for the one that lost the image latent, 1.06e-3 / 2.6e-3 and 1.08e-3 / 2.4e-3 for the clip that lost nothing (a zeroed image latent
leaves half the input channels at zero; the error is the same at loss scale 16 384 and in deterministic mode, so neither underflow nor
summation order).  The batch lies between its clips: measured (profiles/r11/train_batch_parity.txt) B = 2: 2.23 - 2.27e-3 / 6.45 -
7.13e-3, with the spatial loss 2.14e-3 / 6.15 - 6.27e-3; B = 3: 2.02 - 2.04e-3 / 5.15 - 5.38e-3, with the spatial loss 1.89 - 1.93e-3 /
4.40 - 4.48e-3; the camera twin's networks at B = 2: 2.26e-3 / 1.03e-2.  ``DROP_BOUNDS`` holds 1.25 x the largest measured value of each.
The same clips are also noisier run to run: repeated plain two-clip steps with these draws lie up to 1.07e-3 apart (the order of the
reverse pass's fp32 atomics), where repeated one-clip steps without dropout lie 9e-6 apart."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

FR, H, W, D = 4, 8, 8, 16
DROP = 0.1
KW = dict(conditioning_dropout_prob=DROP, loss_scale=4096.0)
RANDOM_P = {1: [0.7], 2: [0.15, 0.7], 3: [0.15, 0.7, 0.25]}      # 0.15: embedding AND image latent dropped; 0.25: the image latent alone; 0.7: neither
ONE_CLIP_BOUNDS = (1.2e-3, 3.0e-3)
DROP_BOUNDS = {(2, False): (2.84e-3, 8.91e-3), (3, False): (2.55e-3, 6.73e-3), (2, True): (2.68e-3, 7.84e-3), (3, True): (2.41e-3, 5.60e-3),     # (B, spatial)
               "camera": (2.83e-3, 1.29e-2)}


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def ctx_index(B, F, S):
    r = torch.arange(B * F * S)
    return ((r // (F * S)) * S + r % S) % B


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def nets(dev):
    from tests.test_backward_gpu import _nets
    return _nets(dev)


def make_batch(B, seed=21, cam=False, drop=True):
    """Clips that differ in everything: latents, embedding, trajectories, sigma, motion value, dropout draw."""
    g = torch.Generator().manual_seed(seed)
    lat = (torch.randn(B, FR, 4, H, W, generator=g) * 0.18215 * 5).half().float()
    emb = torch.randn(B, 1, D, generator=g).half().float()
    traj = (torch.rand(B, FR, 3, H * 8, W * 8, generator=g) * 2 - 1).half().float()
    noise = torch.randn(lat.shape, generator=g)
    sig = torch.tensor([0.9, 1.7, 0.45, 2.6][:B])
    mv = torch.tensor([127.0, 60.0, 200.0, 15.0][:B])
    batch = (lat, emb, mv, traj)
    draws = dict(noise=noise, sigmas=sig, random_p=torch.tensor(RANDOM_P[B] if drop else [0.7] * B), ran_idx=2)
    if cam:
        draws["camera_cond"] = (torch.randn(B, FR, 12, generator=g) * 0.5).half().float()
    return batch, draws


def trainer(nets, **kw):
    from posetraj_amd.training import ControlNetTrainer
    cn_o, _, un, cfg = nets
    return ControlNetTrainer(cfg, cn_o.state_dict(), un, **dict(KW, **kw))


def flat(tr):
    g = tr.gradients()
    return torch.cat([g[k].reshape(-1) for k in tr.params.names]).double().cpu()


# ------------------------------------------------------------------------------------------------- the two kernels, exactly
SHAPES = [(2, 3, 4), (3, 2, 5), (3, 4, 64), (4, 1, 1), (3, 1, 16)]


@pytest.mark.parametrize("C", [8, 320])
@pytest.mark.parametrize("B,F,S", SHAPES)
def test_interleaved_rowvec_kernels_are_exact_on_integer_data(dev, B, F, S, C):
    """Small integers in fp16: every sum (at most 256 rows of |dy| <= 4 on top of a start value) is exact in fp32, so the add, the
    atomic reduction, the two-launch reduction and its repeat must EQUAL index arithmetic on the host.  (3, 2, 5): 10 rows per class, no
    multiple of the 8 row lanes; (3, 4, 64): four slabs per class and both loops of the add.  ``pt_add_rowvec_f16`` admits no C that
    is not a multiple of 8, nor do these."""
    from posetraj_amd import hip
    L = hip.checked()
    g = torch.Generator().manual_seed(B * 1000 + F * 100 + S + C)
    rows = B * F * S
    x = torch.randint(-8, 9, (rows, C), generator=g).half()
    vec = torch.randint(-8, 9, (B, C), generator=g).half()
    dy = torch.randint(-4, 5, (rows, C), generator=g).half()
    j = ctx_index(B, F, S)
    assert torch.equal(torch.bincount(j, minlength=B), torch.full((B,), F * S))             # every class holds exactly F S rows
    xd, vd, dyd = x.to(dev), vec.to(dev), dy.to(dev)
    y = torch.full((rows + 1, C), float("nan"), dtype=torch.float16, device=dev)              # one guard row behind the output
    L.ptb_add_rowvec_interleaved_f16(xd.data_ptr(), vd.data_ptr(), B, F, S, C, y.data_ptr(), None)
    assert torch.equal(y[:rows].cpu(), x + vec[j]) and bool(torch.isnan(y[rows]).all())
    want = torch.full((B, C), 3.0).index_add_(0, j, dy.float())                               # `out +=`: on top of what is there
    out = torch.full((B + 1, C), 3.0, dtype=torch.float32, device=dev)
    L.ptb_colsum_interleaved_f16(dyd.data_ptr(), B, F, S, C, out.data_ptr(), None)
    assert torch.equal(out[:B].cpu(), want) and bool((out[B] == 3.0).all())
    n = L.ptb_colsum_interleaved_ws_floats(B, F, S, C)
    res = []
    for fill in (float("nan"), 7.0):                                                          # whatever the workspace held
        ws = torch.full((n + 1,), fill, dtype=torch.float32, device=dev)
        out = torch.full((B + 1, C), 3.0, dtype=torch.float32, device=dev)
        L.ptb_colsum_interleaved_det_f16(dyd.data_ptr(), B, F, S, C, out.data_ptr(), ws.data_ptr(), n, None)
        assert torch.equal(out[:B].cpu(), want) and bool((out[B] == 3.0).all())
        assert bool(torch.isnan(ws[n])) if math.isnan(fill) else float(ws[n]) == fill
        res.append(out)
    assert torch.equal(res[0], res[1])
    with pytest.raises(RuntimeError, match="workspace"):
        L.ptb_colsum_interleaved_det_f16(dyd.data_ptr(), B, F, S, C, out.data_ptr(), ws.data_ptr(), n - 1, None)


def test_interleaved_rowvec_tape_op_plain_and_deterministic(dev):
    """``autodiff.add_rowvec_interleaved`` on fractional data against autograd over the gather: the gradient passes through to x, the
    context rows receive their classes' sums (one fp16 rounding of an fp32 sum); the deterministic form is bit-equal across runs."""
    from posetraj_amd import autodiff as AD
    B, F, S, C = 3, 4, 16, 64
    g = torch.Generator().manual_seed(3)
    x, vec, dy = (torch.randn(n, C, generator=g).half() for n in (B * F * S, B, B * F * S))
    j = ctx_index(B, F, S)
    vr = vec.float().requires_grad_(True)
    (x.float() + vr[j]).backward(dy.float())
    got = {}
    for det in (False, True, True):
        AD.DETERMINISTIC = det
        try:
            tape, xv, vv = AD.Tape(), AD.Var(x.to(dev)), AD.Var(vec.to(dev))
            o = AD.add_rowvec_interleaved(tape, xv, vv, B, F, S)
            o.g = dy.to(dev)
            tape.backward()
        finally:
            AD.DETERMINISTIC = False
        assert torch.equal(o.v.cpu(), (x.float() + vec.float()[j]).half()) and torch.equal(xv.g.cpu(), dy)
        assert rel(vv.g, vr.grad) < 5e-4
        got.setdefault(det, []).append(vv.g)
    assert torch.equal(got[True][0], got[True][1])
    with pytest.raises(ValueError):
        AD.add_rowvec_interleaved(AD.Tape(), AD.Var(x.to(dev)), AD.Var(vec.to(dev)), B, F, S + 1)


# ------------------------------------------------------------------------------------------------- the step against fp32 autograd
def oracle_step(nets, batch, draws, use_spatial):
    """fp32 autograd over the oracle's networks.  Without the spatial loss: ``oracle.train.training_step_grads``, which takes a
    batch.  With it: the PER-CLIP expression (clip b's own residual rows of frame ``ran_idx``, its own sigma, noisy latent and target;
    the mean over clips), built here from the oracle's networks - the reference's expression is not the target."""
    from oracle import train as OT
    cn_o, un_o = nets[0], nets[1]
    lat, emb, mv, traj = batch
    cam = draws.get("camera_cond")
    if not use_spatial:
        return OT.training_step_grads(cn_o, un_o, lat, draws["noise"], draws["sigmas"], emb, mv, traj, 0.18215, random_p=draws["random_p"],
                                      conditioning_dropout_prob=DROP, use_spatial=False, camera_cond=cam)
    B, F, ri = lat.shape[0], lat.shape[1], draws["ran_idx"]
    for p in un_o.parameters():
        p.requires_grad_(False)
    for p in cn_o.parameters():
        p.requires_grad_(True)
        p.grad = None
    inp, noisy, ts, ehs = OT.training_inputs(lat, draws["noise"], draws["sigmas"], emb, 0.18215, draws["random_p"], DROP)
    ids = OT.train_add_time_ids(6, mv, OT.TRAIN_NOISE_AUG, ehs.dtype, B)
    down, mid = cn_o(inp, ts, ehs, added_time_ids=ids, controlnet_cond=traj, return_dict=False)
    pred = un_o(inp, ts, ehs, added_time_ids=ids, down_block_additional_residuals=list(down), mid_block_additional_residual=mid, return_dict=False)[0]
    s5 = draws["sigmas"].reshape(B, 1, 1, 1, 1)
    loss_t = OT.edm_loss(pred, noisy, lat, s5)
    pred_s = un_o(inp[:, ri].unsqueeze(1), ts, ehs, added_time_ids=ids, down_block_additional_residuals=[d[ri::F] for d in down],
                  mid_block_additional_residual=mid[ri::F], return_dict=False)[0]
    loss_s = OT.edm_loss(pred_s, noisy[:, ri:ri + 1], lat[:, ri:ri + 1], s5)
    (loss_t + 0.5 * loss_s).backward()
    grads = {k: (torch.zeros_like(p) if p.grad is None else p.grad.detach().clone()) for k, p in cn_o.named_parameters()}
    for p in cn_o.parameters():
        p.grad = None
    return dict(loss=(loss_t + 0.5 * loss_s).detach(), loss_temporal=loss_t.detach(), loss_spatial=loss_s.detach(), grads=grads)


def check_step(nets, B, use_spatial, drop=True, label=""):
    from tests.test_backward_gpu import _compare_grads
    batch, draws = make_batch(B, drop=drop)
    label += " dropout hits some clips," if drop else " no clip dropped,"
    bt, bw = DROP_BOUNDS[(B, use_spatial)] if drop else ONE_CLIP_BOUNDS
    tr = trainer(nets)
    r = tr.loss_and_grads(*batch, use_spatial=use_spatial, **draws)
    ro = oracle_step(nets, batch, draws, use_spatial)
    for k in ("loss", "loss_temporal") + (("loss_spatial",) if use_spatial else ()):
        print(f"{label} B = {B}: {k} {r[k]:.6f} vs {float(ro[k]):.6f} ({abs(r[k] / float(ro[k]) - 1):.1e})")
    assert (r["loss_spatial"] is None) == (not use_spatial)
    total, worst = _compare_grads(tr.gradients(), ro["grads"], f"{label} B = {B}")
    for k in ("loss", "loss_temporal") + (("loss_spatial",) if use_spatial else ()):
        assert abs(r[k] / float(ro[k]) - 1) < 1e-3
    assert total < bt and worst < bw
    return tr


@pytest.mark.parametrize("drop", [True, False], ids=["dropout", "nodrop"])
@pytest.mark.parametrize("B", [2, 3])
def test_batched_step_against_fp32_autograd_without_the_spatial_loss(nets, B, drop):
    check_step(nets, B, False, drop, label="temporal loss only,")


@pytest.mark.parametrize("drop", [True, False], ids=["dropout", "nodrop"])
@pytest.mark.parametrize("B", [2, 3])
def test_batched_step_with_the_per_clip_spatial_loss_against_fp32_autograd(nets, B, drop):
    """``ran_idx`` = 2 of 4 frames: neither the first nor the last."""
    tr = check_step(nets, B, True, drop, label="temporal + per-clip spatial loss,")
    assert tr.optimizer_step() is True and float(tr.params.grad.abs().max()) == 0.0


def test_camera_twin_batched_step_against_fp32_autograd(dev):
    import contextlib
    import io
    from oracle import init as OI, nets as ON
    from posetraj_amd import UNetSpatioTemporalConditionControlNetModel
    from posetraj_amd.training import ControlNetTrainer
    from tests.golden.make_golden import TRAIN_CE, TRAIN_CFG
    from tests.test_backward_gpu import _compare_grads
    with contextlib.redirect_stdout(io.StringIO()):
        cn_o = OI.seeded_init_(ON.ControlNetSDVModel(**TRAIN_CFG, conditioning_embedding_out_channels=TRAIN_CE, camera=True), seed=91)
        un_o = OI.seeded_init_(ON.UNetSpatioTemporalConditionControlNetModel(**TRAIN_CFG), seed=92)
    with torch.no_grad():
        for m in (cn_o, un_o):
            for prm in m.parameters():
                prm.copy_(prm.half().float())
    un = UNetSpatioTemporalConditionControlNetModel(**TRAIN_CFG).load_state_dict(un_o.state_dict(), dev, keep_source=True)
    cfg = dict(TRAIN_CFG, conditioning_embedding_out_channels=TRAIN_CE, down_block_types=un.config.down_block_types, camera=True)
    batch, draws = make_batch(2, cam=True)
    tr = ControlNetTrainer(cfg, cn_o.state_dict(), un, **KW)
    r = tr.loss_and_grads(*batch, use_spatial=False, **draws)
    ro = oracle_step((cn_o, un_o), batch, draws, False)
    print(f"camera twin, B = 2: loss {r['loss']:.6f} vs {float(ro['loss']):.6f} ({abs(r['loss'] / float(ro['loss']) - 1):.1e})")
    total, worst = _compare_grads(tr.gradients(), ro["grads"], "camera twin, B = 2")
    assert r["loss_spatial"] is None and abs(r["loss"] / float(ro["loss"]) - 1) < 1e-3
    assert total < DROP_BOUNDS["camera"][0] and worst < DROP_BOUNDS["camera"][1]
    k = "controlnet_cond_embedding.cc_projection.weight"
    assert float(ro["grads"][k].norm()) > 0 and rel(tr.gradients()[k], ro["grads"][k]) < 1e-2
    with pytest.raises(ValueError, match="camera_cond"):
        tr.loss_and_grads(*batch, use_spatial=False, **dict(draws, camera_cond=draws["camera_cond"][:1]))


# ------------------------------------------------------------------------------------------------- equal clips, no leak
def test_three_equal_clips_give_the_one_clip_step(nets):
    """B = 3 copies of one clip with identical draws: identical contexts make the interleave moot and every norm is per sample, so
    the batch mean IS the one-clip loss and gradient - a wrong 1 / B, or a leak between clips through the temporal convolutions, the
    temporal attention or a GroupNorm, is not.  The batch trainer's loss scale is 3 x the one-clip trainer's: the loss kernel's 1 / B
    then hands every clip the one-clip step's output gradient.

    Two bounds.  (1) Reasoned: the batch runs the same network at three times the rows, for which ``pt_igemm_plan`` and the
    reductions choose other tiles, splits and slabs - other fp32 summation orders, so the forward already differs in fp16 roundings
    (the losses differ by 1.5e-5) and the two gradients are two realisations of the step's rounding noise, each within 1.2e-3 of fp32
    autograd (the one-clip bound): <= 2.4e-3 apart, losses within the one-clip 1e-3.  A wrong 1 / B is 0.67 away, a leak O(0.1).
    (2) The noise floor of repeated one-clip steps, measured the way tests/test_grad_checkpoint_gpu.py measures it - ``REPEATS`` fresh
    trainers, two steps each around an optimizer step at learning rate 0, pooled; max(4 x floor, 1e-6).  As that file describes, the
    floor is not one number: samples of four one-clip steps on this input gave 6.0e-6, 9.0e-6 and 5.2e-4 (the discrete step that an
    fp16 flip in a GroupNorm backward opens), and the equal-clips distance, 8.1 - 8.4e-4 in four runs, lies under 4 x the last and far
    above 4 x the others - a batch and a clip never share a summation order, so they differ the way two one-clip steps only
    sometimes do.  The pooled sixteen steps are what makes the floor see that step (profiles/r11/train_batch_parity.txt)."""
    from tests.test_grad_checkpoint_gpu import REPEATS, bound, floor_of
    (lat, emb, mv, traj), draws = make_batch(1)
    ones = []
    for _ in range(REPEATS):
        tr = trainer(nets, learning_rate=0.0)
        for phase in range(2):
            r1 = tr.loss_and_grads(lat, emb, mv, traj, **draws)
            ones.append(flat(tr))
            assert tr.optimizer_step() is True
    floor = floor_of(ones)
    rep = lambda t: t.repeat((3,) + (1,) * (t.dim() - 1))
    tr3 = trainer(nets, loss_scale=3 * 4096.0)
    r3 = tr3.loss_and_grads(rep(lat), rep(emb), rep(mv), rep(traj), noise=rep(draws["noise"]), sigmas=rep(draws["sigmas"]),
                            random_p=rep(draws["random_p"]), ran_idx=draws["ran_idx"])
    d = min(rel(flat(tr3), o) for o in ones)
    print(f"three equal clips vs one clip: losses {r3['loss']!r} / {r1['loss']!r}, spatial {r3['loss_spatial']!r} / {r1['loss_spatial']!r}; "
          f"whole gradient rel-L2 {d:.3e}; floor of {len(ones)} one-clip steps {floor:.3e}; bound {bound(floor):.3e}")
    assert abs(r3["loss"] / r1["loss"] - 1) < 1e-3 and abs(r3["loss_spatial"] / r1["loss_spatial"] - 1) < 1e-3
    assert d <= 2.4e-3
    assert d <= bound(floor)


def test_no_leak_between_clips(nets, monkeypatch):
    """Two clips that share ONE embedding (so the context cannot carry a change either): new latents, trajectories, noise, sigma and
    motion value for clip 1 leave clip 0's rows of ``model_pred`` - what the decoder pass of the tape hands to the loss - bit-identical,
    and change clip 1's."""
    (lat, emb, mv, traj), draws = make_batch(2)
    emb = emb[:1].repeat(2, 1, 1)
    draws = dict(draws, random_p=torch.tensor([0.7, 0.7]))
    (lat2, _, mv2, traj2), draws2 = make_batch(2, seed=77)
    preds = []
    for k in range(2):
        tr = trainer(nets)
        run = tr.decoder.run
        monkeypatch.setattr(tr.decoder, "run", lambda *a, _run=run, **kw: preds.append(_run(*a, **kw)) or preds[-1])
        if k == 0:
            tr.loss_and_grads(lat, emb, mv, traj, use_spatial=False, **draws)
        else:
            mix = lambda a, b: torch.cat([a[:1], b[1:]])
            tr.loss_and_grads(mix(lat, lat2), emb, mix(mv, mv2), mix(traj, traj2), use_spatial=False, noise=mix(draws["noise"], draws2["noise"]),
                              sigmas=torch.tensor([0.9, 0.5]), random_p=draws["random_p"], ran_idx=2)
    a, b = (p.v.view(2, FR * H * W, -1) for p in preds)
    assert torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------- modes at two clips
def test_accumulation_of_two_different_two_clip_micro_batches(nets):
    """The sum rule tests/test_backward_gpu.py checks for one clip, at its bounds (total < 1e-3, worst sizeable tensor < 5e-3): two
    half-weight micro-batches accumulate to the mean of their gradients.  The clips keep their conditioning: a clip whose image
    latent is dropped amplifies every difference a hundredfold (repeated plain steps 1.07e-3 apart instead of 9e-6, see above), and
    with such clips this comparison measured 1.12e-3 / 2.8e-3, with and without atomics - the halved loss scale's fp16 roundings
    through that clip, not the sum rule."""
    from tests.test_backward_gpu import _compare_grads
    b1, d1 = make_batch(2, drop=False)
    b2, d2 = make_batch(2, seed=55, drop=False)
    single = []
    for b, d in ((b1, d1), (b2, d2)):
        tr = trainer(nets)
        tr.loss_and_grads(*b, **d)
        single.append({k: v.cpu() for k, v in tr.gradients().items()})
    two = trainer(nets, gradient_accumulation_steps=2)
    assert two.step(*b1, **d1)["stepped"] is None
    out = two.step(*b2, **d2)
    want = {k: 0.5 * (single[0][k] + single[1][k]) for k in single[0]}
    assert out["stepped"] is True and math.isfinite(out["grad_norm"])
    two = trainer(nets, gradient_accumulation_steps=2)
    two.loss_and_grads(*b1, **d1)
    two.loss_and_grads(*b2, **d2)
    total, worst = _compare_grads(two.gradients(), want, "two accumulated two-clip micro-batches vs the mean of their gradients")
    assert total < 1e-3 and worst < 5e-3


def test_gradient_checkpointing_at_two_clips(nets):
    """Losses EQUAL, gradients within the floor of repeated plain steps (max(4 x floor, 1e-6)), for ``True`` and ``"all"``."""
    batch, draws = make_batch(2)
    res = {}
    for mode in (False, False, False, False, True, "all"):
        tr = trainer(nets, gradient_checkpointing=mode)
        r = tr.loss_and_grads(*batch, **draws)
        res.setdefault(mode, []).append((r, flat(tr)))
    plain = [f for _, f in res[False]]
    floor = max(rel(a, b) for i, a in enumerate(plain) for b in plain[:i])
    for mode in (True, "all"):
        r, f = res[mode][0]
        d = min(rel(f, p) for p in plain)
        print(f"B = 2, gradient_checkpointing={mode!r}: vs the nearest plain step {d:.3e}; floor of 4 plain steps {floor:.3e}")
        assert all(r[k] == res[False][0][0][k] for k in ("loss", "loss_temporal", "loss_spatial"))
        assert d <= max(4 * floor, 1e-6)


def test_deterministic_mode_at_two_clips(nets):
    """Two fresh trainers: bit-equal gradients and losses, bit-equal parameters after one optimizer step."""
    batch, draws = make_batch(2)
    runs = []
    for _ in range(2):
        tr = trainer(nets, deterministic=True, learning_rate=1e-4)
        r = tr.loss_and_grads(*batch, **draws)
        g = tr.params.grad.clone()
        assert tr.optimizer_step() is True
        runs.append((r, g, tr.params.flat.clone()))
    assert float(runs[0][1].abs().max()) > 0
    assert all(runs[0][0][k] == runs[1][0][k] for k in ("loss", "loss_temporal", "loss_spatial"))
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])


def test_ema_with_8bit_adam_takes_a_two_clip_step(nets):
    batch, draws = make_batch(2)
    tr = trainer(nets, use_ema=True, use_8bit_adam=True, learning_rate=1e-4)
    before = tr.params.flat.clone()
    out = tr.step(*batch, **draws)
    assert out["stepped"] is True and math.isfinite(out["loss"]) and math.isfinite(out["grad_norm"])
    assert not torch.equal(before, tr.params.flat) and tr.ema.optimization_step == 1


def test_captured_step_refuses_a_batch(nets):
    batch, draws = make_batch(2)
    tr = trainer(nets, use_graph=True)
    with pytest.raises(ValueError, match="use_graph.*one clip"):
        tr.loss_and_grads(*batch, **draws)


# ------------------------------------------------------------------------------------------------- one clip is untouched
def test_one_clip_never_reaches_the_batch_ops(nets, monkeypatch):
    """A one-clip step with the batch ops out of reach - the tape ops raise, and so does the library entry point - has the losses of
    the same step left alone."""
    from posetraj_amd import autodiff as AD, hip
    batch, draws = make_batch(1)
    plain = trainer(nets).loss_and_grads(*batch, **draws)

    def unreachable(*a, **kw):
        raise AssertionError("a batch op ran at B == 1")

    for name in ("add_rowvec_interleaved", "repeat_rows", "concat_rows"):
        monkeypatch.setattr(AD, name, unreachable)
    real = hip.checked()

    class Guard:
        def __getattr__(self, name):
            if name.startswith("ptb_"):
                raise AssertionError(f"{name} called at B == 1")
            return getattr(real, name)

    monkeypatch.setattr(hip, "checked", lambda: Guard())
    guarded = trainer(nets).loss_and_grads(*batch, **draws)
    assert all(guarded[k] == plain[k] for k in ("loss", "loss_temporal", "loss_spatial"))
