"""``--use_ema`` on the device: the two EMA kernels against torch's own fp32 statements, the fused AdamW + EMA pass against the
plain fused AdamW pass, and ``ControlNetTrainer(use_ema=True)`` - three steps, one of them skipped - against a CPU replay of
diffusers' ``EMAModel`` (restated below), the validation swap and checkpoint resume.

Every comparison is ``torch.equal``: both sides perform the same IEEE fp32 operations in the same order (``d = s - p``,
``t = omd * d``, ``s = s - t``: three roundings - a build that contracts the last two into a fused multiply-add fails here)."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GRID = 16384 * 256 * 4                      # elements one sweep of the element-wise grid covers: beyond it the grid-stride loop iterates


class RestatedEMA:
    """diffusers 0.24.0 ``training_utils.EMAModel`` (constructor, ``get_decay``, ``step``), restated from memory, over a list of tensors."""

    def __init__(self, parameters, decay=0.9999, min_decay=0.0, update_after_step=0, use_ema_warmup=False, inv_gamma=1.0, power=2 / 3):
        self.shadow_params = [p.clone().detach() for p in parameters]
        self.decay, self.min_decay, self.update_after_step = decay, min_decay, update_after_step
        self.use_ema_warmup, self.inv_gamma, self.power = use_ema_warmup, inv_gamma, power
        self.optimization_step, self.cur_decay_value = 0, None

    def get_decay(self, optimization_step):
        step = max(0, optimization_step - self.update_after_step - 1)
        if step <= 0:
            return 0.0
        if self.use_ema_warmup:
            cur_decay_value = 1 - (1 + step / self.inv_gamma) ** -self.power
        else:
            cur_decay_value = (1 + step) / (10 + step)
        cur_decay_value = min(cur_decay_value, self.decay)
        return max(cur_decay_value, self.min_decay)

    @torch.no_grad()
    def step(self, parameters):
        self.optimization_step += 1
        decay = self.get_decay(self.optimization_step)
        self.cur_decay_value = decay
        one_minus_decay = 1 - decay
        for s_param, param in zip(self.shadow_params, parameters):
            s_param.sub_(one_minus_decay * (s_param - param))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _wide(n, seed):
    """fp32 values of both signs over 24 decades (normal numbers, nothing near overflow) and a few exact zeros; two calls with different
    seeds give unrelated magnitudes element by element: differences that absorb the smaller operand, products that round."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g) * torch.pow(10.0, torch.rand(n, generator=g) * 24 - 12)
    x[::1009] = 0.0
    return x


@pytest.mark.parametrize("n", [4 * 262147, GRID + 4 * 333])
def test_ema_update_kernel_equals_the_three_torch_operations(dev, n):
    from posetraj_amd import hip, ops
    L, st = hip.lib(), ops._stream()
    s0, p = _wide(n, 1), _wide(n, 2)
    p[5::64] = s0[5::64]                                      # shadow == parameter: stays put exactly
    p[6::64] = s0[6::64] * (1 + 2.0 ** -20)                   # nearly equal: the difference is a few ulps
    pd = p.to(dev)
    omds = [1.0, 1.0 - 0.9999, 9 / 11] if n < GRID else [1.0 - 0.9999]
    for omd in omds:
        want = s0.clone()
        want.sub_(omd * (want - p))
        sd = s0.to(dev)
        hip.check(L.pt_ema_update_f32(sd.data_ptr(), pd.data_ptr(), n, omd, st), "pt_ema_update_f32")
        got = sd.cpu()
        assert torch.isfinite(want).all()
        assert torch.equal(got, want), (omd, int((got != want).sum()), n)
        assert torch.equal(pd.cpu(), p)                       # the parameters are read only
    # the checks of pt_adamw_fused_f32: n a multiple of 4, 16-byte aligned buffers
    assert L.pt_ema_update_f32(sd.data_ptr(), pd.data_ptr(), n - 2, 0.5, st) != 0 and b"multiple of 4" in L.pt_last_error()
    assert L.pt_ema_update_f32(sd.data_ptr() + 4, pd.data_ptr(), n - 4, 0.5, st) != 0 and b"aligned" in L.pt_last_error()


@pytest.mark.parametrize("n", [4 * 262147, GRID + 4 * 333])
def test_adamw_ema_equals_fused_adamw_then_ema_update(dev, n):
    """``pt_adamw_ema_f32`` vs ``pt_adamw_fused_f32`` on copies of the same buffers: parameters, moments, fp16 mirror and the zeroed
    gradient bit-identical; the shadow = ``pt_ema_update_f32`` (itself pinned to torch above) applied with the NEW parameters."""
    from posetraj_amd import hip, ops
    L, st = hip.lib(), ops._stream()
    g = torch.Generator().manual_seed(7)
    p0 = torch.randn(n, generator=g).to(dev)
    gr0 = (torch.randn(n, generator=g) * 25.0).to(dev)        # loss-scaled gradients (inv_scale below)
    m0 = (torch.randn(n, generator=g) * 0.1).to(dev)
    v0 = (torch.rand(n, generator=g) * 0.01).to(dev)
    s0 = _wide(n, 3).to(dev)
    s0[: n // 2] = p0[: n // 2] * 1.001                       # half of the shadow near the parameters, as in training
    adam = (n, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 3, 1 / 256.0)
    omd = 9 / 11
    a = [t.clone() for t in (p0, gr0, m0, v0)]
    ha = torch.zeros(n, dtype=torch.float16, device=dev)
    hip.check(L.pt_adamw_fused_f32(*(t.data_ptr() for t in a), *adam, ha.data_ptr(), 1, st), "pt_adamw_fused_f32")
    sa = s0.clone()
    hip.check(L.pt_ema_update_f32(sa.data_ptr(), a[0].data_ptr(), n, omd, st), "pt_ema_update_f32")
    b = [t.clone() for t in (p0, gr0, m0, v0)]
    hb = torch.zeros(n, dtype=torch.float16, device=dev)
    sb = s0.clone()
    hip.check(L.pt_adamw_ema_f32(*(t.data_ptr() for t in b), *adam, hb.data_ptr(), 1, sb.data_ptr(), omd, st), "pt_adamw_ema_f32")
    for name, x, y in zip(("p", "g", "m", "v"), a, b):
        assert torch.equal(x, y), name
    assert torch.equal(ha, hb) and float(b[1].abs().max()) == 0.0 and not torch.equal(b[0], p0)
    assert torch.equal(sa, sb), int((sa != sb).sum())
    if n < GRID:                                              # without the mirror and without zeroing: the gradient survives, the shadow is the same
        c = [t.clone() for t in (p0, gr0, m0, v0)]
        sc = s0.clone()
        hip.check(L.pt_adamw_ema_f32(*(t.data_ptr() for t in c), *adam, None, 0, sc.data_ptr(), omd, st), "pt_adamw_ema_f32")
        assert torch.equal(c[0], a[0]) and torch.equal(c[1], gr0) and torch.equal(sc, sa)
        assert L.pt_adamw_ema_f32(*(t.data_ptr() for t in c), *adam, None, 0, None, omd, st) != 0 and b"ema_shadow" in L.pt_last_error()


# ------------------------------------------------------------------------------------------------- the trainer
EMA_KW = dict(use_ema=True)                                   # the defaults: decay 0 on the first step, 2/11 on the second, 3/12 on the third


@pytest.fixture(scope="module")
def run(dev, golden, tmp_path_factory):
    """Three ``step()``s of one EMA trainer on the tiny networks and the ``train_grads`` inputs of tests/test_backward_gpu.py: normal,
    forced to skip (``optimizer_step(grad_norm=inf)``: nothing overflows on the device), normal.  The state after the second is saved."""
    from posetraj_amd.training import ControlNetTrainer
    from tests.test_backward_gpu import _nets
    g = golden("train_grads")
    cn_o, un_o, un, cfg = _nets(dev)
    t = lambda n: torch.from_numpy(g[n])
    draws = dict(noise=t("noise"), sigmas=t("sigmas"), random_p=t("random_p"), ran_idx=int(g["ran_idx"]))
    batch = (t("latents"), t("emb"), torch.tensor([127.0]), t("traj"))
    sd0 = {k: v.clone() for k, v in cn_o.state_dict().items()}
    kw = dict(learning_rate=2e-4, conditioning_dropout_prob=0.1, loss_scale=4096.0)
    tr = ControlNetTrainer(cfg, sd0, un, **kw, **EMA_KW)
    snaps = [{k: v.cpu() for k, v in tr.state_dict().items()}]
    stepped = []
    ck = str(tmp_path_factory.mktemp("ema") / "checkpoint-2")
    for i in range(3):
        if i == 1:
            tr.loss_and_grads(*batch, **draws)
            stepped.append(tr.optimizer_step(grad_norm=float("inf")))
        else:
            stepped.append(tr.step(*batch, **draws)["stepped"])
        snaps.append({k: v.cpu() for k, v in tr.state_dict().items()})
        if i == 1:
            tr.save_state(ck)
            saved = dict(shadow={k: v.cpu() for k, v in tr.ema_state_dict().items()}, scalars=tr.ema.scalars(), cur=tr.ema.cur_decay_value,
                         steps=(tr.optimizer_steps, tr.skipped_steps, tr.loss_scale))
    ema = {k: v.cpu() for k, v in tr.ema_state_dict().items()}
    return dict(tr=tr, snaps=snaps, stepped=stepped, ema=ema, ck=ck, saved=saved, nets=(un, cfg, sd0, kw), batch=batch, draws=draws)


def test_trainer_ema_equals_a_cpu_replay_of_emamodel(run):
    tr, snaps = run["tr"], run["snaps"]
    names = list(snaps[0])
    ref = RestatedEMA([snaps[0][k] for k in names])
    for snap in snaps[1:]:
        ref.step([snap[k] for k in names])
    assert run["stepped"] == [True, False, True]
    assert all(torch.equal(snaps[1][k], snaps[2][k]) for k in names)                                # the skipped step left the parameters alone
    assert any(not torch.equal(snaps[0][k], snaps[1][k]) for k in names) and any(not torch.equal(snaps[2][k], snaps[3][k]) for k in names)
    assert tr.ema.optimization_step == 3 == ref.optimization_step and tr.ema.cur_decay_value == ref.cur_decay_value == 3 / 12
    assert (tr.optimizer_steps, tr.skipped_steps) == (2, 1)
    assert set(run["ema"]) == set(names)
    for k, want in zip(names, ref.shadow_params):
        got = run["ema"][k]
        assert got.dtype == torch.float32 and got.shape == want.shape and torch.equal(got, want), k
    assert any(not torch.equal(run["ema"][k], snaps[3][k]) for k in names)                         # an average, not a copy of the parameters


def test_separate_launches_give_the_same_shadow_and_ema_off_allocates_nothing(run, dev):
    """``ema_fused = False`` (AdamW, then the EMA launch): the same three steps' shadow is the replay of ITS snapshots too; a trainer
    without EMA has no ``ema`` and no fifth buffer."""
    from posetraj_amd.training import ControlNetTrainer
    un, cfg, sd0, kw = run["nets"]
    before = torch.cuda.memory_allocated()
    off = ControlNetTrainer(cfg, sd0, un, **kw)
    grown_off = torch.cuda.memory_allocated() - before
    assert off.ema is None
    with pytest.raises(RuntimeError, match="use_ema"):
        off.ema_state_dict()
    before = torch.cuda.memory_allocated()
    sep = ControlNetTrainer(cfg, sd0, un, **kw, **EMA_KW)
    grown_on = torch.cuda.memory_allocated() - before
    assert sep.ema.shadow.numel() == sep.params.numel and sep.ema.shadow.dtype == torch.float32
    assert 0 <= (grown_on - grown_off) - 4 * sep.params.numel < (1 << 21)                            # exactly one more fp32 buffer (allocator rounding)
    sep.ema_fused = False
    names = sep.params.names
    ref = RestatedEMA([v.cpu() for v in sep.state_dict().values()])
    for i in range(2):
        if i == 1:
            sep.loss_and_grads(*run["batch"], **run["draws"])
            assert sep.optimizer_step(grad_norm=float("inf")) is False
        else:
            assert sep.step(*run["batch"], **run["draws"])["stepped"] is True
        now = sep.state_dict()
        ref.step([now[k].cpu() for k in names])
    got = sep.ema_state_dict()
    assert sep.ema.optimization_step == 2 and all(torch.equal(got[k].cpu(), want) for k, want in zip(names, ref.shadow_params))


def test_validation_swap_store_copy_to_restore(run):
    tr = run["tr"]
    P = tr.params
    master, shadow = P.flat.clone(), {k: v.clone() for k, v in tr.ema_state_dict().items()}
    v0 = P.version
    tr.ema.store()
    tr.ema.copy_to()
    assert P.version > v0
    now = tr.state_dict()
    for k in shadow:
        assert torch.equal(now[k], shadow[k]), k
        assert torch.equal(P.half_view(k), shadow[k].half()), k
    v1 = P.version
    tr.ema.restore()
    assert P.version > v1 and torch.equal(P.flat, master) and tr.ema.temp_stored is None
    assert all(torch.equal(tr.ema_state_dict()[k], shadow[k]) for k in shadow)                       # the swap never touches the shadow
    k = next(k for k in shadow if len(P.shapes[k]) == 1)
    assert torch.equal(P.half_view(k), P.value(k).half())


def test_resume_restores_shadow_and_counters(run, dev):
    from posetraj_amd import ControlNetSDVModel
    from posetraj_amd.training import ControlNetTrainer
    un, cfg, sd0, kw = run["nets"]
    ck, saved = run["ck"], run["saved"]
    assert sorted(os.listdir(ck)) == ["controlnet", "controlnet_ema", "optimizer.safetensors", "trainer_state.json"]
    b = ControlNetTrainer(cfg, sd0, un, **kw, **EMA_KW)
    state = b.load_state(ck)
    got = b.ema_state_dict()
    for k, want in saved["shadow"].items():
        assert torch.equal(got[k].cpu(), want), k
    assert b.ema.scalars() == saved["scalars"] and b.ema.optimization_step == 2 and b.ema.cur_decay_value == saved["cur"] == 2 / 11
    assert (b.optimizer_steps, b.skipped_steps, b.loss_scale) == saved["steps"] == (1, 1, 2048.0) and state["ema"]["optimization_step"] == 2
    params = b.state_dict()
    for k, v in run["snaps"][2].items():
        assert torch.equal(params[k].cpu(), v), k
    m = ControlNetSDVModel.from_pretrained(ck, subfolder="controlnet_ema", device=dev, keep_source=True)
    msd = m.state_dict()
    assert set(msd) == set(saved["shadow"])
    for k, want in saved["shadow"].items():
        assert torch.equal(msd[k].cpu(), want.half()), k
    off = ControlNetTrainer(cfg, sd0, un, **kw)               # without the flag the folder is ignored
    off.load_state(ck)
    assert off.ema is None and off.optimizer_steps == 1
