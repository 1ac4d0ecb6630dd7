"""DPM-Solver++(2M) on the MI355X: the two step kernels of include/posetraj_sampler.h exactly against fp32 tensor arithmetic,
``DPMPP2MDiscreteScheduler.step`` against the fp64 recurrence, the denoise loop after every step against an fp32 oracle loop written out
below, the solver's convergence on the HIP path, and the wiring (which kernel a scheduler takes, one captured graph for both).

The loop's bound per step is 1.25 x the storage model ``m_i``: the rel-L2 between the oracle loop below under
``oracle.quant.storage("fp16-fused")`` (the tensors the HIP path keeps in fp16) and under ``"fp32"`` - the project's rule for a loop
iteration.  The CPU oracle gives m = 1.92e-5, 1.11e-3, 2.67e-3, 2.67e-3 for 2M (Euler on the same inputs: 1.92e-5, 5.99e-4, 1.52e-3,
1.52e-3; the larger 2M figures are the solver's |b| + |c| ~ 2.8 at the late steps).  Measured on the MI355X, eager and graph + two
streams alike: 1.90e-5, 1.09e-3, 2.72e-3, 2.72e-3; 2M@25 / Euler@25 against Euler@200: 0.558 (profiles/r14/sampler_steps.txt).
"""
import math

import pytest
import torch

from tests import parity as P

pytestmark = pytest.mark.gpu
STEPS, FRAMES, HW, SCALE = 4, 14, (8, 8), 0.9
GUARD = 64                                                    # floats of canary on either side of every buffer a kernel writes


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return "cuda:0"


def r32(v):
    """The fp32 value a C ``float`` parameter receives."""
    return torch.tensor(float(v), dtype=torch.float32).item()


def _coef_sets(with_prev):
    """Step scalars as the scheduler produces them (25-step SVD table: sigma = 700 .. 0.002) and one arbitrary set, rounded to fp32."""
    from posetraj_amd import DPMPP2MDiscreteScheduler, SVD_SCHEDULER_CONFIG
    s = DPMPP2MDiscreteScheduler(**SVD_SCHEDULER_CONFIG)
    s.set_timesteps(25)
    sets = [s.coefficients(12), s.coefficients(23), (0.3, -1.7, 0.25, 1.9, -0.45)] if with_prev else \
           [s.coefficients(0), s.coefficients(24), (0.3, -1.7, 0.25, 1.9, 0.0)]
    assert all((c[4] != 0.0) == with_prev for c in sets)
    return [tuple(r32(v) for v in c) for c in sets]


def _guarded(n, dev, fill):
    """A contiguous fp32 buffer of ``n`` elements inside a larger one whose margins are canaries -> (whole, view)."""
    whole = torch.full((n + 2 * GUARD,), 12345.0, dtype=torch.float32, device=dev)
    view = whole[GUARD:GUARD + n]
    view.copy_(fill.reshape(-1))
    return whole, view


def _guards_intact(whole):
    return bool((whole[:GUARD] == 12345.0).all()) and bool((whole[-GUARD:] == 12345.0).all())


def _update(mo, x, dp, coefs):
    """The header's arithmetic in its stated order with torch ``mul`` / ``add`` only (one fp32 rounding each, no fused multiply-add)."""
    c_skip, c_out, a, b, c = coefs
    D = torch.add(torch.mul(mo, c_out), torch.mul(x, c_skip))
    xn = torch.add(torch.mul(x, a), torch.mul(D, b))
    if c != 0.0:
        xn = torch.add(xn, torch.mul(dp, c))
    return D, xn


# ----------------------------------------------------------------------------------------------------- pts_cfg_multistep_step
def _cfg_case(dev, Bc, F, h, w, ldn, f32, coefs, seed):
    from posetraj_amd import ops
    g = torch.Generator(device=dev).manual_seed(seed)
    with_prev = coefs[4] != 0.0
    pred = torch.randn(2 * Bc, F, h, w, ldn, generator=g, device=dev)
    pred[..., 4:] = float("nan")                               # channels >= 4: never read (a read shows as NaN), never written
    pred = pred if f32 else pred.half()
    guid = (1.0 + 2.0 * torch.rand(Bc, F, generator=g, device=dev)).contiguous()           # differs per clip and frame
    x0 = torch.randn(Bc, F, 4, h, w, generator=g, device=dev) * 50.0
    dp0 = torch.randn(Bc, F, 4, h, w, generator=g, device=dev) if with_prev else torch.full((Bc, F, 4, h, w), float("nan"), device=dev)
    pred_in, guid_in = pred.clone(), guid.clone()
    xw, x = _guarded(x0.numel(), dev, x0)
    dw, dp = _guarded(dp0.numel(), dev, dp0)
    ops.cfg_multistep_step(pred, guid, coefs, x.view(Bc, F, 4, h, w), dp.view(Bc, F, 4, h, w))
    torch.cuda.synchronize()
    pu, pc = pred_in[:Bc, ..., :4].float(), pred_in[Bc:, ..., :4].float()
    mo = torch.add(pu, torch.mul(torch.sub(pc, pu), guid_in[:, :, None, None, None]))
    if not f32:
        mo = mo.half().float()
    D, xn = _update(mo.permute(0, 1, 4, 2, 3).contiguous(), x0, dp0, coefs)
    where = (Bc, F, h, w, ldn, f32, coefs)
    assert torch.equal(x.view_as(xn), xn) and torch.equal(dp.view_as(D), D), where
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(dp).all()), where
    assert _guards_intact(xw) and _guards_intact(dw), where
    assert torch.equal(pred.view(torch.int16 if not f32 else torch.int32), pred_in.view(torch.int16 if not f32 else torch.int32)), where   # NaN canaries: bitwise
    assert torch.equal(guid, guid_in), where


@pytest.mark.parametrize("with_prev", [False, True], ids=["c=0,history=NaN", "c!=0"])
@pytest.mark.parametrize("ldn", [4, 8])
@pytest.mark.parametrize("f32", [True, False], ids=["fp32", "fp16"])
def test_cfg_multistep_step_equals_fp32_tensor_arithmetic(dev, f32, ldn, with_prev):
    """Every (Bc, F, h, w) of {1, 2} x {1, 14} x {(1, 1), (3, 5), (8, 8), (33, 7)}; with ``c == 0`` the history buffer holds NaN and
    must not be read."""
    seed = 0
    for coefs in _coef_sets(with_prev):
        for Bc in (1, 2):
            for F in (1, 14):
                for h, w in ((1, 1), (3, 5), (8, 8), (33, 7)):
                    seed += 1
                    _cfg_case(dev, Bc, F, h, w, ldn, f32, coefs, seed)


@pytest.mark.parametrize("f32", [True, False], ids=["fp32", "fp16"])
def test_cfg_multistep_step_beyond_one_pass_of_the_grid_and_on_unaligned_predictions(dev, f32):
    """2 x 14 x 192 x 200 pixels are more than the 4096 x 256 threads of one pass: the grid-stride loop runs twice for some threads.
    ``ldn = 6`` and a prediction that starts 4 bytes (fp32) / 2 bytes (fp16) off a vector boundary take the per-channel loads."""
    from posetraj_amd import hip, ops
    for with_prev in (False, True):
        _cfg_case(dev, 2, 14, 192, 200, 4, f32, _coef_sets(with_prev)[0], 77 + with_prev)
        _cfg_case(dev, 2, 3, 5, 7, 6, f32, _coef_sets(with_prev)[2], 79 + with_prev)
    Bc, F, h, w, ldn = 1, 2, 3, 5, 8
    coefs = _coef_sets(True)[2]
    g = torch.Generator(device=dev).manual_seed(5)
    flat = torch.randn(2 * Bc * F * h * w * ldn + 1, generator=g, device=dev)
    flat = flat if f32 else flat.half()
    pred = flat[1:].view(2 * Bc, F, h, w, ldn)                                             # off by one element
    guid = 1.0 + 2.0 * torch.rand(Bc, F, generator=g, device=dev)
    x0, dp0 = torch.randn(Bc, F, 4, h, w, generator=g, device=dev), torch.randn(Bc, F, 4, h, w, generator=g, device=dev)
    x, dp = x0.clone(), dp0.clone()
    hip.checked().pts_cfg_multistep_step(pred.data_ptr(), 1 if f32 else 0, ldn, guid.data_ptr(), *coefs, Bc, F, h, w, x.data_ptr(), dp.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    pu, pc = pred[:Bc, ..., :4].float(), pred[Bc:, ..., :4].float()
    mo = torch.add(pu, torch.mul(torch.sub(pc, pu), guid[:, :, None, None, None]))
    mo = mo if f32 else mo.half().float()
    D, xn = _update(mo.permute(0, 1, 4, 2, 3).contiguous(), x0, dp0, coefs)
    assert torch.equal(x, xn) and torch.equal(dp, D)


# ---------------------------------------------------------------------------------------------------------- pts_multistep_step
@pytest.mark.parametrize("n", [1, 7, 4096, 3 * 10 ** 6 + 5])
@pytest.mark.parametrize("f32", [True, False], ids=["fp32", "fp16"])
def test_multistep_step_equals_fp32_tensor_arithmetic(dev, f32, n):
    """Flat tensors, ``prev_sample`` aliasing ``sample`` and not, ``c == 0`` over a NaN history and ``c != 0``, 16-byte aligned buffers
    (vector accesses + the n % 4 tail) and buffers one float off (element accesses)."""
    from posetraj_amd import hip
    L, st = hip.checked(), torch.cuda.current_stream().cuda_stream
    seed = 0
    for with_prev in (False, True):
        for coefs in _coef_sets(with_prev)[::2]:
            for aliased in (False, True):
                for off in (0, 1):
                    seed += 1
                    g = torch.Generator(device=dev).manual_seed(seed)
                    mo = torch.randn(n + off, generator=g, device=dev)
                    mo = (mo if f32 else mo.half())[off:]
                    x0 = torch.randn(n, generator=g, device=dev) * 50.0
                    dp0 = torch.randn(n, generator=g, device=dev) if with_prev else torch.full((n,), float("nan"), device=dev)
                    xw, x = _guarded(n + off, dev, torch.cat([torch.zeros(off, device=dev), x0]))
                    dw, dp = _guarded(n + off, dev, torch.cat([torch.zeros(off, device=dev), dp0]))
                    ow, out = (xw, x) if aliased else _guarded(n + off, dev, torch.zeros(n + off, device=dev))
                    mo_in = mo.clone()
                    L.pts_multistep_step(mo.data_ptr(), 1 if f32 else 0, x[off:].data_ptr(), *coefs, dp[off:].data_ptr(), out[off:].data_ptr(), n, st)
                    torch.cuda.synchronize()
                    D, xn = _update(mo_in.float(), x0, dp0, coefs)
                    where = (n, f32, coefs, aliased, off)
                    assert torch.equal(out[off:], xn) and torch.equal(dp[off:], D), where
                    assert bool(torch.isfinite(out[off:]).all()), where
                    assert aliased or torch.equal(x[off:], x0), where
                    assert _guards_intact(xw) and _guards_intact(dw) and _guards_intact(ow), where
                    assert bool((out[:off] == 0).all()) and bool((dp[:off] == 0).all()) and torch.equal(mo, mo_in), where


# ------------------------------------------------------------------------------------------------------------- scheduler.step
def test_scheduler_step_follows_the_fp64_recurrence_and_resets_its_history(dev):
    """Six steps on a random fp32 ``model_output`` sequence.  After every step the returned sample is compared with the recurrence in
    fp64 - fp64 coefficients, fed with the fp32 sample and history the device held before that step - within the running error bound
    of the kernel's 8 roundings (each at most 2^-24 relative to its own result, carried through at most |b| times):
    ``16 2^-24 (|a x| + |b D| + |c Dp| + |b mo c_out| + |b x c_skip|)`` per element.  The coefficients reach the kernel as fp32
    (2^-24 relative each, inside the same bound's slack of 2).  ``set_timesteps`` and ``_step_index = None`` start a new run."""
    from posetraj_amd import DPMPP2MDiscreteScheduler, SVD_SCHEDULER_CONFIG
    N, shape = 6, (1, 14, 4, 9, 7)
    s = DPMPP2MDiscreteScheduler(**SVD_SCHEDULER_CONFIG)
    s.set_timesteps(N, device=dev)
    g = torch.Generator(device=dev).manual_seed(11)
    mos = [torch.randn(shape, generator=g, device=dev) for _ in range(N)]
    x = torch.randn(shape, generator=g, device=dev) * float(s.init_noise_sigma)
    x_start, firsts = x.clone(), []
    assert s._denoised_prev is None
    for i, t in enumerate(s.timesteps):
        hist = None if s._denoised_prev is None else s._denoised_prev.clone()
        assert (hist is None) == (i == 0)
        c_skip, c_out, a, b, c = s.coefficients(i)
        x64, mo64, dp64 = x.double(), mos[i].double(), torch.zeros_like(x, dtype=torch.float64) if hist is None else hist.double()
        D64 = mo64 * c_out + x64 * c_skip
        want = a * x64 + b * D64 + c * dp64
        bound = 16 * 2.0 ** -24 * ((a * x64).abs() + (b * D64).abs() + (c * dp64).abs() + (b * mo64 * c_out).abs() + (b * x64 * c_skip).abs())
        out = s.step(mos[i], t, x)
        x_new = out.prev_sample
        assert x_new.dtype == torch.float32 and out.pred_original_sample is None and s.step_index == i + 1
        err = (x_new.double() - want).abs()
        assert bool((err <= bound).all()), (i, float((err / bound.clamp_min(1e-300)).max()))
        assert bool(((s._denoised_prev.double() - D64).abs() <= 4 * 2.0 ** -24 * ((mo64 * c_out).abs() + (x64 * c_skip).abs())).all()), i
        firsts.append(x_new.clone())
        x = x_new
    assert bool(torch.isfinite(x).all())
    with pytest.raises(ValueError, match="shape"):                                         # another shape in the middle of a run
        s._step_index = 2
        s.step(mos[2][:, :7], s.timesteps[2], firsts[1][:, :7])
    s.set_timesteps(N, device=dev)                                                          # a new run: the first step is the Euler step again
    assert s._denoised_prev is None and s._step_index is None
    again = s.step(mos[0], s.timesteps[0], x_start, return_dict=False)[0]
    assert torch.equal(again, firsts[0])
    second = s.step(mos[1], s.timesteps[1], again, return_dict=False)[0]
    assert torch.equal(second, firsts[1])
    s._step_index = None                                                                    # ... and so does a cleared step index
    assert torch.equal(s.step(mos[0], s.timesteps[0], x_start, return_dict=False)[0], firsts[0])
    h16 = DPMPP2MDiscreteScheduler(**SVD_SCHEDULER_CONFIG)                                  # an fp16 model output comes back as fp16
    h16.set_timesteps(N, device=dev)
    assert h16.step(mos[0].half(), h16.timesteps[0], x_start.half()).prev_sample.dtype == torch.float16


# --------------------------------------------------------------------------------------------- the loop against the fp32 oracle
def oracle_denoise(cn, unet, sched, solver, *, latents, image_latents, image_embeddings, controlnet_condition, steps, scale, camera_cond=None):
    """``oracle/loop.py: denoise`` (same body, same ``q`` marks) returning the latents after every step; ``solver`` "euler" takes the
    oracle scheduler's step, "2m" the update of k-diffusion's ``sample_dpmpp_2m`` in its own form - ``t = -ln sigma``,
    ``h = t' - t``, ``r = h_last / h``, ``x' = (sigma'/sigma) x - expm1(-h) ((1 + 1/(2r)) D - D_prev / (2r))``, the first step without
    a history and the step to sigma' = 0 returning D - in fp32 tensors."""
    from oracle import loop as OL
    from oracle.quant import q
    sched.set_timesteps(steps)
    sig = [float(v) for v in sched.sigmas]
    g = OL.guidance_ramp(1.0, 3.0, latents.shape[1], latents.shape[0], latents.dtype, latents.ndim)
    ids = OL.hot_added_time_ids(image_embeddings.dtype)
    rec, d_prev = [], None
    with torch.no_grad():
        for i, t in enumerate(sched.timesteps):
            x = q(sched.scale_model_input(torch.cat([latents] * 2), t))
            x = torch.cat([x, image_latents], dim=2)
            kw = dict(camera_cond=camera_cond) if camera_cond is not None else {}
            down, mid = cn(x, t, encoder_hidden_states=image_embeddings, controlnet_cond=controlnet_condition, added_time_ids=ids,
                           conditioning_scale=scale, guess_mode=False, return_dict=False, **kw)
            pred = unet(x, t, encoder_hidden_states=image_embeddings, down_block_additional_residuals=down,
                        mid_block_additional_residual=mid, added_time_ids=ids, return_dict=False)[0]
            un, co = pred.chunk(2)
            mo = q(un + g * (co - un))
            if solver == "euler":
                latents = q(sched.step(mo, t, latents).prev_sample)
            else:
                s, s_next = sig[i], sig[i + 1]
                D = mo * (-s / (s * s + 1) ** 0.5) + latents / (s * s + 1)
                if s_next == 0.0:
                    latents = D
                else:
                    h = math.log(s) - math.log(s_next)
                    if d_prev is None:
                        dd = D
                    else:
                        r = (math.log(sig[i - 1]) - math.log(s)) / h
                        dd = (1 + 1 / (2 * r)) * D - (1 / (2 * r)) * d_prev
                    latents = (s_next / s) * latents - math.expm1(-h) * dd
                latents, d_prev = q(latents), D
                sched._step_index += 1
            rec.append(latents.clone())
    return rec


class Rig:
    """Nets, inputs, pipelines and the cached oracle / HIP runs of one (tiny) network pair."""

    def __init__(self, dev, camera):
        from posetraj_amd import DPMPP2MDiscreteScheduler, EulerDiscreteScheduler, SVD_SCHEDULER_CONFIG
        from posetraj_amd import StableVideoDiffusionPipelineControlNet as BasePipe
        from posetraj_amd.pipeline_stable_video_diffusion_controlnet_cam import StableVideoDiffusionPipelineControlNet as CamPipe
        from oracle import sched as OS
        self.dev, self.camera = dev, camera
        self.cn_o, self.unet_o = P.build_oracle_nets(0, camera)
        self.cn_h, self.unet_h = P.build_hip_nets(self.cn_o, self.unet_o, dev, camera)
        lat, self.il, self.emb, self.cond = P.loop_inputs(0, FRAMES, *HW, self.unet_o.config.cross_attention_dim)
        self.cam = P.loop_camera_input(0, FRAMES) if camera else None
        self.new_osched = lambda: OS.OracleEulerDiscreteScheduler(**OS.SVD_SCHEDULER_CONFIG)
        so = self.new_osched()
        so.set_timesteps(STEPS)
        self.lat0 = lat * so.init_noise_sigma                                               # sigma_max = 700 at every step count
        self.schedulers = dict(euler=lambda: EulerDiscreteScheduler(**SVD_SCHEDULER_CONFIG), dpmpp2m=lambda: DPMPP2MDiscreteScheduler(**SVD_SCHEDULER_CONFIG))
        self.new_pipe = lambda sampler: (CamPipe if camera else BasePipe)(unet=self.unet_h, controlnet=self.cn_h, scheduler=self.schedulers[sampler]())
        self.pipes = {}
        self._oracle, self._hip = {}, {}

    def pipe(self, sampler):
        if sampler not in self.pipes:
            self.pipes[sampler] = self.new_pipe(sampler)
        return self.pipes[sampler]

    def oracle(self, solver, mode="fp32"):
        from oracle import quant as OQ
        if (solver, mode) not in self._oracle:
            with OQ.storage(mode):
                self._oracle[(solver, mode)] = oracle_denoise(
                    self.cn_o, self.unet_o, self.new_osched(), solver, latents=self.lat0, image_latents=self.il.unsqueeze(1).repeat(1, FRAMES, 1, 1, 1),
                    image_embeddings=self.emb, controlnet_condition=self.cond, steps=STEPS, scale=SCALE, camera_cond=self.cam)
        return self._oracle[(solver, mode)]

    def denoise(self, pipe, steps, graph, scale=SCALE, callback=None):
        d = self.dev
        out = pipe.denoise(self.lat0.to(d), self.il.to(d), self.emb.to(d), self.cond.to(d), num_inference_steps=steps, controlnet_cond_scale=scale,
                           camera_cond=None if self.cam is None else self.cam.to(d), use_graph=graph, overlap_streams=graph,
                           callback_on_step_end=callback)
        torch.cuda.synchronize()
        return out

    def hip(self, sampler, graph):
        """The latents after every step of the HIP loop (``callback_on_step_end``)."""
        if (sampler, graph) not in self._hip:
            rec = []
            out = self.denoise(self.pipe(sampler), STEPS, graph, callback=lambda p_, i, t, k: rec.append(k["latents"].clone()) or {})
            assert len(rec) == STEPS and torch.equal(rec[-1], out)
            self._hip[(sampler, graph)] = [r.cpu() for r in rec]
        return self._hip[(sampler, graph)]


@pytest.fixture(scope="module")
def rig(dev):
    return Rig(dev, camera=False)


@pytest.fixture(scope="module")
def rig_cam(dev):
    return Rig(dev, camera=True)


def test_loop_matches_the_oracle_after_every_step(rig, capsys):
    """N = 4, scale 0.9, 14 frames, 8 x 8 latent.  Bound per step: 1.25 x the storage model m_i (module docstring).  A run that
    ignored the scheduler would fail: the oracle's 2M latents lie >= 4 bounds from the oracle's Euler latents at steps 2 and 3.  Eager
    and (graph + two streams) agree bit for bit."""
    ora, fused, euler = rig.oracle("2m"), rig.oracle("2m", "fp16-fused"), rig.oracle("euler")
    m = [P.rel_l2(a, b) for a, b in zip(fused, ora)]
    bound = [1.25 * v for v in m]
    sep = [P.rel_l2(a, b) for a, b in zip(ora, euler)]
    runs = {g: rig.hip("dpmpp2m", g) for g in (False, True)}
    dist = {g: [P.rel_l2(a, o) for a, o in zip(runs[g], ora)] for g in runs}
    d_euler = [P.rel_l2(a, o) for a, o in zip(rig.hip("euler", True), euler)]
    fmt = lambda vs: " ".join("%.3e" % v for v in vs)
    with capsys.disabled():
        print(f"\n  DPM-Solver++(2M), rel-L2 of the latents after steps 0..{STEPS - 1} against the fp32 oracle loop"
              f"\n    storage model m (fp16-fused | fp32)   {fmt(m)}\n    bound = 1.25 m                        {fmt(bound)}"
              f"\n    HIP eager                             {fmt(dist[False])}\n    HIP graph + two streams               {fmt(dist[True])}"
              f"\n    oracle 2M | oracle Euler              {fmt(sep)}\n    HIP Euler | oracle Euler (graph)      {fmt(d_euler)}")
    # the first step IS the Euler step, in another fp32 operation order: x ~ 700 goes to ~ 70, a few roundings of 2^-24 x 700 / 70 each
    assert sep[0] <= 1e-5, sep
    assert sep[2] >= 4 * bound[2] and sep[3] >= 4 * bound[3], (sep, bound)
    for g in dist:
        for i in range(STEPS):
            assert dist[g][i] <= bound[i], (g, i, dist[g][i], bound[i])
    assert all(torch.equal(a, b) for a, b in zip(runs[False], runs[True]))
    assert P.rel_l2(rig.hip("dpmpp2m", True)[0], rig.hip("euler", True)[0]) <= 1e-5            # ... on the device too


def test_two_m_at_25_steps_is_closer_to_the_converged_run_than_euler_at_25(rig, capsys):
    """Reference: the existing Euler loop at 200 steps, captured graph, same inputs, scale 1.0.  The CPU oracle gives 5.46e-2 for 2M and
    9.78e-2 for Euler (ratio 0.56); fp16 noise is 2e-3."""
    ref = rig.denoise(rig.pipe("euler"), 200, True, scale=1.0)
    e25 = rig.denoise(rig.pipe("euler"), 25, True, scale=1.0)
    m25 = rig.denoise(rig.pipe("dpmpp2m"), 25, True, scale=1.0)
    d_e, d_m = P.rel_l2(e25, ref), P.rel_l2(m25, ref)
    with capsys.disabled():
        print(f"\n  distance to Euler@200 (HIP, graph): Euler@25 {d_e:.3e}, 2M@25 {d_m:.3e}, ratio {d_m / d_e:.3f}")
    assert bool(torch.isfinite(m25).all())
    assert d_m <= 0.75 * d_e, (d_m, d_e)


# --------------------------------------------------------------------------------------------------------------------- wiring
def _count_step_kernels(monkeypatch):
    from posetraj_amd import ops
    calls = dict(euler=0, multistep=0, args=[])
    euler, multi = ops.cfg_euler_step, ops.cfg_multistep_step

    def count_euler(*a, **k):
        calls["euler"] += 1
        return euler(*a, **k)

    def count_multi(pred, guidance, coefs, x, d_prev):
        calls["multistep"] += 1
        calls["args"].append((coefs, x, d_prev, x.clone()))
        return multi(pred, guidance, coefs, x, d_prev)

    monkeypatch.setattr(ops, "cfg_euler_step", count_euler)
    monkeypatch.setattr(ops, "cfg_multistep_step", count_multi)
    return calls


def test_the_scheduler_picks_the_step_kernel_and_both_share_one_graph(rig, monkeypatch):
    """Euler scheduler: ``ops.cfg_euler_step`` N times, ``ops.cfg_multistep_step`` never; the new scheduler: the reverse, the first
    step with ``c == 0``, every step with the same history tensor.  Swapping the scheduler on ONE pipeline object replays the graph
    that was captured before: no new capture."""
    from posetraj_amd import DPMPP2MDiscreteScheduler
    calls = _count_step_kernels(monkeypatch)
    pipe = rig.new_pipe("euler")
    for graph in (False, True):
        calls.update(euler=0, multistep=0)
        e = rig.denoise(pipe, STEPS, graph)
        assert (calls["euler"], calls["multistep"]) == (STEPS, 0)
    state, graph_obj = pipe._step_graphs.of_kind("plain"), pipe._step_graphs.of_kind("plain").graph
    euler_config = pipe.scheduler.config
    pipe.scheduler = DPMPP2MDiscreteScheduler.from_config(pipe.scheduler.config)
    assert pipe.scheduler.config == euler_config
    for graph in (True, False):
        calls.update(euler=0, multistep=0, args=[])
        m = rig.denoise(pipe, STEPS, graph)
        assert (calls["euler"], calls["multistep"]) == (0, STEPS)
        cs = [a[0][4] for a in calls["args"]]
        assert cs[0] == 0.0 and all(c < 0.0 for c in cs[1:-1]) and cs[-1] == 0.0 and calls["args"][-1][0][2:] == (0.0, 1.0, 0.0)
        assert all(a[2] is calls["args"][0][2] for a in calls["args"]) and calls["args"][0][2].shape == calls["args"][0][1].shape
        assert torch.equal(m.cpu(), rig.hip("dpmpp2m", graph)[-1])
    assert pipe._step_graphs.of_kind("plain") is state and state.graph is graph_obj and len(pipe._step_graphs) == 1
    assert torch.equal(e.cpu(), rig.hip("euler", True)[-1]) and not torch.equal(e, m)


def test_one_step_returns_the_denoised_estimate(rig, monkeypatch):
    """``num_inference_steps = 1`` is one step to sigma' = 0: coefficients (0, 1, 0), the latents ARE the denoised estimate (0 x + 1 D
    is exact).  The Euler step to zero computes the same value by cancelling the 700-scale sample, x - ((x - D) / sigma) sigma: three
    roundings of up to 2^-24 x 700 = 4.2e-5 each on values of order 1, hence the 1e-3."""
    calls = _count_step_kernels(monkeypatch)
    m = rig.denoise(rig.new_pipe("dpmpp2m"), 1, False)
    e = rig.denoise(rig.new_pipe("euler"), 1, False)
    (coefs, x, d_prev, _), = calls["args"]
    assert coefs[2:] == (0.0, 1.0, 0.0) and torch.equal(m, d_prev) and bool(torch.isfinite(m).all())
    assert P.rel_l2(m, e) <= 1e-3


def test_the_control_window_and_weights_work_with_the_new_scheduler(rig):
    """Orthogonal features: a control window, per-step scales and a weight map run through the same loop; the first step of each run
    equals the Euler scheduler's (c = 0) and the later ones do not."""
    d = rig.dev
    w = torch.ones(FRAMES, *HW)
    w[:, :, HW[1] // 2:] = 0.0
    kw = dict(controlnet_cond_scale=[0.3, 0.9, 0.5, 0.9], control_weight=w.to(d), control_guidance_end=0.75)
    recs = {}
    for sampler in ("euler", "dpmpp2m"):
        rec = recs.setdefault(sampler, [])
        rig.new_pipe(sampler).denoise(rig.lat0.to(d), rig.il.to(d), rig.emb.to(d), rig.cond.to(d), num_inference_steps=STEPS, use_graph=True,
                                      overlap_streams=True, callback_on_step_end=lambda p_, i, t, k, rec=rec: rec.append(k["latents"].clone()) or {}, **kw)
        torch.cuda.synchronize()
    assert P.rel_l2(recs["dpmpp2m"][0], recs["euler"][0]) <= 1e-5 and P.rel_l2(recs["dpmpp2m"][-1], recs["euler"][-1]) > 1e-2
    assert all(bool(torch.isfinite(r).all()) for r in recs["dpmpp2m"])
    assert not torch.equal(recs["dpmpp2m"][-1].cpu(), rig.hip("dpmpp2m", True)[-1])


def test_callback_latents_replace_the_sample_and_the_history_stays(rig, monkeypatch):
    """Latents handed back by ``callback_on_step_end`` are what the next step starts from; the previous estimate is kept.  A callback
    that hands back an unchanged copy reproduces the run without a callback bit for bit."""
    calls = _count_step_kernels(monkeypatch)
    pipe = rig.new_pipe("dpmpp2m")
    same = rig.denoise(pipe, STEPS, False, callback=lambda p_, i, t, k: {"latents": k["latents"].clone()})
    assert torch.equal(same.cpu(), rig.hip("dpmpp2m", False)[-1])
    calls.update(args=[])
    edited = {}

    def edit(p_, i, t, k):
        if i == 1:
            edited["x"] = k["latents"] * 0.5 + 0.25
            return {"latents": edited["x"]}
        return {}

    out = rig.denoise(pipe, STEPS, False, callback=edit)
    args = calls["args"]
    assert torch.equal(args[2][3], edited["x"]) and args[2][2] is args[1][2] and args[2][0][4] < 0.0      # step 2: edited sample, same history, c != 0
    assert not torch.equal(out.cpu(), rig.hip("dpmpp2m", False)[-1]) and bool(torch.isfinite(out).all())


@pytest.mark.parametrize("camera", [False, True], ids=["base", "camera"])
def test_call_reaches_the_new_scheduler(rig, rig_cam, camera):
    """``__call__(output_type="latent")`` of the base and of the camera pipeline needs nothing beyond the scheduler object: it equals
    the direct ``denoise`` call and differs from the Euler scheduler's result."""
    b = rig_cam if camera else rig
    d = b.dev
    lat = torch.randn(1, FRAMES, 4, *HW, generator=torch.Generator().manual_seed(3))
    common = dict(height=8 * HW[0], width=8 * HW[1], num_frames=FRAMES, num_inference_steps=STEPS, latents=lat, output_type="latent",
                  image_embeddings=b.emb.to(d), image_latents=b.il.to(d), return_dict=False, use_graph=False, overlap_streams=False,
                  controlnet_cond_scale=SCALE)
    positional = (None, b.cond[0], b.cam[0].tolist()) if camera else (None, b.cond[0])
    got, plain = (b.new_pipe(s)(*positional, **common) for s in ("dpmpp2m", "euler"))
    pipe = b.new_pipe("dpmpp2m")
    pipe.scheduler.set_timesteps(STEPS, device=d)
    want = pipe.denoise(pipe.prepare_latents(1, FRAMES, 8, 8 * HW[0], 8 * HW[1], torch.float32, d, None, lat), b.il.to(d), b.emb.to(d),
                        b.cond.to(d), num_inference_steps=STEPS, controlnet_cond_scale=SCALE, camera_cond=None if b.cam is None else b.cam.to(d))
    torch.cuda.synchronize()
    assert torch.equal(got, want) and not torch.equal(got, plain) and bool(torch.isfinite(got).all())
