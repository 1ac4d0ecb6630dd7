"""Control window, per-step scale and spatial control weights of ``StableVideoDiffusionPipelineControlNet.denoise`` on the MI355X:
the accumulation kernel of include/posetraj_control.h exactly against fp32 tensor arithmetic, one weighted accumulation call against
the fused one, the loop's three kinds of step against an fp32 oracle loop written out below, and which steps launch the ControlNet.

Measured on the MI355X (profiles/r12/control_schedule.txt), rel-L2 of the latents after steps 0, 1, 2, 3 against the oracle loop:
  d0 (default path, existing code)   1.904e-05  5.971e-04  1.406e-03  1.404e-03    camera twin 1.950e-05  5.901e-04  1.443e-03  1.442e-03
  bound = min(1.5 d0, 2.2e-3)        2.857e-05  8.956e-04  2.109e-03  2.107e-03
  A  weight map                      2.514e-05  7.567e-04  1.912e-03  1.910e-03    oracle separation from its default run 1.012
  B  per-step scales                 2.347e-05  5.995e-04  1.602e-03  1.600e-03    0.292
  C  window (0.25, 0.75)             2.778e-05  5.826e-04  1.414e-03  1.413e-03    1.873e-02
  D  A + B + end 0.75                2.808e-05  7.909e-04  1.896e-03  1.894e-03    1.093
  D2 second weight map, same graphs  2.669e-05  6.553e-04  1.742e-03  1.741e-03    0.751
  E  A on the camera twin            2.549e-05  7.562e-04  1.910e-03  1.909e-03    1.015
Eager and (graph + two streams) agree bit for bit in every scenario, as for the default path.  One accumulation call: 13 of 13 tensors
on the ``torch.equal`` branch (same ``(cfg, splits)`` for the fused and the fp32-output zero-conv), 0 elements differ.

Scenario E runs on the TINY camera twin (``parity.build_oracle_nets(0, camera=True)``): ``parity.build_oracle_camera_controlnet`` is the
full-width ControlNet (0.68 B parameters), which pairs with no tiny U-Net and whose CPU oracle loop takes minutes, not seconds.
"""
import ctypes

import pytest
import torch

from tests import parity as P

pytestmark = pytest.mark.gpu
TOL_LOOP_FP32 = 2.2e-3          # the project's bound for one loop iteration against the fp32 oracle (tests/test_parity_ladder_gpu.py)
STEPS, FRAMES, HW = 4, 14, (8, 8)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return "cuda:0"


# ---------------------------------------------------------------------------------------------------------------- the kernel
W_VALUES = (0.0, 1.0, -0.5, -2.0, 1e-30, 1.5, 3.0, 0.37)


def _kernel_case(dev, rows, C, ldy, ldt, with_lo, scale, seed):
    """Padded buffers with live values everywhere (3 rows beyond ``rows``, the pitch padding): whatever the kernel must not touch is a
    canary.  Returns (t, w, y, y_lo, expected y buffer)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    R = rows + 3
    mag = 10.0 ** (torch.rand(R, ldt, generator=g, device=dev) * 6 - 3)          # |t| spread over 1e-3 .. 1e3
    t = torch.randn(R, ldt, generator=g, device=dev).clamp(-1, 1) * mag
    y = (torch.randn(R, ldy, generator=g, device=dev) * 4).half()                # fp16-representable
    y_lo = (torch.randn(R, ldy, generator=g, device=dev) * 2e-3).half() if with_lo else None
    w = torch.tensor(W_VALUES, device=dev)[torch.randint(0, len(W_VALUES), (R,), generator=g, device=dev)]
    k = w[:rows] * scale                                                         # one fp32 product (the scalar is taken to fp32)
    rs = y[:rows, :C].float() + y_lo[:rows, :C].float() if with_lo else y[:rows, :C].float()
    want = y.clone()
    want[:rows, :C] = (t[:rows, :C] * k[:, None] + rs).half()
    return t, w, y, y_lo, want


@pytest.mark.parametrize("C", [8, 64, 320, 1280])
@pytest.mark.parametrize("rows", [1, 37, 210, 4097])
def test_weighted_residual_add_equals_fp32_tensor_arithmetic_bit_for_bit(dev, rows, C):
    """``fp16(t * (scale * w)[:, None] + (y.float() + y_lo.float()))`` in that order, ``torch.equal`` over the WHOLE padded buffers: the
    pitch padding (c >= C) and the rows beyond ``rows`` keep their canaries, and ``t`` / ``w`` / ``y_lo`` are read only."""
    from posetraj_amd import hip, ops
    L, case = hip.checked(), 0
    for ldy in (C, C + 8):
        for ldt in (C, C + 16):
            for with_lo in (True, False):
                for scale in (1.0, 0.9, 1.4):
                    case += 1
                    t, w, y, y_lo, want = _kernel_case(dev, rows, C, ldy, ldt, with_lo, scale, seed=1000 * rows + C + case)
                    keep = [a.clone() for a in (t, w)] + ([y_lo.clone()] if with_lo else [])
                    L.ptc_weighted_residual_add_f16(t.data_ptr(), ldt, w.data_ptr(), scale, y.data_ptr(), None if y_lo is None else y_lo.data_ptr(),
                                                    ldy, rows, C, ops._stream())
                    torch.cuda.synchronize()
                    assert torch.equal(y, want), (rows, C, ldy, ldt, with_lo, scale, int((y != want).sum()))
                    assert all(torch.equal(a, b) for a, b in zip(keep, [t, w] + ([y_lo] if with_lo else [])))


def test_weighted_residual_add_wrapper_and_refusals(dev):
    """``ops.weighted_residual_add`` on a wide-stream tensor (reads the pair, counts the in-place write, refuses a stale pair), and the
    host-side ``PT_CHECK``s: returned status codes, nothing is launched."""
    from posetraj_amd import hip, ops
    t, w, y, y_lo, want = _kernel_case(dev, 37, 64, 64, 64, True, 0.9, seed=5)
    ops._attach_lo(y, y_lo)
    before = ops._inplace_writes.get(y.data_ptr(), 0)
    out = ops.weighted_residual_add(t, w, y, 0.9, rows=37)
    assert out is y and torch.equal(y, want) and ops._inplace_writes[y.data_ptr()] == before + 1
    with pytest.raises(RuntimeError, match="stale"):                              # the high half was rewritten: the pair is stale
        ops.weighted_residual_add(t, w, y, 0.9, rows=37)
    ops.drop_lo(y)
    with pytest.raises(RuntimeError, match="float32"):
        ops.weighted_residual_add(t.half(), w, y, 0.9)
    L, st = hip.lib(), ops._stream()
    t, w, y, _, _ = _kernel_case(dev, 8, 64, 72, 80, False, 1.0, seed=6)
    y0 = y.clone()
    bad = lambda *a: L.ptc_weighted_residual_add_f16(*a) != 0
    assert bad(t.data_ptr(), 80, w.data_ptr(), 1.0, y.data_ptr(), None, 72, 8, 12, st) and b"C %" in L.pt_last_error()          # C = 12
    assert bad(t.data_ptr(), 80, w.data_ptr(), 1.0, y.data_ptr(), None, 68, 8, 64, st) and b"pitch" in L.pt_last_error()        # odd pitch
    assert bad(t.data_ptr(), 76, w.data_ptr(), 1.0, y.data_ptr(), None, 72, 8, 64, st) and b"pitch" in L.pt_last_error()
    assert bad(t.data_ptr(), 80, w.data_ptr(), 1.0, y.data_ptr() + 2, None, 72, 8, 64, st) and b"aligned" in L.pt_last_error()  # misaligned
    assert bad(t.data_ptr() + 4, 80, w.data_ptr(), 1.0, y.data_ptr(), None, 72, 8, 64, st) and b"aligned" in L.pt_last_error()
    assert bad(t.data_ptr(), 80, None, 1.0, y.data_ptr(), None, 72, 8, 64, st) and b"null" in L.pt_last_error()                 # null w
    assert bad(t.data_ptr(), 80, w.data_ptr(), 1.0, y.data_ptr(), None, 72, 0, 64, st)
    assert bad(t.data_ptr(), 48, w.data_ptr(), 1.0, y.data_ptr(), None, 72, 8, 64, st)                                          # pitch < C
    torch.cuda.synchronize()
    assert torch.equal(y, y0)
    with pytest.raises(RuntimeError, match="ptc_weighted_residual_add_f16"):
        hip.checked().ptc_weighted_residual_add_f16(None, 80, None, 1.0, None, None, 72, 8, 64, st)


# ---------------------------------------------------------------------------------------------- one accumulation call
@pytest.fixture(scope="module")
def nets(dev):
    cn_o, unet_o = P.build_oracle_nets(seed=0)
    cn_h, unet_h = P.build_hip_nets(cn_o, unet_o, dev)
    return cn_o, unet_o, cn_h, unet_h


def _clone_wide(s):
    from posetraj_amd import ops
    c = s.clone()
    if getattr(s, "lo", None) is not None:
        ops._attach_lo(c, s.lo.clone())
    return c


def _fp16_ulp(v):
    """One fp16 unit in the last place at magnitude ``v`` (fp32 tensor): 2^(floor(log2 v) - 10), 2^-24 below the normal range."""
    _, e = torch.frexp(v.clamp_min(2.0 ** -14))                                   # v = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(v), e - 11)


def test_weighted_accumulation_with_unit_weights_equals_the_fused_epilogue(nets, dev, capsys):
    """``_accumulate_into_weighted`` with all-ones weights against ``_accumulate_into`` on cloned skips, scale 0.9: the same operations
    (fp32 zero-conv output, x scale, + the skip pair, one rounding).  Where ``pt_igemm_plan`` names the same (cfg, splits) for the
    fp32-output form and the fused form of a zero-conv the two tensors are EQUAL; where the plans differ the accumulators may differ in
    their summation order and the results are held to one fp16 ulp at max(|skip_in|, |a|, |b|)."""
    from posetraj_amd import hip, ops
    _, _, cn_h, unet_h = nets
    j = {k: v.to(dev) for k, v in P.tiny_inputs(seed=0).items()}
    args = (j["sample"].half(), j["t"], j["ehs"].half(), j["ids"])
    enc = unet_h._encode(*args)
    taps, xm = cn_h._features(*args, j["cond"].half(), None)
    mult = unet_h._multiplicity(enc, len(taps))
    skip_in = [s.float() + (s.lo.float() if getattr(s, "lo", None) is not None else 0) for s in enc["skips"] + [enc["x"]]]
    sk_a, mid_a = [_clone_wide(s) for s in enc["skips"]], _clone_wide(enc["x"])
    sk_b, mid_b = [_clone_wide(s) for s in enc["skips"]], _clone_wide(enc["x"])
    sizes = {tuple(t.shape[1:3]) for t in taps + [xm]}
    ones = {sz: torch.ones(taps[0].shape[0] * sz[0] * sz[1], dtype=torch.float32, device=dev) for sz in sizes}

    Cl, plans = hip.checked(), []
    orig = Cl.pt_igemm_f16

    def spy(pref, stream):                                                       # the plan of every igemm launch, asked of the library itself
        cfg, sp = ctypes.c_int32(), ctypes.c_int32()
        hip.check(hip.lib().pt_igemm_plan(pref, ctypes.byref(cfg), ctypes.byref(sp), None), "pt_igemm_plan")
        plans.append((cfg.value, sp.value))
        return orig(pref, stream)

    Cl.pt_igemm_f16 = spy
    try:
        cn_h._accumulate_into(taps, xm, 0.9, sk_a, mult, mid_a)
        n_fused = len(plans)
        cn_h._accumulate_into_weighted(taps, xm, 0.9, ones, sk_b, mult, mid_b)
    finally:
        Cl.pt_igemm_f16 = orig
    torch.cuda.synchronize()
    assert n_fused == 13 and len(plans) == 26 and all(mult)
    equal = ulp = 0
    for i, (a, b, s0) in enumerate(zip(sk_a + [mid_a], sk_b + [mid_b], skip_in)):
        assert getattr(a, "lo", None) is None and getattr(b, "lo", None) is None          # both paths leave plain fp16
        same_plan = plans[i] == plans[13 + i]
        ndiff = int((a != b).sum())
        with capsys.disabled():
            print(f"\n  tensor {i:2d} {tuple(a.shape)}: fused plan {plans[i]}, fp32-output plan {plans[13 + i]} -> "
                  f"{'torch.equal' if same_plan else 'one fp16 ulp'} branch, {ndiff} of {a.numel()} elements differ", end="")
        if same_plan:
            equal += 1
            assert torch.equal(a, b), (i, ndiff)
        else:
            ulp += 1
            bound = _fp16_ulp(torch.maximum(s0.abs(), torch.maximum(a.float().abs(), b.float().abs())))
            assert bool(((a.float() - b.float()).abs() <= bound).all()), i
        assert not torch.equal(a.float(), s0)                                             # the residual did move the skip
    with capsys.disabled():
        print(f"\n  plan branches: {equal} torch.equal, {ulp} one-ulp")
    assert equal + ulp == 13


# --------------------------------------------------------------------------------------------- the loop against the fp32 oracle
def oracle_denoise(cn, unet, sched, *, latents, image_latents, image_embeddings, controlnet_condition, scales, weight=None, on=None,
                   camera_cond=None, min_guidance_scale=1.0, max_guidance_scale=3.0):
    """``oracle/loop.py: denoise`` with a ``conditioning_scale`` per step, the residuals multiplied by the pooled ``weight`` ``[F, h, w]``
    (both CFG halves alike) and replaced by zeros on off steps.  Returns the latents after every step."""
    from oracle import loop as OL
    sched.set_timesteps(len(scales))
    nf = latents.shape[1]
    g = OL.guidance_ramp(min_guidance_scale, max_guidance_scale, nf, latents.shape[0], latents.dtype, latents.ndim)
    ids = OL.hot_added_time_ids(image_embeddings.dtype)
    rec = []
    with torch.no_grad():
        for i, t in enumerate(sched.timesteps):
            x = sched.scale_model_input(torch.cat([latents] * 2), t)
            x = torch.cat([x, image_latents], dim=2)
            kw = dict(camera_cond=camera_cond) if camera_cond is not None else {}
            down, mid = cn(x, t, encoder_hidden_states=image_embeddings, controlnet_cond=controlnet_condition, added_time_ids=ids,
                           conditioning_scale=scales[i], guess_mode=False, return_dict=False, **kw)
            res = list(down) + [mid]
            if weight is not None:
                res = [r * torch.nn.functional.adaptive_avg_pool2d(weight, r.shape[-2:]).repeat(2, 1, 1).unsqueeze(1) for r in res]
            if on is not None and not on[i]:
                res = [torch.zeros_like(r) for r in res]
            pred = unet(x, t, encoder_hidden_states=image_embeddings, down_block_additional_residuals=res[:-1],
                        mid_block_additional_residual=res[-1], added_time_ids=ids, return_dict=False)[0]
            un, co = pred.chunk(2)
            latents = sched.step(un + g * (co - un), t, latents).prev_sample
            rec.append(latents.clone())
    return rec


def weight_map_a():
    w = torch.ones(FRAMES, *HW)
    w[:, :, HW[1] // 2:] = 0.0
    w[7:] *= 0.25
    return w


WINDOW_ON = [False, True, True, False]                                            # (0.25, 0.75) at N = 4
# scenario -> (pipeline arguments, oracle arguments)
SCENARIOS = {
    "default": (dict(controlnet_cond_scale=0.9), dict(scales=[0.9] * 4)),
    "A": (dict(controlnet_cond_scale=0.9, control_weight=weight_map_a()), dict(scales=[0.9] * 4, weight=weight_map_a())),
    "B": (dict(controlnet_cond_scale=[0.3, 0.9, 0.5, 0.9]), dict(scales=[0.3, 0.9, 0.5, 0.9])),
    "C": (dict(controlnet_cond_scale=0.9, control_guidance_start=0.25, control_guidance_end=0.75), dict(scales=[0.9] * 4, on=WINDOW_ON)),
    "D": (dict(controlnet_cond_scale=[0.3, 0.9, 0.5, 0.9], control_weight=weight_map_a(), control_guidance_end=0.75),
          dict(scales=[0.3, 0.9, 0.5, 0.9], weight=weight_map_a(), on=[True, True, True, False])),
}
_w9 = torch.rand(FRAMES, *HW, generator=torch.Generator().manual_seed(9))
SCENARIOS["D2"] = (dict(SCENARIOS["D"][0], control_weight=_w9), dict(SCENARIOS["D"][1], weight=_w9))


class Bench:
    """Nets, inputs, pipeline and the cached oracle / HIP runs of one (tiny) network pair."""

    def __init__(self, dev, camera):
        from posetraj_amd import EulerDiscreteScheduler, StableVideoDiffusionPipelineControlNet, SVD_SCHEDULER_CONFIG
        from oracle import sched as OS
        self.dev, self.camera = dev, camera
        self.cn_o, self.unet_o = P.build_oracle_nets(0, camera)
        self.cn_h, self.unet_h = P.build_hip_nets(self.cn_o, self.unet_o, dev, camera)
        lat, self.il, self.emb, self.cond = P.loop_inputs(0, FRAMES, *HW, self.unet_o.config.cross_attention_dim)
        self.cam = P.loop_camera_input(0, FRAMES) if camera else None
        self.new_sched = lambda: OS.OracleEulerDiscreteScheduler(**OS.SVD_SCHEDULER_CONFIG)
        so = self.new_sched()
        so.set_timesteps(STEPS)
        self.lat0 = lat * so.init_noise_sigma
        self.new_pipe = lambda: StableVideoDiffusionPipelineControlNet(unet=self.unet_h, controlnet=self.cn_h,
                                                                       scheduler=EulerDiscreteScheduler(**SVD_SCHEDULER_CONFIG))
        self.pipe = self.new_pipe()
        self._oracle, self._hip = {}, {}

    def oracle(self, name):
        if name not in self._oracle:
            self._oracle[name] = oracle_denoise(self.cn_o, self.unet_o, self.new_sched(), latents=self.lat0,
                                                image_latents=self.il.unsqueeze(1).repeat(1, FRAMES, 1, 1, 1), image_embeddings=self.emb,
                                                controlnet_condition=self.cond, camera_cond=self.cam, **SCENARIOS[name][1])
        return self._oracle[name]

    def run(self, name, graph, pipe=None):
        """The latents after every step of the HIP loop (``callback_on_step_end``)."""
        rec, d = [], self.dev
        kw = {k: (v.to(d) if torch.is_tensor(v) else v) for k, v in SCENARIOS[name][0].items()}
        out = (pipe or self.pipe).denoise(self.lat0.to(d), self.il.to(d), self.emb.to(d), self.cond.to(d), num_inference_steps=STEPS,
                                          camera_cond=None if self.cam is None else self.cam.to(d), use_graph=graph, overlap_streams=graph,
                                          callback_on_step_end=lambda p_, i, t, k: rec.append(k["latents"].clone()) or {}, **kw)
        torch.cuda.synchronize()
        assert len(rec) == STEPS and torch.equal(rec[-1], out)
        return [r.cpu() for r in rec]

    def hip(self, name, graph):
        if (name, graph) not in self._hip:
            self._hip[(name, graph)] = self.run(name, graph)
        return self._hip[(name, graph)]

    def bound(self):
        """1.5 x d0[step], d0 = the default path's own distance from the oracle's default run on these nets and inputs (existing code:
        the same value on the parent commit), and never above TOL_LOOP_FP32 for steps 0 - 2."""
        d0 = [P.rel_l2(a, b) for a, b in zip(self.hip("default", False), self.oracle("default"))]
        return d0, [min(1.5 * d, TOL_LOOP_FP32) if i < STEPS - 1 else 1.5 * d for i, d in enumerate(d0)]


@pytest.fixture(scope="module")
def bench(dev):
    return Bench(dev, camera=False)


@pytest.fixture(scope="module")
def bench_cam(dev):
    return Bench(dev, camera=True)


def test_oracle_loop_restates_the_projects_oracle(bench):
    """With scale 0.9 and no extras the loop above is ``oracle/loop.py: denoise``: distance 0."""
    from oracle import loop as OL
    rec = []
    ref = OL.denoise(bench.cn_o, bench.unet_o, bench.new_sched(), latents=bench.lat0,
                     image_latents=bench.il.unsqueeze(1).repeat(1, FRAMES, 1, 1, 1), image_embeddings=bench.emb,
                     controlnet_condition=bench.cond, num_inference_steps=STEPS, controlnet_cond_scale=0.9, record=rec)
    mine = bench.oracle("default")
    assert torch.equal(ref, mine[-1]) and all(torch.equal(a, b) for a, b in zip(rec, mine))


def _check_scenario(b, name, capsys, hip_runs=None):
    d0, bound = b.bound()
    ora, base = b.oracle(name), b.oracle("default")
    sep = P.rel_l2(ora[-2], base[-2]), P.rel_l2(ora[-1], base[-1])
    # told apart from a run that ignored the argument: the oracle's own result lies 4 bounds away from its default run
    assert sep[1] >= 4 * max(bound), (name, sep, bound)
    default_bitwise = all(torch.equal(a, c) for a, c in zip(b.hip("default", False), b.hip("default", True)))
    runs = hip_runs or {g: b.hip(name, g) for g in (False, True)}
    dist = {g: [P.rel_l2(a, o) for a, o in zip(runs[g], ora)] for g in runs}
    with capsys.disabled():
        print(f"\n  {name}{' (camera)' if b.camera else ''}: d0 = {['%.3e' % v for v in d0]}, bound = {['%.3e' % v for v in bound]}, "
              f"oracle separation from default (step {STEPS - 2}, {STEPS - 1}) = {sep[0]:.3e}, {sep[1]:.3e}", end="")
        for g in dist:
            print(f"\n    {'graph + two streams' if g else 'eager'}: {['%.3e' % v for v in dist[g]]}", end="")
        print(f"\n    default path graph == eager bit for bit: {default_bitwise}")
    for g in dist:
        for i in range(STEPS):
            assert dist[g][i] <= bound[i], (name, g, i, dist[g][i], bound[i])
    if default_bitwise and len(runs) == 2:
        assert all(torch.equal(a, c) for a, c in zip(runs[False], runs[True])), name


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_loop_scenarios_match_the_oracle_after_every_step(bench, name, capsys):
    """A: weight map (right half zero, frames 7.. at a quarter); B: per-step scales; C: window (0.25, 0.75).  Eager, and as replayed
    graphs with the two encoders on two streams; the latents after EVERY step against the oracle's."""
    _check_scenario(bench, name, capsys)


def test_loop_weight_scales_and_window_together_reuse_their_graphs_for_another_weight_map(bench, capsys):
    """D = A + B + ``control_guidance_end = 0.75``, twice on ONE pipeline object; the second run has another weight map (``torch.rand``,
    seed 9).  It must replay the graphs the first run captured - no new capture - and still match its own oracle: weights baked
    into a graph would reproduce the first run."""
    pipe = bench.new_pipe()
    first = {False: bench.run("D", False, pipe), True: bench.run("D", True, pipe)}
    states = {k: pipe._step_graphs.get(k) for k in pipe._step_graphs}
    graphs = {k: s.graph for k, s in states.items()}
    assert sorted(k.kind for k in states) == ["off", "weighted"] and pipe._step_graphs.of_kind("plain") is None
    assert pipe._step_graphs.of_kind("off").graph.pool() == pipe._step_graphs.of_kind("weighted").graph.pool()
    _check_scenario(bench, "D", capsys, first)
    second = {False: bench.run("D2", False, pipe), True: bench.run("D2", True, pipe)}
    assert set(pipe._step_graphs) == set(states)
    assert all(pipe._step_graphs.get(k) is states[k] and states[k].graph is graphs[k] for k in states)
    _check_scenario(bench, "D2", capsys, second)
    assert P.rel_l2(bench.oracle("D2")[-1], bench.oracle("D")[-1]) >= 4 * max(bench.bound()[1])       # the two maps are told apart


def test_loop_weight_map_on_the_camera_twin(bench_cam, capsys):
    """E: scenario A through the camera ControlNet (``camera_cond`` reaches the condition encoder; the weighted graph owns its camera
    buffer like the plain one)."""
    _check_scenario(bench_cam, "A", capsys)


# ------------------------------------------------------------------------------------------------------------- launch count
def test_steps_outside_the_window_do_not_launch_the_controlnet(bench):
    """Eager mode, counters around the ControlNet's three entry points: N = 4 with windows (0, 1), (0, 0.5), (0.25, 0.75), (0.1, 0.15)
    and scales [0.9, 0, 0.9, 0] evaluates the ControlNet 4, 2, 2, 0 and 2 times, off steps accumulate nothing, and the (0, 1) call is
    the call without the new arguments: plain steps only, equal output."""
    pipe, cn, d = bench.new_pipe(), bench.cn_h, bench.dev
    calls = dict(features=0, plain=0, weighted=0)
    orig = cn._features, cn._accumulate_into, cn._accumulate_into_weighted

    def counted(name, fn):
        def f(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return f

    cn._features, cn._accumulate_into, cn._accumulate_into_weighted = (counted(n, f) for n, f in zip(calls, orig))
    try:
        def run(**kw):
            for k in calls:
                calls[k] = 0
            out = pipe.denoise(bench.lat0.to(d), bench.il.to(d), bench.emb.to(d), bench.cond.to(d), num_inference_steps=STEPS, **kw)
            torch.cuda.synchronize()
            return out, dict(calls)
        base, n = run(controlnet_cond_scale=0.9)
        assert n == dict(features=4, plain=4, weighted=0)
        out, n = run(controlnet_cond_scale=0.9, control_guidance_start=0.0, control_guidance_end=1.0)
        assert n == dict(features=4, plain=4, weighted=0) and torch.equal(out, base)
        for (s, e), want in (((0.0, 0.5), 2), ((0.25, 0.75), 2), ((0.1, 0.15), 0)):
            out, n = run(controlnet_cond_scale=0.9, control_guidance_start=s, control_guidance_end=e)
            assert n == dict(features=want, plain=want, weighted=0), ((s, e), n)
            assert not torch.equal(out, base)
        out, n = run(controlnet_cond_scale=[0.9, 0, 0.9, 0])
        assert n == dict(features=2, plain=0, weighted=2), n
        out, n = run(controlnet_cond_scale=0.9, control_weight=torch.ones(FRAMES, *HW))
        assert n == dict(features=4, plain=0, weighted=4), n
    finally:
        for k in ("_features", "_accumulate_into", "_accumulate_into_weighted"):
            del cn.__dict__[k]
    assert len(pipe._step_graphs) == 0


def test_new_arguments_reach_call_and_the_camera_pipeline(bench_cam):
    """``__call__`` of the base and of the camera pipeline (``**kw``) hand the three arguments to ``denoise``: the result equals the
    direct ``denoise`` call's, a bad argument is a ``ValueError`` before any stage runs."""
    from posetraj_amd import EulerDiscreteScheduler, SVD_SCHEDULER_CONFIG
    from posetraj_amd.pipeline_stable_video_diffusion_controlnet_cam import StableVideoDiffusionPipelineControlNet as CamPipe
    b, d = bench_cam, bench_cam.dev
    pipe = CamPipe(unet=b.unet_h, controlnet=b.cn_h, scheduler=EulerDiscreteScheduler(**SVD_SCHEDULER_CONFIG))
    lat = torch.randn(1, FRAMES, 4, *HW, generator=torch.Generator().manual_seed(3))
    kw = dict(controlnet_cond_scale=[0.3, 0.9, 0.5, 0.9], control_weight=weight_map_a(), control_guidance_end=0.75)
    common = dict(height=8 * HW[0], width=8 * HW[1], num_frames=FRAMES, num_inference_steps=STEPS, latents=lat, output_type="latent",
                  image_embeddings=b.emb.to(d), image_latents=b.il.to(d), return_dict=False, use_graph=False, overlap_streams=False)
    got = pipe(None, b.cond[0], b.cam[0].tolist(), **common, **kw)
    pipe.scheduler.set_timesteps(STEPS, device=d)
    want = pipe.denoise(pipe.prepare_latents(1, FRAMES, 8, 8 * HW[0], 8 * HW[1], torch.float32, d, None, lat), b.il.to(d), b.emb.to(d),
                        b.cond.to(d), num_inference_steps=STEPS, camera_cond=b.cam.to(d), **kw)
    plain = pipe(None, b.cond[0], b.cam[0].tolist(), **common, controlnet_cond_scale=0.9)
    assert torch.equal(got, want) and not torch.equal(got, plain)
    with pytest.raises(ValueError, match="control_guidance_end"):
        pipe(None, b.cond[0], b.cam[0].tolist(), **common, control_guidance_end=1.5)
    with pytest.raises(ValueError, match="control_weight"):
        pipe(None, b.cond[0], b.cam[0].tolist(), **common, control_weight=torch.ones(FRAMES, 4, 4))
