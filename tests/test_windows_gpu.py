"""Overlapping frame windows on the MI355X: the two kernels of include/posetraj_window.h bit for bit against the existing prologue and
against fp32 tensor arithmetic, one window against the plain loop, the windowed loop against an fp32 oracle loop with the windowing
written out below, ``window_batch``, and ``__call__`` end to end.

The loop's bound (rel-L2 of the final latents against the oracle loop) is ``TW.LOOP_BOUND`` = 1e-3; where a run does not meet it, the
rule is 1.25 x the distance of an independent 2-clip batch of the same two windows from its own oracle, measured in the test on the
same request (``Rig.batch_distance``).

Measured on the MI355X (profiles/r19/windows.txt), Ft = 7, Fw = 4, s = 3, 3 steps; eager and graph + two streams alike, window_batch 1
and 2 alike (bit for bit):
  scenario, sampler        windowed | oracle   independent 2-clip batch | its oracle   bound = 1.25 x   windowed | native 7-frame call
  plain, Euler             1.654e-03           1.641e-03                               2.052e-03        3.042e-01
  plain, 2M                3.861e-03           4.091e-03                               5.114e-03        3.118e-01
  weighted + off, Euler    1.690e-03           1.699e-03                               2.124e-03        3.452e-01
  weighted + off, 2M       4.225e-03           4.037e-03                               5.046e-03        3.763e-01
1e-3 does not hold for this 3-step loop, and does not for the existing batch on the same request either: the second rule applies.
"""
import ctypes
import math

import pytest
import torch

from tests import parity as P
from tests import windows as TW

pytestmark = pytest.mark.gpu
GUARD = 64                                                    # elements of canary on either side of every buffer a kernel writes
SHAPES = ((3, 5), (8, 8))
FT, FW, STRIDE, HW, STEPS, SCALE = 7, 4, 3, (8, 8), 3, 0.9


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return "cuda:0"


def _guarded(shape, dev, dtype, fill, canary):
    """A contiguous tensor of ``shape`` inside a larger buffer whose margins hold ``canary`` -> (whole, view)."""
    n = math.prod(shape)
    whole = torch.full((n + 2 * GUARD,), canary, dtype=dtype, device=dev)
    view = whole[GUARD:GUARD + n].view(shape)
    if fill is not None:
        view.copy_(fill)
    return whole, view


def _margins(whole, canary):
    m = torch.cat([whole[:GUARD], whole[-GUARD:]])
    return bool(torch.isnan(m).all()) if canary != canary else bool((m == canary).all())


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


NAN = float("nan")


# ---------------------------------------------------------------------------------------------------------- the prologue
@pytest.mark.parametrize("case,starts", TW.PLAN_CASES, ids=[str(c) for c, _ in TW.PLAN_CASES])
def test_window_rows_equal_the_existing_prologue_on_the_windows_frames_bit_for_bit(dev, case, starts):
    """Rows k and K + k of the output against ``ops.scale_concat_input`` of frames ``starts[k] .. + Fw``; the inputs sit between NaN
    margins (a read beyond them shows), the output between sentinels."""
    from posetraj_amd import ops, windows as W
    Ft, Fw, s = case
    assert list(W.window_plan(Ft, Fw, s).starts) == starts
    K = len(starts)
    g = torch.Generator(device=dev).manual_seed(Ft * 10 + Fw)
    for h, w in SHAPES:
        xw, x = _guarded((1, Ft, 4, h, w), dev, torch.float32, torch.randn(1, Ft, 4, h, w, generator=g, device=dev) * 40.0, NAN)
        iw, il = _guarded((2, 4, h, w), dev, torch.float16, torch.randn(2, 4, h, w, generator=g, device=dev).half(), NAN)
        x_in, il_in = x.clone(), il.clone()
        for sigma in (700.0, 1.5, 0.002):
            ow, out = _guarded((2 * K, Fw, h, w, 8), dev, torch.float16, None, 777.0)
            got = W.scale_concat_windows(x, il, sigma, starts, Fw, out=out)
            torch.cuda.synchronize()
            assert got.data_ptr() == out.data_ptr() and _margins(ow, 777.0) and bool(torch.isfinite(out).all())
            for k, st in enumerate(starts):
                want = ops.scale_concat_input(x_in[:, st:st + Fw].contiguous(), il_in, sigma)                   # [2, Fw, h, w, 8]
                assert torch.equal(_bits(out[k]), _bits(want[0])) and torch.equal(_bits(out[K + k]), _bits(want[1])), (case, (h, w), sigma, k)
            fresh = W.scale_concat_windows(x[0], il, sigma, starts, Fw)                                         # [Ft, 4, h, w] form, own output
            assert torch.equal(_bits(fresh), _bits(out))
        assert torch.equal(_bits(x), _bits(x_in)) and torch.equal(_bits(il), _bits(il_in)) and _margins(xw, NAN) and _margins(iw, NAN)


def test_a_group_of_windows_is_a_plan_of_its_own(dev):
    """``WindowStaging``: group g of the (9, 4, 2) plan, 2 windows per group, equals the rows of those windows in the whole plan's output."""
    from posetraj_amd import windows as W
    plan = W.window_plan(9, 4, 2)
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(1, 9, 4, 3, 5, generator=g, device=dev)
    il = torch.randn(2, 4, 3, 5, generator=g, device=dev).half()
    whole = W.scale_concat_windows(x, il, 1.5, plan.starts, 4)
    st = W.WindowStaging(plan, 2)
    assert st.input_shape(3, 5) == (4, 4, 3, 5, 8)
    for gi in range(2):
        st.select(gi)
        part = st.stage(x, il, 1.5)
        rows = [gi * 2, gi * 2 + 1, 4 + gi * 2, 4 + gi * 2 + 1]
        assert torch.equal(_bits(part), _bits(whole[rows]))


# ---------------------------------------------------------------------------------------------------------- the epilogue
def _merge_case(dev, case, starts, h, w, ldn, f32, seed, integer=False):
    from posetraj_amd import windows as W
    Ft, Fw, s = case
    K = len(starts)
    g = torch.Generator(device=dev).manual_seed(seed)
    if integer:                                              # every product and sum exact: an indexing fault cannot hide behind rounding
        pred = torch.randint(-8, 9, (2 * K, Fw, h, w, ldn), generator=g, device=dev).float()
        guid = torch.randint(1, 4, (Fw,), generator=g, device=dev).float()
        cover = TW.covering(Ft, Fw, starts)
        wts = torch.ones(K, Fw)
        for f, ks in enumerate(cover):
            assert len(ks) <= 2
            if len(ks) == 2:
                wts[ks[0], f - starts[ks[0]]], wts[ks[1], f - starts[ks[1]]] = 0.25, 0.75
        wts = wts.to(dev)
    else:
        pred = torch.randn(2 * K, Fw, h, w, ldn, generator=g, device=dev) * 3.0
        guid = (1.0 + 2.0 * torch.rand(Fw, generator=g, device=dev)).contiguous()
        wts = torch.from_numpy(W.window_plan(Ft, Fw, s).weights).to(dev)
    pred[..., 4:] = NAN                                      # channels >= 4: never read (a read shows as NaN)
    pw, pred = _guarded(tuple(pred.shape), dev, torch.float32 if f32 else torch.float16, pred if f32 else pred.half(), NAN)
    gw, guid = _guarded((Fw,), dev, torch.float32, guid, NAN)
    ww, wts = _guarded((K, Fw), dev, torch.float32, wts, NAN)
    ow, out = _guarded((Ft, 4, h, w), dev, torch.float32, None, 12345.0)
    pred_in = pred.clone()
    W.cfg_window_merge(pred, guid, wts, starts, Ft, out=out)
    torch.cuda.synchronize()
    want = TW.merge_reference(pred_in, guid.clone(), wts.clone(), starts, Ft)
    where = (case, (h, w), ldn, f32, integer)
    assert torch.equal(_bits(out), _bits(want)), where
    assert bool(torch.isfinite(out).all()) and _margins(ow, 12345.0), where
    assert torch.equal(_bits(pred), _bits(pred_in)) and _margins(pw, NAN) and _margins(gw, NAN) and _margins(ww, NAN), where
    if integer:                                              # exact in any order: the fp64 sum by the definition
        p64 = pred_in[..., :4].double()
        ref = torch.zeros(Ft, 4, h, w, dtype=torch.float64, device=dev)
        for k, st in enumerate(starts):
            mo = p64[k] + guid.double().view(Fw, 1, 1, 1) * (p64[K + k] - p64[k])
            ref[st:st + Fw] += (wts[k].double().view(Fw, 1, 1, 1) * mo).permute(0, 3, 1, 2)
        assert torch.equal(out.double(), ref), where
    return out


@pytest.mark.parametrize("ldn", [4, 8])
@pytest.mark.parametrize("f32", [True, False], ids=["fp32", "fp16"])
def test_merge_equals_fp32_tensor_arithmetic_bit_for_bit(dev, f32, ldn):
    """Every plan case ((9, 4, 2) has frames under 1, 2 and 3 windows) at 3 x 5 and 8 x 8, random data; then integer predictions with
    weights {0.25, 0.75}, exact in any order."""
    seed = 0
    for case, starts in TW.PLAN_CASES:
        for h, w in SHAPES:
            seed += 1
            _merge_case(dev, case, starts, h, w, ldn, f32, seed)
    for case, starts in (TW.PLAN_CASES[1], TW.PLAN_CASES[3]):                             # (7, 4, 3) and (6, 4, 3): one overlap each
        for h, w in SHAPES:
            seed += 1
            _merge_case(dev, case, starts, h, w, ldn, f32, seed, integer=True)


def test_merge_of_an_unaligned_prediction_and_beyond_one_pass_of_the_grid(dev):
    """An fp32 prediction whose base is 4-byte aligned only takes the scalar loads; 3 frames x 600 x 600 pixels are more than the
    grid's 256 x 16 x 256 threads, so the grid-stride loop runs more than once."""
    from posetraj_amd import windows as W
    g = torch.Generator(device=dev).manual_seed(77)
    starts, Ft, Fw, h, w = [0, 1], 3, 2, 3, 5
    buf = torch.randn(4 * Fw * h * w * 4 + 1, generator=g, device=dev)
    pred = buf[1:].view(4, Fw, h, w, 4)
    assert pred.data_ptr() % 16 == 4
    guid = torch.tensor([1.0, 3.0], device=dev)
    wts = torch.from_numpy(W.window_plan(Ft, Fw, 1).weights).to(dev)
    assert torch.equal(W.cfg_window_merge(pred, guid, wts, starts, Ft), TW.merge_reference(pred, guid, wts, starts, Ft))
    h = w = 600
    pred = torch.randn(4, Fw, h, w, 4, generator=g, device=dev).half()
    got = W.cfg_window_merge(pred, guid, wts, starts, Ft)
    assert torch.equal(got, TW.merge_reference(pred, guid, wts, starts, Ft))
    x = torch.randn(1, Ft, 4, h, w, generator=g, device=dev)
    il = torch.randn(2, 4, h, w, generator=g, device=dev).half()
    from posetraj_amd import ops
    rows = W.scale_concat_windows(x, il, 1.5, starts, Fw)
    for k, st in enumerate(starts):
        want = ops.scale_concat_input(x[:, st:st + Fw].contiguous(), il, 1.5)
        assert torch.equal(_bits(rows[k]), _bits(want[0])) and torch.equal(_bits(rows[2 + k]), _bits(want[1]))


def test_invalid_starts_return_a_status_that_names_the_entry_point_and_launch_nothing(dev):
    from posetraj_amd import hip, windows as W
    raw = ctypes.CDLL(hip.WINDOW_LIB_PATH)
    for name, (res, args) in hip.WINDOW_ABI.signatures.items():
        getattr(raw, name).restype, getattr(raw, name).argtypes = res, args
    Ft, Fw, h, w = 7, 4, 3, 5
    pred = torch.randn(4, Fw, h, w, 4, device=dev)
    guid, wts = torch.ones(Fw, device=dev), torch.ones(2, Fw, device=dev)
    ow, out = _guarded((Ft, 4, h, w), dev, torch.float32, None, 12345.0)
    x, il = torch.randn(1, Ft, 4, h, w, device=dev), torch.randn(2, 4, h, w, device=dev).half()
    o2w, o2 = _guarded((4, Fw, h, w, 8), dev, torch.float16, None, 777.0)
    for starts in ([1, 3], [0, 4], [3, 0], [0, 0], [0, 2]):
        a = (ctypes.c_int32 * 2)(*starts)
        rc = raw.ptw_cfg_window_merge(pred.data_ptr(), 1, 4, guid.data_ptr(), wts.data_ptr(), a, 2, Fw, Ft, h, w, out.data_ptr(), None)
        assert rc != 0 and "ptw_cfg_window_merge" in raw.ptw_last_error().decode(), starts
        rc = raw.ptw_scale_concat_windows(x.data_ptr(), il.data_ptr(), 1.5, a, 2, Fw, Ft, h, w, o2.data_ptr(), None)
        assert rc != 0 and "ptw_scale_concat_windows" in raw.ptw_last_error().decode(), starts
        with pytest.raises(RuntimeError, match="ptw_cfg_window_merge"):
            W.cfg_window_merge(pred, guid, wts, starts, Ft, out=out)
        with pytest.raises(RuntimeError, match="ptw_scale_concat_windows"):
            W.scale_concat_windows(x, il, 1.5, starts, Fw, out=o2)
    torch.cuda.synchronize()
    assert bool((ow == 12345.0).all()) and bool((o2w == 777.0).all())                     # nothing was launched


# ---------------------------------------------------------------------------------------------------------- the loop
def weight_map():
    w = torch.ones(FT, *HW)
    w[:, :, HW[1] // 2:] = 0.0
    w[4:] *= 0.25
    return w


# scenario -> (pipeline arguments, oracle arguments): "plain" steps only; "weighted" steps 0 and 1, step 2 outside the control window
SCENARIOS = {
    "plain": (dict(controlnet_cond_scale=SCALE), dict(scales=[SCALE] * STEPS)),
    "weighted+off": (dict(controlnet_cond_scale=SCALE, control_weight=weight_map(), control_guidance_end=0.7),
                     dict(scales=[SCALE] * STEPS, weight=weight_map(), on=[True, True, False])),
}


def oracle_windowed(cn, unet, sched, solver, plan, *, latents, il, emb, cond, scales, weight=None, on=None):
    """The fp32 oracle's loop with the windowing written out: per step one-clip evaluations of the two networks per window (on the
    window's slices of the latents, the maps and the weight map), window-local guidance, the blend with ``plan.weights``, then the
    scheduler's step on the blended prediction - "euler": the oracle scheduler's; "2m": k-diffusion's ``sample_dpmpp_2m`` update
    (as tests/test_sampler_gpu.py writes it).  ``latents`` ``[1, Ft, 4, h, w]``.  A one-window plan is the plain loop of one clip."""
    from oracle import loop as OL
    Fw = plan.window_frames
    sched.set_timesteps(len(scales))
    sig = [float(v) for v in sched.sigmas]
    g = OL.guidance_ramp(1.0, 3.0, Fw, 1, latents.dtype, latents.ndim)
    ids = OL.hot_added_time_ids(emb.dtype)
    wts = torch.from_numpy(plan.weights)
    ilw = il.unsqueeze(1).repeat(1, Fw, 1, 1, 1)
    d_prev = None
    with torch.no_grad():
        for i, t in enumerate(sched.timesteps):
            merged = torch.zeros_like(latents)
            for k, s in enumerate(plan.starts):
                x = sched.scale_model_input(torch.cat([latents[:, s:s + Fw]] * 2), t)
                x = torch.cat([x, ilw], dim=2)
                down, mid = cn(x, t, encoder_hidden_states=emb, controlnet_cond=cond[:, s:s + Fw], added_time_ids=ids,
                               conditioning_scale=scales[i], guess_mode=False, return_dict=False)
                res = list(down) + [mid]
                if weight is not None:
                    res = [r * torch.nn.functional.adaptive_avg_pool2d(weight[s:s + Fw], r.shape[-2:]).repeat(2, 1, 1).unsqueeze(1) for r in res]
                if on is not None and not on[i]:
                    res = [torch.zeros_like(r) for r in res]
                pred = unet(x, t, encoder_hidden_states=emb, down_block_additional_residuals=res[:-1], mid_block_additional_residual=res[-1],
                            added_time_ids=ids, return_dict=False)[0]
                un, co = pred.chunk(2)
                merged[:, s:s + Fw] += wts[k].view(1, Fw, 1, 1, 1) * (un + g * (co - un))
            if solver == "euler":
                latents = sched.step(merged, t, latents).prev_sample
            else:
                s0, s1 = sig[i], sig[i + 1]
                D = merged * (-s0 / (s0 * s0 + 1) ** 0.5) + latents / (s0 * s0 + 1)
                if s1 == 0.0:
                    latents = D
                else:
                    hh = math.log(s0) - math.log(s1)
                    if d_prev is None:
                        dd = D
                    else:
                        r = (math.log(sig[i - 1]) - math.log(s0)) / hh
                        dd = (1 + 1 / (2 * r)) * D - (1 / (2 * r)) * d_prev
                    latents = (s1 / s0) * latents - math.expm1(-hh) * dd
                d_prev = D
                sched._step_index += 1
    return latents


class Rig:
    """Tiny nets (zero-convs randomised: tests/parity.py), one request of FT frames, the pipelines, and the cached oracle / HIP runs."""

    def __init__(self, dev):
        from posetraj_amd import DPMPP2MDiscreteScheduler, EulerDiscreteScheduler, StableVideoDiffusionPipelineControlNet, SVD_SCHEDULER_CONFIG
        from posetraj_amd.windows import window_plan
        from oracle import sched as OS
        self.dev = dev
        self.cn_o, self.unet_o = P.build_oracle_nets(0)
        self.cn_h, self.unet_h = P.build_hip_nets(self.cn_o, self.unet_o, dev)
        lat, self.il, self.emb, self.cond = P.loop_inputs(0, FT, *HW, self.unet_o.config.cross_attention_dim)
        self.new_osched = lambda: OS.OracleEulerDiscreteScheduler(**OS.SVD_SCHEDULER_CONFIG)
        so = self.new_osched()
        so.set_timesteps(STEPS)
        self.lat0 = lat * so.init_noise_sigma
        self.plan = window_plan(FT, FW, STRIDE)
        assert list(self.plan.starts) == [0, 3]
        scheds = dict(euler=EulerDiscreteScheduler, dpmpp2m=DPMPP2MDiscreteScheduler)
        self.new_pipe = lambda sampler: StableVideoDiffusionPipelineControlNet(unet=self.unet_h, controlnet=self.cn_h,
                                                                               scheduler=scheds[sampler](**SVD_SCHEDULER_CONFIG))
        self._pipes, self._oracle, self._hip, self._batch = {}, {}, {}, {}

    def pipe(self, sampler):
        if sampler not in self._pipes:
            self._pipes[sampler] = self.new_pipe(sampler)
        return self._pipes[sampler]

    def oracle(self, name, sampler):
        if (name, sampler) not in self._oracle:
            self._oracle[(name, sampler)] = oracle_windowed(self.cn_o, self.unet_o, self.new_osched(), "euler" if sampler == "euler" else "2m", self.plan,
                                                            latents=self.lat0, il=self.il, emb=self.emb, cond=self.cond, **SCENARIOS[name][1])
        return self._oracle[(name, sampler)]

    def denoise(self, sampler, graph, lat=None, pipe=None, **kw):
        d = self.dev
        kw = {k: (v.to(d) if torch.is_tensor(v) else v) for k, v in kw.items()}
        out = (pipe or self.pipe(sampler)).denoise((self.lat0 if lat is None else lat).to(d), self.il.to(d), self.emb.to(d), self.cond.to(d),
                                                  num_inference_steps=STEPS, use_graph=graph, overlap_streams=graph, **kw)
        torch.cuda.synchronize()
        return out.cpu()

    def hip(self, name, sampler, batch, graph):
        key = (name, sampler, batch, graph)
        if key not in self._hip:
            self._hip[key] = self.denoise(sampler, graph, window_frames=FW, window_stride=STRIDE, window_batch=batch, **SCENARIOS[name][0])
        return self._hip[key]

    def batch_distance(self, name, sampler):
        """The existing code's distance on the same request: the two windows as an ``independent_clips`` batch of 2 clips of FW frames
        (no blending: each clip denoised on its own) against the oracle's loop on each clip alone."""
        from posetraj_amd.windows import window_plan
        if (name, sampler) not in self._batch:
            d, one = self.dev, window_plan(FW, FW, FW)
            kw_h, kw_o = SCENARIOS[name]
            cut = lambda t: torch.stack([t[:, s:s + FW] for s in self.plan.starts], 1).flatten(0, 1)
            refs = []
            for s in self.plan.starts:
                o = dict(kw_o, weight=kw_o["weight"][s:s + FW]) if "weight" in kw_o else kw_o
                refs.append(oracle_windowed(self.cn_o, self.unet_o, self.new_osched(), "euler" if sampler == "euler" else "2m", one,
                                            latents=self.lat0[:, s:s + FW], il=self.il, emb=self.emb, cond=self.cond[:, s:s + FW], **o))
            kw = dict(kw_h, control_weight=cut(kw_h["control_weight"][None])) if "control_weight" in kw_h else kw_h
            kw = {k: (v.to(d) if torch.is_tensor(v) else v) for k, v in kw.items()}
            out = self.new_pipe(sampler).denoise(cut(self.lat0).to(d), self.il.repeat_interleave(2, 0).to(d), self.emb.repeat_interleave(2, 0).to(d),
                                                 cut(self.cond).to(d), num_inference_steps=STEPS, independent_clips=True, **kw)
            torch.cuda.synchronize()
            self._batch[(name, sampler)] = TW.rel_l2(out, torch.cat(refs))
        return self._batch[(name, sampler)]


@pytest.fixture(scope="module")
def rig(dev):
    return Rig(dev)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_one_window_is_the_plain_loop_bit_for_bit(rig, graph):
    """4 frames, 2 steps of DPM-Solver++(2M): ``denoise(window_frames=4)`` goes through the window path (one window, weight 1.0) and must
    equal ``denoise()`` bit for bit - the guidance order and the multistep arithmetic are shared.  (Euler: ``cfg_euler_kernel``'s fp32
    guidance is not under ``contract(off)``; that path is held to the oracle below.)"""
    d, lat = rig.dev, rig.lat0[:, :FW]
    args = (rig.il.to(d), rig.emb.to(d), rig.cond[:, :FW].to(d))
    kw = dict(num_inference_steps=2, controlnet_cond_scale=SCALE, use_graph=graph, overlap_streams=graph)
    pipe = rig.new_pipe("dpmpp2m")
    seen = []
    plain = pipe.denoise(lat.to(d), *args, **kw)
    win = pipe.denoise(lat.to(d), *args, window_frames=FW, callback_on_step_end=lambda p_, i, t, k: seen.append(tuple(k["latents"].shape)) or {}, **kw)
    again = pipe.denoise(lat.to(d), *args, **kw)                       # the plain loop after a windowed call: the shared state is clean
    torch.cuda.synchronize()
    assert torch.equal(win, plain) and torch.equal(again, plain) and bool(torch.isfinite(win).all())
    assert seen == [(1, FW, 4, *HW)] * 2
    if graph:
        assert len(pipe._step_graphs) == 1 and all(s.windows is None for s in pipe._step_graphs.values())         # one graph served all three


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("sampler", ["euler", "dpmpp2m"])
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_windowed_loop_matches_the_oracle_with_the_windowing_written_out(rig, name, sampler, batch, capsys):
    """Ft = 7, Fw = 4, s = 3 (two windows, frame 3 under both), 8 x 8 latent, 3 steps; eager and (graph + two streams).  Bound: module
    docstring.  The windowed result must also lie more than 10 bounds from the native 7-frame call: ignoring the windows fails."""
    ora = rig.oracle(name, sampler)
    runs = {g: rig.hip(name, sampler, batch, g) for g in (False, True)}
    dist = {g: TW.rel_l2(runs[g], ora) for g in runs}
    d_batch = rig.batch_distance(name, sampler)
    bound = max(TW.LOOP_BOUND, 1.25 * d_batch)
    native = rig.denoise(sampler, False, **SCENARIOS[name][0])
    sep = TW.rel_l2(runs[False], native)
    with capsys.disabled():
        print(f"\n  {name}, {sampler}, window_batch = {batch}: windowed | oracle eager {dist[False]:.3e}, graph + two streams {dist[True]:.3e}; "
              f"independent 2-clip batch | its oracle {d_batch:.3e}; bound {bound:.3e}; windowed | native {FT}-frame call {sep:.3e}")
    assert runs[False].shape == (1, FT, 4, *HW) and bool(torch.isfinite(runs[False]).all())
    for g in dist:
        assert dist[g] <= bound, (name, sampler, batch, g, dist[g], bound)
    assert sep > 10 * bound, (sep, bound)


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_groups_of_one_and_of_k_windows_give_the_same_latents(rig, name, capsys):
    """2M path, eager and graph: the networks are per clip, only the batched launch shapes differ."""
    for g in (False, True):
        one, both = rig.hip(name, "dpmpp2m", 1, g), rig.hip(name, "dpmpp2m", 2, g)
        d = TW.rel_l2(one, both)
        with capsys.disabled():
            print(f"\n  {name}, {'graph' if g else 'eager'}: window_batch 1 | 2 rel-L2 {d:.3e}, bit for bit: {torch.equal(one, both)}")
        assert torch.equal(one, both), (name, g, d)


def test_windowed_graphs_are_those_of_an_independent_batch(rig):
    """One pipeline: a windowed call with ``window_batch = 2`` captures one graph; an ``independent_clips`` batch of 2 clips of FW frames
    then replays it (no new capture), and a second windowed call - another plan over the same geometry - replays it too."""
    d = rig.dev
    pipe = rig.new_pipe("dpmpp2m")
    first = rig.denoise("dpmpp2m", True, pipe=pipe, window_frames=FW, window_stride=STRIDE, controlnet_cond_scale=SCALE)
    assert torch.equal(first, rig.hip("plain", "dpmpp2m", 2, True))
    states = dict(pipe._step_graphs)
    assert len(states) == 1 and [k.Bc for k in states] == [2] and [k.F for k in states] == [FW]
    cut = lambda t: torch.stack([t[:, s:s + FW] for s in rig.plan.starts], 1).flatten(0, 1)
    kw = dict(num_inference_steps=STEPS, controlnet_cond_scale=SCALE, independent_clips=True)
    args = (cut(rig.lat0).to(d), rig.il.repeat_interleave(2, 0).to(d), rig.emb.repeat_interleave(2, 0).to(d), cut(rig.cond).to(d))
    replayed = pipe.denoise(*args, use_graph=True, overlap_streams=True, **kw)
    assert dict(pipe._step_graphs) == states and all(pipe._step_graphs[k].graph is s.graph for k, s in states.items())
    eager = rig.new_pipe("dpmpp2m").denoise(*args, **kw)
    torch.cuda.synchronize()
    assert torch.equal(replayed, eager)
    lat8 = torch.cat([rig.lat0, rig.lat0[:, :1]], 1)                                      # 8 frames, stride 4: two windows, no overlap
    cond8 = torch.cat([rig.cond, rig.cond[:, :1]], 1)
    out8 = pipe.denoise(lat8.to(d), rig.il.to(d), rig.emb.to(d), cond8.to(d), num_inference_steps=STEPS, controlnet_cond_scale=SCALE,
                        use_graph=True, overlap_streams=True, window_frames=FW, window_stride=FW)
    torch.cuda.synchronize()
    assert dict(pipe._step_graphs) == states and out8.shape == (1, 8, 4, *HW) and bool(torch.isfinite(out8).all())


# ---------------------------------------------------------------------------------------------------------- __call__
def test_call_end_to_end_on_the_camera_twin(dev):
    """Tiny VAE and a CLIP stand-in, the camera pipeline (``**kw``), Ft = 7: ``output_type`` "latent" equals the direct ``denoise`` call
    on the same inputs (so ``camera_cond [7, 12]`` reaches the windows sliced), after one step the frames under the first window alone do
    not depend on the second window's camera rows, and "pt" decodes 7 frames in chunks of ``window_frames``."""
    from oracle import init as OI, vae as OV
    from posetraj_amd import EulerDiscreteScheduler, SVD_SCHEDULER_CONFIG
    from posetraj_amd.autoencoder_kl_temporal_decoder import AutoencoderKLTemporalDecoder
    from posetraj_amd.pipeline_stable_video_diffusion_controlnet_cam import StableVideoDiffusionPipelineControlNet as CamPipe
    cn_o, unet_o = P.build_oracle_nets(0, camera=True)
    cn_h, unet_h = P.build_hip_nets(cn_o, unet_o, dev, camera=True)
    vae_o = OI.seeded_init_(OV.AutoencoderKLTemporalDecoder(**OV.tiny_vae_config()), seed=3).eval()
    vae = AutoencoderKLTemporalDecoder(**OV.tiny_vae_config()).load_state_dict(vae_o.state_dict(), dev)
    proj = torch.randn(3, unet_o.config.cross_attention_dim, generator=torch.Generator().manual_seed(2)).to(dev)

    class Clip:                                              # stands in for CLIPVisionModelWithProjection: [B, 3, 224, 224] -> [B, D]
        dtype = torch.float32

        def __call__(self, x):
            return torch.tanh(x.mean((2, 3)) @ proj)
    pipe = CamPipe(vae=vae, image_encoder=Clip(), unet=unet_h, controlnet=cn_h, scheduler=EulerDiscreteScheduler(**SVD_SCHEDULER_CONFIG))
    g = torch.Generator().manual_seed(21)
    image = torch.rand(1, 3, 64, 64, generator=g)
    maps = torch.rand(FT, 3, 64, 64, generator=g)
    cam = (torch.randn(FT, 12, generator=g) * 0.3).half().float()
    lat = torch.randn(1, FT, 4, *HW, generator=g)
    chunks = []
    decode = vae.decode
    vae.decode = lambda z, num_frames=None, **kw: chunks.append((z.shape[0], num_frames)) or decode(z, num_frames=num_frames, **kw)
    common = dict(height=64, width=64, num_frames=FT, num_inference_steps=2, latents=lat, return_dict=False, controlnet_cond_scale=SCALE,
                  window_frames=FW, window_stride=STRIDE)
    seed = lambda: torch.Generator().manual_seed(5)
    try:
        full = pipe(image, maps, cam.tolist(), output_type="latent", generator=seed(), **common)
        assert not chunks
        frames = pipe(image, maps, cam.tolist(), output_type="pt", generator=seed(), **common)
    finally:
        del vae.decode
    assert full.shape == (1, FT, 4, *HW) and bool(torch.isfinite(full).all())
    assert isinstance(frames, list) and len(frames) == 1 and frames[0].shape == (FT, 3, 64, 64) and bool(torch.isfinite(frames[0]).all())
    assert chunks == [(4, 4), (3, 3)]                                                     # decode_chunk_size defaults to window_frames
    # the loop alone, from given stage outputs: __call__ equals the direct denoise call on the camera rows [2, 7, 12]
    emb = pipe._encode_image(image, dev, 1, True)
    mode = torch.randn(1, 4, *HW, generator=g).half()
    il = torch.cat([torch.zeros_like(mode), mode]).to(dev)
    given = dict(common, image_embeddings=emb, image_latents=il, output_type="latent")
    got = pipe(None, maps, cam.tolist(), **given)
    pipe.scheduler.set_timesteps(2, device=dev)
    cond = torch.cat([pipe.preprocess_condition(maps, 64, 64).unsqueeze(0)] * 2)
    lat0 = pipe.prepare_latents(1, FT, 8, 64, 64, emb.dtype, dev, None, lat)
    kw = dict(controlnet_cond_scale=SCALE, use_graph=True, overlap_streams=True, window_frames=FW, window_stride=STRIDE)
    want = pipe.denoise(lat0, il, emb, cond, num_inference_steps=2, camera_cond=torch.cat([cam.unsqueeze(0)] * 2), **kw)
    assert torch.equal(got, want)
    # one step: frames 0 .. 2 lie under the first window alone, whose camera rows are 0 .. 3
    cam2 = cam.clone()
    cam2[FW:] += 0.5                                                                      # rows 4 .. 6: the second window's alone
    one = pipe(None, maps, cam.tolist(), **dict(given, num_inference_steps=1))
    other = pipe(None, maps, cam2.tolist(), **dict(given, num_inference_steps=1))
    torch.cuda.synchronize()
    assert torch.equal(other[:, :STRIDE], one[:, :STRIDE]) and not torch.equal(other[:, STRIDE:], one[:, STRIDE:])
