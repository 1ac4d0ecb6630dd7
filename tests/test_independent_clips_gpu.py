"""``independent_clips`` on the MI355X: ``vec_mode`` 3 of ``pt_igemm_f16`` and of the fused feed-forward's prologue exactly, on integer
data, against the index of include/posetraj_hip.h; no leak between the clips of a batch, bit for bit; every clip of an independent
batch against the fp32 oracle run on that clip ALONE (tests/test_independent_clips_cpu.py holds the inputs to the condition that the
reference's coupled batch lies >= 10 bounds away); the denoise loop, eager and captured; ``__call__`` with K requests; the trainer
against the MEAN of the oracle's one-clip fp32-autograd steps, at the bounds of the existing batch tests.

Exactness.  Activations in {-3 .. 3}, weights in {-2 .. 2}, bias, residual and row vectors small integers: every partial sum is an integer
far below 2^24, the result an integer below 2^11, so the fp16 output is THE integer whatever the tile, the split or the order of
summation (the argument of tests/test_igemm_exact_gpu.py).  The table's rows are pairwise different (row r lies near 32 r): a row taken
from another clip, or from the other CFG half, changes every column."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import independent_clips as IC
from tests import parity as P
from tests.test_train_batch_gpu import DROP, DROP_BOUNDS, flat, make_batch, nets, rel, trainer  # noqa: F401  (nets: a fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from posetraj_amd import ops
    d = torch.device("cuda:0")
    ops.ensure_ready(d)
    return d


# ------------------------------------------------------------------------------------------------- vec_mode 3, exactly
INDEX_CASES = [(2, 2, 5), (3, 3, 15), (2, 2, 6)]       # (Bc, F, S): 40 rows; 270 rows - across a 256-row tile, odd S, 2 Bc = 6; even S


def forced(cfg):
    """pt_igemm_force_config for the duration of a ``with``."""
    import contextlib
    from posetraj_amd import hip

    @contextlib.contextmanager
    def cm():
        L = hip.lib()
        try:
            assert L.pt_igemm_force_config(cfg) == 0
            yield
        finally:
            L.pt_igemm_force_config(-1)
    return cm()


def run_igemm(dev, c, K, cfg, with_res=True):
    from posetraj_amd import ops, packing
    pw = packing.pack_linear(c["w"], c["bias"], dev)
    with forced(cfg):
        out = ops.igemm(c["x"].half().to(dev), pw, res=c["res"].half().to(dev) if with_res else None, vec=c["vec"].half().to(dev), **c["vec_kw"])
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("Bc,F,S", INDEX_CASES)
def test_igemm_mode3_is_exact_under_every_forced_configuration(dev, Bc, F, S, cfg):
    """N = K = 64, channel-aligned K, residual + row vector.  Mode 3 runs in the plain-loop kernels' instances of their own: a forced
    256 x 320 tile (cfg 3) is planned as 128 x 320, the 256 x 256 tile (cfg 0) takes its plain loop (igemm.hip: plan)."""
    c = IC.integer_case(Bc, F, S)
    got = run_igemm(dev, c, 64, cfg)
    bad = int((got != c["want"]).sum())
    print(f"vec_mode 3 (Bc, F, S) = ({Bc}, {F}, {S}) cfg {cfg}: {bad} of {got.numel()} elements differ")
    assert got.dtype == torch.float16 and bad == 0
    coupled = c["x"].double() @ c["w"].double().t() + c["bias"].double() + c["res"].double() + \
        c["vec"].double()[torch.from_numpy(IC.mode2_index(np.arange(c["M"]), F * S, S, 2 * Bc))]
    assert not torch.equal(coupled.half(), c["want"])                                      # the reference's index is another result here


@pytest.mark.parametrize("cfg", [0, 1, 2, 4, 5])
def test_igemm_mode3_is_exact_on_the_generic_k_kernels(dev, cfg):
    """K = 72 is no multiple of the 64-deep tile: the generic gather of mode 3's plain-loop instances."""
    c = IC.integer_case(3, 3, 15, K=72)
    got = run_igemm(dev, c, 72, cfg)
    assert int((got != c["want"]).sum()) == 0
    got = run_igemm(dev, IC.integer_case(2, 2, 5, K=72), 72, cfg, with_res=False)           # one side input
    c2 = IC.integer_case(2, 2, 5, K=72)
    assert torch.equal(got, (c2["want"].double() - c2["res"].double()).half())


def test_igemm_mode3_is_exact_through_split_k(dev):
    """270 x 320 x 3200 on the automatic plan: split-K slabs and the reducer's epilogue (the plan is asked, not assumed)."""
    from posetraj_amd import hip
    Bc, F, S = 3, 3, 15
    c = IC.integer_case(Bc, F, S, N=320, K=3200)
    p = hip.IgemmParams()
    p.x0 = p.w = p.out = p.vec = p.res = 256
    p.C0, p.ld0, p.ldo, p.ldv, p.ldr, p.N = 3200, 3200, 320, 320, 320, 320
    p.Nimg, p.Hin, p.Win, p.Hout, p.Wout, p.KH, p.KW, p.stride = c["M"], 1, 1, 1, 1, 1, 1, 1
    p.M, p.K, p.Kpad = c["M"], 3200, 3200
    p.vec_mode, p.vG, p.vFS, p.vS, p.vB = 3, Bc, F * S, S, 2 * Bc
    assert hip.lib().pt_igemm_splitk_ws_bytes(ctypes.byref(p)) > 0
    got = run_igemm(dev, c, 3200, -1)
    assert int((got != c["want"]).sum()) == 0


def test_library_refuses_bad_mode3_arguments_at_the_launch(dev):
    from posetraj_amd import ops, packing
    c = IC.integer_case(2, 2, 5)
    pw = packing.pack_linear(c["w"], c["bias"], dev)
    x, vec = c["x"].half().to(dev), c["vec"].half().to(dev)
    for bad in (dict(vG=0), dict(vB=3), dict(vS=0), dict(vFS=0)):
        with pytest.raises(RuntimeError, match="pt_igemm_f16.*vec_mode 3"):
            ops.igemm(x, pw, vec=vec, **dict(c["vec_kw"], **bad))


def ffn_operands(dev, M, seed=3):
    from posetraj_amd import packing
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, k=1.0: (torch.randn(*s, generator=g) * k).half().float()
    w1 = packing.pack_linear(rn(128, 320, k=0.05), rn(128, k=0.1), dev, geglu=True)          # inner = 64
    w2 = packing.pack_linear(rn(320, 64, k=0.1), rn(320, k=0.1), dev)
    wo = packing.pack_linear(rn(320, 320, k=0.05), rn(320, k=0.1), dev)
    a, u, hs = (rn(M, 320).half().to(dev) for _ in range(3))
    ln = ((1 + rn(320, k=0.1)).half().to(dev), rn(320, k=0.1).half().to(dev))
    return w1, w2, wo, a, u, hs, ln


def test_ffn_prologue_mode3_reads_the_rows_of_the_index(dev):
    """C = 320, (Bc, F, S) = (2, 3, 23): 276 rows, across the 128-row workgroup, odd S.  The same launch with the table EXPANDED on the
    host by the index model (one row per token, mode 1 with vG = 1) runs the same arithmetic on the same values: bit equality holds
    exactly when the kernel's index is the model's.  The reference's index (mode 2) gives another result."""
    from posetraj_amd import ops
    Bc, F, S = 2, 3, 23
    M = 2 * Bc * F * S
    w1, w2, wo, a, u, hs, ln = ffn_operands(dev, M)
    tbl = (torch.randn(2 * Bc, 320, generator=torch.Generator().manual_seed(9)) + 4.0 * torch.arange(2 * Bc)[:, None]).half().to(dev)
    run = lambda **pre: ops.ffn_geglu(a, w1, w2, blend=hs, alpha=0.25, pre=dict(w=wo, res=u, ln=ln, **pre))
    got = run(vec=tbl, vec_mode=3, vG=Bc, vFS=F * S, vS=S, vB=2 * Bc)
    idx = torch.from_numpy(IC.mode3_index(np.arange(M), Bc, F * S, S, 2 * Bc)).to(dev)
    want = run(vec=tbl[idx].contiguous(), vec_mode=1, vG=1)
    coupled = run(vec=tbl, vec_mode=2, vFS=F * S, vS=S, vB=2 * Bc)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want) and not torch.equal(got, coupled)
    one = run(vec=tbl, vec_mode=3, vG=1, vFS=F * S, vS=S, vB=2 * Bc)                        # vG = 1 is mode 2
    assert torch.equal(one, coupled)
    with pytest.raises(RuntimeError, match="pt_ffn_geglu_f16.*pre_vec_mode 3"):
        run(vec=tbl, vec_mode=3, vG=0, vFS=F * S, vS=S, vB=2 * Bc)
    with pytest.raises(RuntimeError, match="pt_ffn_geglu_f16.*pre_vB"):
        run(vec=tbl, vec_mode=3, vG=3, vFS=F * S, vS=S, vB=2 * Bc)
    with pytest.raises(RuntimeError, match="pt_ffn_geglu_f16.*vec_mode 3 serves pre_vec"):
        ops.ffn_geglu(a, w1, w2, res=u, vec=tbl, vec_mode=3, vG=Bc, vFS=F * S, vS=S, vB=2 * Bc)


# ------------------------------------------------------------------------------------------------- the networks' forward on a batch
class Rig:
    def __init__(self, dev):
        from posetraj_amd import DPMPP2MDiscreteScheduler, EulerDiscreteScheduler, SVD_SCHEDULER_CONFIG
        from posetraj_amd import StableVideoDiffusionPipelineControlNet as Pipe
        self.dev = dev
        self.cn_o, self.unet_o = P.build_oracle_nets(0)
        self.cn_h, self.unet_h = P.build_hip_nets(self.cn_o, self.unet_o, dev)
        sched = dict(euler=EulerDiscreteScheduler, dpmpp2m=DPMPP2MDiscreteScheduler)
        self.new_pipe = lambda sampler="euler": Pipe(unet=self.unet_h, controlnet=self.cn_h, scheduler=sched[sampler](**SVD_SCHEDULER_CONFIG))
        self.pipe = self.new_pipe()

    def forward(self, batch, independent):
        """ControlNet + U-Net of one loop iteration on ``IC.clip_batch`` -> the prediction ``[2 Bc, F, 4, h, w]`` fp32 on the host."""
        d, Bc = self.dev, batch["sample"].shape[0] // 2
        with torch.no_grad():
            pred = self.pipe._networks_step("plain", batch["sample"].half().to(d), batch["t"], batch["ehs"].half().to(d), batch["cond"].half().to(d),
                                            None, batch["ids"].to(d), IC.COND_SCALE, None, False, None, Bc if independent else 0)
        torch.cuda.synchronize()
        return pred.permute(0, 1, 4, 2, 3).float().cpu()

    def _args(self, batch, independent):
        d, Bc = self.dev, batch["sample"].shape[0] // 2
        return (batch["sample"].half().to(d), batch["t"], batch["ehs"].half().to(d), batch["ids"].to(d)), (dict(independent_clips=Bc) if independent else {})

    def unet_forward(self, batch, down, mid, independent):
        """The U-Net alone on given ControlNet residuals (``forward``'s two halves; the flag is the pipeline's private argument)."""
        args, ind = self._args(batch, independent)
        with torch.no_grad():
            state = self.unet_h._encode(*args, **ind)
            y = self.unet_h._decode(state, [r.half().to(self.dev) for r in down], mid.half().to(self.dev), return_dict=False)[0]
        torch.cuda.synchronize()
        return y.float().cpu()

    def controlnet_mid(self, batch, independent):
        """The ControlNet's mid residual x COND_SCALE (``forward``'s last launch on ``_features``) -> ``[2 Bc F, C, h', w']``."""
        from posetraj_amd import ops
        args, ind = self._args(batch, independent)
        with torch.no_grad():
            _, x = self.cn_h._features(*args, batch["cond"].half().to(self.dev), None, **ind)
            n, hh, ww, c = x.shape
            y = ops.igemm(x, self.cn_h.controlnet_mid_block, geom=(n, hh, ww), out_scale=IC.COND_SCALE).view(n, hh, ww, c).permute(0, 3, 1, 2)
        torch.cuda.synchronize()
        return y.float().cpu()


@pytest.fixture(scope="module")
def rig(dev):
    return Rig(dev)


@pytest.mark.parametrize("Bc", [2, 3])
def test_no_leak_between_the_clips_of_an_independent_batch(rig, Bc):
    """Two runs of the same shapes - the same plan, the same summation order.  The second changes clip 1's embedding, latents, image
    latents and maps: clip 0's rows (and clip 2's) of the prediction stay bit-identical and clip 1's change.  With the flag off clip
    0's rows change: the reference's batch lets clip 1's image into clip 0's video."""
    F, h, w = 2, 8, 24
    a, b = IC.clip_batch(Bc, F, h, w), IC.clip_batch(Bc, F, h, w, change_clip=1)
    ya, yb = rig.forward(a, True), rig.forward(b, True)
    for c in range(Bc):
        same = torch.equal(IC.clip_rows(ya, c), IC.clip_rows(yb, c))
        assert same == (c != 1), (Bc, c)
    assert bool(torch.isfinite(ya).all())
    ca, cb = rig.forward(a, False), rig.forward(b, False)
    assert not torch.equal(IC.clip_rows(ca, 0), IC.clip_rows(cb, 0))
    assert not torch.equal(ca, ya)


@pytest.mark.parametrize("Bc,F,h,w", IC.FORWARD_CASES)
def test_every_clip_of_an_independent_batch_matches_the_oracle_on_that_clip_alone(rig, Bc, F, h, w):
    """Per clip, against the fp32 oracle run on that clip ALONE.  Three quantities, each at the bound tests/test_parity_ladder_gpu.py
    states for it:

    * ``unet`` - the prediction of the U-Net forward on the oracle's own ControlNet residuals, the quantity "the project's stated forward
      bound" is stated for ("<= 1e-3 for one network forward", ``TOL_UNET_FP32``): rel-L2 <= 1e-3;
    * ``mid`` - the ControlNet's mid residual: <= 1.55e-3 (``TOL_CN_FP32``);
    * ``chained`` - the prediction of the two networks chained, as a loop iteration runs them: <= 2.2e-3 (``TOL_LOOP_FP32``; the ladder
      measures 1.4 - 1.8e-3 for it on these networks) AND no further from the oracle than 1.25 x what the ONE-CLIP call - the launches
      the project has always issued - measures on the same request in the same run.  The two differ in the rows per launch, hence in
      tile plans and summation order: two realisations of the same rounding noise, so neither is "the" distance; 1.25 is the project's
      margin over a measured distance.  Measured (profiles/r18/independent_clips.txt, section 3): 1.10 - 1.26e-3 for the batch, and on
      these small shapes the batch's rows came out bit-identical to the one-clip call's.

    The coupled batch lies >= 10 x the widest of these bounds from the chained reference on these inputs
    (tests/test_independent_clips_cpu.py), and the run with the flag off is held to that here."""
    from tests.test_parity_ladder_gpu import TOL_CN_FP32, TOL_LOOP_FP32, TOL_UNET_FP32
    assert TOL_UNET_FP32 == IC.FORWARD_BOUND and TOL_LOOP_FP32 == IC.CHAINED_BOUND
    batch = IC.clip_batch(Bc, F, h, w)
    alone = [IC.oracle_networks(rig.cn_o, rig.unet_o, IC.one_clip(batch, c)) for c in range(Bc)]
    halves_major = lambda ts: torch.cat([t[half * F:(half + 1) * F] for half in (0, 1) for t in ts])      # [2 F, ...] per clip -> [2 Bc F, ...]
    down = [halves_major([a["down"][j] for a in alone]) for j in range(len(alone[0]["down"]))]
    mid = halves_major([a["mid"] for a in alone])
    legs = {flag: dict(unet=rig.unet_forward(batch, down, mid, flag), mid=rig.controlnet_mid(batch, flag), chained=rig.forward(batch, flag))
            for flag in (True, False)}
    rows = lambda t, c: IC.clip_rows(t.reshape(2 * Bc, F, *t.shape[-3:]), c)
    for c in range(Bc):
        ref = dict(unet=alone[c]["pred"], mid=alone[c]["mid"].reshape(2, F, *mid.shape[-3:]) * IC.COND_SCALE, chained=alone[c]["pred_chained"])
        for leg, bound in (("unet", TOL_UNET_FP32), ("mid", TOL_CN_FP32), ("chained", TOL_LOOP_FP32)):
            d, dc = IC.rel_l2(rows(legs[True][leg], c), ref[leg]), IC.rel_l2(rows(legs[False][leg], c), ref[leg])
            print(f"Bc = {Bc}, F = {F}, {h} x {w}, clip {c}, {leg}: independent batch vs the oracle on the clip alone {d:.3e} (bound {bound}); flag off {dc:.3e}")
            assert d <= bound, (leg, c, d)
        single = rig.forward(IC.one_clip(batch, c), False)                                  # the one-clip call: mode 2, as ever
        d, ds = IC.rel_l2(rows(legs[True]["chained"], c), ref["chained"]), IC.rel_l2(single, ref["chained"])
        dd = IC.rel_l2(rows(legs[True]["chained"], c), single)
        print(f"Bc = {Bc}, F = {F}, {h} x {w}, clip {c}, chained: batch {d:.3e}, one-clip call {ds:.3e} vs the oracle; batch vs one-clip call {dd:.3e}")
        assert d <= 1.25 * ds, (c, d, ds)
        assert IC.rel_l2(rows(legs[False]["chained"], c), ref["chained"]) >= 10 * IC.CHAINED_BOUND


# ------------------------------------------------------------------------------------------------- the loop
STEPS, FRAMES, HW = 3, 4, (8, 8)


def spy_modes(monkeypatch):
    """Every ``vec_mode`` that reaches ``ops.igemm`` / the prologue of ``ops.ffn_geglu``."""
    from posetraj_amd import ops
    seen, ig, ff = [], ops.igemm, ops.ffn_geglu
    monkeypatch.setattr(ops, "igemm", lambda *a, **kw: seen.append(kw.get("vec_mode", 0)) or ig(*a, **kw))
    monkeypatch.setattr(ops, "ffn_geglu", lambda *a, **kw: seen.append((kw.get("pre") or {}).get("vec_mode", 0)) or ff(*a, **kw))
    return seen


def loop(rig, pipe, inputs, graph, flag):
    d = rig.dev
    lat, il, emb, cond = inputs
    pipe.scheduler.set_timesteps(STEPS)
    out = pipe.denoise((lat * pipe.scheduler.init_noise_sigma).to(d), il.to(d), emb.to(d), cond.to(d), num_inference_steps=STEPS,
                       controlnet_cond_scale=IC.COND_SCALE, use_graph=graph, overlap_streams=graph, independent_clips=flag)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("sampler", ["euler", "dpmpp2m"])
def test_loop_graph_equals_eager_and_the_two_modes_never_share_a_graph(rig, sampler):
    _, batch = IC.loop_requests(2, FRAMES, *HW)
    pipe = rig.new_pipe(sampler)
    eager = loop(rig, pipe, batch, False, True)
    assert len(pipe._step_graphs) == 0
    graph = loop(rig, pipe, batch, True, True)
    assert torch.equal(eager, graph) and bool(torch.isfinite(graph).all())
    (key, st), = pipe._step_graphs.items()
    assert ("independent_clips", True) in key.dispatch and key.Bc == 2 and pipe._step_graphs.of_kind("plain") is st
    again = loop(rig, pipe, batch, True, True)                                              # the same graph, replayed
    assert torch.equal(again, graph) and pipe._step_graphs.of_kind("plain") is st
    coupled = loop(rig, pipe, batch, True, False)                                           # the flag flipped: a capture of its own
    (key2, st2), = pipe._step_graphs.items()
    assert ("independent_clips", False) in key2.dispatch and key2 != key and st2 is not st and st2.graph is not st.graph
    assert torch.equal(coupled, loop(rig, pipe, batch, False, False)) and not torch.equal(coupled, graph)
    back = loop(rig, pipe, batch, True, True)                                               # and back: captured again, the same result
    assert torch.equal(back, graph) and pipe._step_graphs.of_kind("plain") is not st2 and ("independent_clips", True) in pipe._step_graphs.of_kind("plain").key.dispatch


def test_one_clip_is_untouched_by_the_flag(rig, monkeypatch):
    """Bc = 1: bit-identical with and without the flag, and no launch carries mode 3; at Bc = 2 the flag's launches do and the
    default's do not."""
    seen = spy_modes(monkeypatch)
    reqs, batch = IC.loop_requests(2, FRAMES, *HW)
    pipe = rig.new_pipe()
    on = loop(rig, pipe, reqs[0], False, True)
    assert 2 in seen and 3 not in seen
    del seen[:]
    assert torch.equal(on, loop(rig, pipe, reqs[0], False, False)) and 3 not in seen
    del seen[:]
    loop(rig, pipe, batch, False, False)
    assert 2 in seen and 3 not in seen
    del seen[:]
    loop(rig, pipe, batch, False, True)
    assert 3 in seen and 2 not in seen


def test_call_with_two_requests_gives_each_its_own_clip(rig):
    """``__call__(independent_clips=True)``: a list of two images, two map sets, two generators, ``output_type="latent"``.  Request k
    within the loop tolerance (``TOL_NET`` of tests/test_model_gpu.py) of the ORACLE chain run on request k alone, from the latents
    generator k gives a call of its own."""
    from oracle import loop as OL, sched as OS
    from posetraj_amd.pipeline_stable_video_diffusion_controlnet import randn_tensor
    from tests.test_model_gpu import TOL_NET
    d, K, F, steps = rig.dev, 2, 14, 2
    h, w = HW
    reqs, (_, il, emb, cond) = IC.loop_requests(K, F, h, w)
    gens = lambda: [torch.Generator().manual_seed(40 + k) for k in range(K)]
    pipe = rig.new_pipe()
    out = pipe([torch.zeros(3, 8 * h, 8 * w)] * K, [r[3][0] for r in reqs], height=8 * h, width=8 * w, num_frames=F, num_inference_steps=steps,
               generator=gens(), output_type="latent", image_embeddings=emb.to(d), image_latents=il.to(d), controlnet_cond_scale=IC.COND_SCALE,
               independent_clips=True)
    torch.cuda.synchronize()
    assert isinstance(out.frames, list) and len(out.frames) == K and all(tuple(f.shape) == (1, F, 4, h, w) for f in out.frames)
    tensor = pipe(None, torch.stack([r[3][0] for r in reqs]), height=8 * h, width=8 * w, num_frames=F, num_inference_steps=steps, generator=gens(),
                  output_type="latent", image_embeddings=emb.to(d), image_latents=il.to(d), controlnet_cond_scale=IC.COND_SCALE,
                  independent_clips=True, return_dict=False)                                # the maps as one [K, F, 3, H, W] tensor
    assert all(torch.equal(a, b) for a, b in zip(out.frames, tensor))
    for k, g in enumerate(gens()):
        so = OS.OracleEulerDiscreteScheduler(**OS.SVD_SCHEDULER_CONFIG)
        so.set_timesteps(steps)
        lat0 = randn_tensor((1, F, 4, h, w), generator=g, device="cpu", dtype=torch.float32) * so.init_noise_sigma
        _, il_k, emb_k, cond_k = reqs[k]
        ref = OL.denoise(rig.cn_o, rig.unet_o, so, latents=lat0, image_latents=il_k.unsqueeze(1).repeat(1, F, 1, 1, 1), image_embeddings=emb_k,
                         controlnet_condition=cond_k, num_inference_steps=steps, controlnet_cond_scale=IC.COND_SCALE)
        r = P.rel_l2(out.frames[k], ref)
        print(f"__call__ with {K} requests, request {k}: rel-L2 {r:.3e} against the oracle chain on that request alone (bound {TOL_NET})")
        assert r < TOL_NET


# ------------------------------------------------------------------------------------------------- training
def oracle_mean_of_one_clip_steps(nets, batch, draws, use_spatial):
    """The MEAN over the clips of ``oracle.train.training_step_grads`` at B = 1: losses and every gradient."""
    from oracle import train as OT
    cn_o, un_o = nets[0], nets[1]
    lat, emb, mv, traj = batch
    B = lat.shape[0]
    outs = [OT.training_step_grads(cn_o, un_o, lat[b:b + 1], draws["noise"][b:b + 1], draws["sigmas"][b:b + 1], emb[b:b + 1], mv[b:b + 1],
                                   traj[b:b + 1], 0.18215, random_p=draws["random_p"][b:b + 1], conditioning_dropout_prob=DROP,
                                   ran_idx=draws["ran_idx"], use_spatial=use_spatial) for b in range(B)]
    mean = {k: sum(float(o[k]) for o in outs) / B for k in ("loss", "loss_temporal") + (("loss_spatial",) if use_spatial else ())}
    mean["grads"] = {k: sum(o["grads"][k] for o in outs) / B for k in outs[0]["grads"]}
    return mean


BOUNDS = dict(DROP_BOUNDS)
BOUNDS[(3, True)] = (DROP_BOUNDS[(3, True)][0], 8.60e-3)         # worst sizeable tensor: 1.25 x 6.88e-3 (the docstring below)


@pytest.mark.parametrize("use_spatial", [False, True], ids=["temporal", "spatial"])
@pytest.mark.parametrize("B", [2, 3])
def test_independent_batch_step_is_the_mean_of_the_oracles_one_clip_steps(nets, B, use_spatial):
    """Clips that differ in everything, dropout draws that hit some clips (``make_batch``); losses within 1e-3 and every gradient within
    ``DROP_BOUNDS`` of tests/test_train_batch_gpu.py for the same B - with ONE figure of its own (``BOUNDS``): the worst sizeable
    tensor at B = 3 with the spatial loss.  Measured (profiles/r18/independent_clips.txt): whole gradient 2.47e-3 / 2.56e-3 / 2.19e-3 /
    2.04e-3 for (2, temporal) / (2, spatial) / (3, temporal) / (3, spatial), all inside the coupled batch's bounds; worst tensor 6.71e-3 /
    6.58e-3 / 5.62e-3 / 6.88e-3, the last against a coupled bound of 5.60e-3 (1.25 x the coupled batch's 4.40 - 4.48e-3).  Why: that file's
    docstring measures the UNCHANGED one-clip step on the clip whose embedding and image latent are dropped at 6.6e-3 and 8.8e-3 for its
    worst tensor (fp16 roundings through an input half of whose channels are zero; the same in deterministic mode and at another loss
    scale), and the independent batch IS the mean of the one-clip steps, where the coupled batch mixes that clip's context into the
    others: one tensor (mid_block.resnets.0.spatial_res_block.conv1.weight) lies between its clips' figures, not under the coupled
    batch's.  Its bound is 1.25 x the measured 6.88e-3, the project's convention."""
    from tests.test_backward_gpu import _compare_grads
    batch, draws = make_batch(B)
    tr = trainer(nets, independent_clips=True)
    r = tr.loss_and_grads(*batch, use_spatial=use_spatial, **draws)
    ro = oracle_mean_of_one_clip_steps(nets, batch, draws, use_spatial)
    label = f"independent_clips, B = {B}, {'temporal + spatial' if use_spatial else 'temporal'} loss"
    keys = ("loss", "loss_temporal") + (("loss_spatial",) if use_spatial else ())
    for k in keys:
        print(f"{label}: {k} {r[k]:.6f} vs the mean of the one-clip oracle steps {ro[k]:.6f} ({abs(r[k] / ro[k] - 1):.1e})")
    total, worst = _compare_grads(tr.gradients(), ro["grads"], label)
    bt, bw = BOUNDS[(B, use_spatial)]
    print(f"{label}: whole gradient {total:.3e} (bound {bt}), worst sizeable tensor {worst:.3e} (bound {bw})")
    for k in keys:
        assert abs(r[k] / ro[k] - 1) < 1e-3
    assert total < bt and worst < bw


def test_training_no_leak_when_the_embedding_changes_too(nets, monkeypatch):
    """What the existing no-leak test cannot ask of the reference's batch: clip 1 gets a new EMBEDDING as well as new latents,
    trajectories, noise, sigma and motion value, and clip 0's rows of ``model_pred`` stay bit-identical.  Without the flag they change."""
    (lat, emb, mv, traj), draws = make_batch(2)
    draws = dict(draws, random_p=torch.tensor([0.7, 0.7]))
    (lat2, emb2, mv2, traj2), draws2 = make_batch(2, seed=77)
    mix = lambda a, b: torch.cat([a[:1], b[1:]])
    for flag in (True, False):
        preds = []
        for k in range(2):
            tr = trainer(nets, independent_clips=flag)
            run = tr.decoder.run
            monkeypatch.setattr(tr.decoder, "run", lambda *a, _run=run, **kw: preds.append(_run(*a, **kw)) or preds[-1])
            if k == 0:
                tr.loss_and_grads(lat, emb, mv, traj, use_spatial=False, **draws)
            else:
                tr.loss_and_grads(mix(lat, lat2), mix(emb, emb2), mix(mv, mv2), mix(traj, traj2), use_spatial=False,
                                  noise=mix(draws["noise"], draws2["noise"]), sigmas=torch.tensor([0.9, 0.5]), random_p=draws["random_p"], ran_idx=2)
        a, b = (p.v.view(2, -1, p.v.shape[-1]) for p in preds)
        assert torch.equal(a[0], b[0]) == flag and not torch.equal(a[1], b[1])


def test_one_clip_step_is_untouched_by_the_flag(nets):
    batch, draws = make_batch(1)
    plain, flagged = (trainer(nets, independent_clips=f).loss_and_grads(*batch, **draws) for f in (False, True))
    assert all(plain[k] == flagged[k] for k in ("loss", "loss_temporal", "loss_spatial"))


def test_gradient_checkpointing_at_two_independent_clips(nets):
    """Losses EQUAL, gradients within the floor of repeated plain steps (max(4 x floor, 1e-6)), as at two coupled clips."""
    batch, draws = make_batch(2)
    runs = {}
    for mode in (False, False, False, True):
        tr = trainer(nets, independent_clips=True, gradient_checkpointing=mode)
        runs.setdefault(mode, []).append((tr.loss_and_grads(*batch, **draws), flat(tr)))
    plain = [f for _, f in runs[False]]
    floor = max(rel(a, b) for i, a in enumerate(plain) for b in plain[:i])
    r, f = runs[True][0]
    d = min(rel(f, p) for p in plain)
    print(f"independent_clips, B = 2, gradient_checkpointing=True: vs the nearest plain step {d:.3e}; floor of 3 plain steps {floor:.3e}")
    assert all(r[k] == runs[False][0][0][k] for k in ("loss", "loss_temporal", "loss_spatial"))
    assert d <= max(4 * floor, 1e-6)


def test_deterministic_mode_at_two_independent_clips(nets):
    batch, draws = make_batch(2)
    runs = []
    for _ in range(2):
        tr = trainer(nets, independent_clips=True, deterministic=True, learning_rate=1e-4)
        r = tr.loss_and_grads(*batch, **draws)
        g = tr.params.grad.clone()
        assert tr.optimizer_step() is True
        runs.append((r, g, tr.params.flat.clone()))
    assert float(runs[0][1].abs().max()) > 0
    assert all(runs[0][0][k] == runs[1][0][k] for k in ("loss", "loss_temporal", "loss_spatial"))
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])


def test_accumulation_of_two_independent_two_clip_micro_batches(nets):
    """The sum rule at the bounds of the coupled test (whole gradient < 1e-3, worst sizeable tensor < 5e-3), clips keeping their
    conditioning for the reason given there."""
    from tests.test_backward_gpu import _compare_grads
    b1, d1 = make_batch(2, drop=False)
    b2, d2 = make_batch(2, seed=55, drop=False)
    single = []
    for b, d in ((b1, d1), (b2, d2)):
        tr = trainer(nets, independent_clips=True)
        tr.loss_and_grads(*b, **d)
        single.append({k: v.cpu() for k, v in tr.gradients().items()})
    two = trainer(nets, independent_clips=True, gradient_accumulation_steps=2)
    two.loss_and_grads(*b1, **d1)
    two.loss_and_grads(*b2, **d2)
    want = {k: 0.5 * (single[0][k] + single[1][k]) for k in single[0]}
    total, worst = _compare_grads(two.gradients(), want, "independent_clips: two accumulated two-clip micro-batches vs the mean of their gradients")
    assert total < 1e-3 and worst < 5e-3 and math.isfinite(total)


def test_captured_step_refuses_an_independent_batch(nets):
    batch, draws = make_batch(2)
    with pytest.raises(ValueError, match="use_graph.*one clip"):
        trainer(nets, independent_clips=True, use_graph=True).loss_and_grads(*batch, **draws)


# ------------------------------------------------------------------------------------------------- __call__: the stages around the loop
def test_call_stages_treat_every_request_as_a_call_of_its_own(dev):
    """The image path and the decode of ``__call__(independent_clips=True)``, with stand-ins for CLIP, the VAE and the loop: K = 2
    images through the resize, the encoder, the noise augmentation (generator k for request k, handed over as a TUPLE) and the VAE
    encode; ``output_type="pt"`` through the clip-by-clip decode.  Request k's embeddings, image latents, control maps, starting
    latents and frames equal what a call with request k alone (and generator k) gets.  The decoder stand-in subtracts the mean of the
    latents it is handed in one call, so a decode call that spanned two requests would show."""
    import types
    from posetraj_amd import EulerDiscreteScheduler, StableVideoDiffusionPipelineControlNet, SVD_SCHEDULER_CONFIG
    K, F, H = 2, 4, 64
    micro = dict(block_out_channels=(32, 32, 64, 64), num_attention_heads=(1, 1, 2, 2), cross_attention_dim=16, addition_time_embed_dim=8,
                 projection_class_embeddings_input_dim=24, layers_per_block=2, num_frames=F, in_channels=8)
    stub = types.SimpleNamespace(config=types.SimpleNamespace(**micro), device=dev)

    class Clip:                                               # per image: a function of that image's channel means
        dtype = torch.float32

        def __call__(self, x):
            v = x.float().cpu().mean(dim=(2, 3)).sum(1, keepdim=True)
            return types.SimpleNamespace(image_embeds=torch.sin(torch.arange(16)[None, :] * 0.37 + v) * 0.8)

    class Vae(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))
            self.config = types.SimpleNamespace(block_out_channels=(1, 1, 1, 1), scaling_factor=0.18215, force_upcast=False, out_channels=3)
            self.decode_calls = []

        @property
        def dtype(self):
            return self.p.dtype

        def encode(self, image):
            pooled = torch.nn.functional.avg_pool2d(image, 8)
            lat = torch.cat([pooled, pooled.mean(1, keepdim=True)], dim=1)
            return types.SimpleNamespace(latent_dist=types.SimpleNamespace(mode=lambda: lat))

        def decode(self, z, num_frames=None):
            self.decode_calls.append(z.shape[0])
            y = torch.nn.functional.interpolate((z - z.mean())[:, :3].float(), scale_factor=8.0, mode="nearest")
            return types.SimpleNamespace(sample=torch.tanh(y))

    def run(images, maps, gens, **kw):
        vae = Vae()
        pipe = StableVideoDiffusionPipelineControlNet(vae=vae, image_encoder=Clip(), unet=stub, controlnet=stub, scheduler=EulerDiscreteScheduler(**SVD_SCHEDULER_CONFIG))
        seen = {}

        def fake_denoise(lat, image_latents, image_embeddings, cond, *a, **k):
            seen.update(lat=lat.cpu(), il=image_latents.float().cpu(), emb=image_embeddings.float().cpu(), cond=cond.cpu(), kw=k)
            return lat * 0.01
        pipe.denoise = fake_denoise
        out = pipe(images, maps, height=H, width=H, num_frames=F, num_inference_steps=2, noise_aug_strength=0.05, generator=gens, output_type="pt",
                   decode_chunk_size=3, **kw)
        torch.cuda.synchronize()
        return out.frames, seen, vae.decode_calls

    g = torch.Generator().manual_seed(11)
    images = [torch.rand(3, H, H, generator=g) * 2 - 1 for _ in range(K)]
    maps = [torch.rand(F, 3, H, H, generator=g) * 2 - 1 for _ in range(K)]
    gens = lambda: tuple(torch.Generator().manual_seed(70 + k) for k in range(K))
    frames, seen, calls = run(images, maps, gens(), independent_clips=True, num_videos_per_prompt=None)
    assert seen["kw"]["independent_clips"] is True and isinstance(frames, list) and len(frames) == K
    assert tuple(seen["emb"].shape) == (2 * K, 1, 16) and tuple(seen["il"].shape) == (2 * K, 4, 8, 8) and tuple(seen["cond"].shape) == (2 * K, F, 3, H, H)
    assert float(seen["emb"][:K].abs().max()) == 0.0 and float(seen["il"][:K].abs().max()) == 0.0            # uncond halves first
    assert calls == [3, 1] * K                                                                                # 4 frames in chunks of 3, per request
    for k in range(K):
        f1, s1, _ = run(images[k][None], maps[k], gens()[k])
        assert torch.equal(seen["emb"][[k, K + k]], s1["emb"]) and torch.equal(seen["il"][[k, K + k]], s1["il"])
        assert torch.equal(seen["cond"][[k, K + k]], s1["cond"]) and torch.equal(seen["lat"][k:k + 1], s1["lat"])
        assert tuple(frames[k].shape) == (F, 3, H, H) and torch.equal(frames[k].cpu(), f1[0].cpu())
    assert not torch.equal(seen["emb"][K], seen["emb"][K + 1]) and not torch.equal(frames[0].cpu(), frames[1].cpu())
