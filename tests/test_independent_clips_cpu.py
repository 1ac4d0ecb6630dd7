"""``independent_clips`` (pipeline and trainer) and ``vec_mode`` 3 (include/posetraj_hip.h), the host side: the index algebra, the
library's argument checks, the inputs of the GPU tests held to the condition that makes them discriminating, and the host logic of the
flag.  No GPU."""
import ctypes
import inspect
import types

import numpy as np
import pytest
import torch

from tests import independent_clips as IC


# ------------------------------------------------------------------------------------------------- the index
def test_mode3_gives_every_clip_the_rows_of_a_call_of_its_own():
    """Every Bc in 1..4, F in 1..3, S in 1..7 (odd S included: the mid block at 320 x 576 has S = 5 x 9).  Row (half, c, f, s) must get
    table row ((half S + s) % 2) Bc + c - what clip c gets at Bc = 1 under mode 2, re-based into the halves-major batch table - and
    vG = 1 must be mode 2 on every row."""
    for Bc in range(1, 5):
        for F in range(1, 4):
            for S in range(1, 8):
                m = np.arange(2 * Bc * F * S)
                half, c, s = m // (Bc * F * S), (m // (F * S)) % Bc, m % S
                got = IC.mode3_index(m, Bc, F * S, S, 2 * Bc)
                alone = IC.mode2_index((half * F + (m // S) % F) * S + s, F * S, S, 2)        # the same token in a one-clip call
                assert np.array_equal(alone, (half * S + s) % 2)
                assert np.array_equal(got, alone * Bc + c), (Bc, F, S)
                assert got.min() >= 0 and got.max() < 2 * Bc
                for vB in (2 * Bc, Bc, 3 * Bc):                                                # vG = 1 is mode 2, whatever the table
                    assert np.array_equal(IC.mode3_index(m, 1, F * S, S, vB), IC.mode2_index(m, F * S, S, vB))
                # the trainer's frozen encoder: a batch without halves (vB = vG = B) - every row of clip b gets row b
                mb = np.arange(Bc * F * S)
                assert np.array_equal(IC.mode3_index(mb, Bc, F * S, S, Bc), mb // (F * S))
    # and the coupled index really is another one at Bc > 1 (what the flag is for)
    m = np.arange(2 * 2 * 2 * 5)
    assert not np.array_equal(IC.mode3_index(m, 2, 10, 5, 4), IC.mode2_index(m, 10, 5, 4))


def _plan(**kw):
    from posetraj_amd import hip
    p = hip.IgemmParams()
    p.x0 = p.w = p.out = p.vec = 256                  # never dereferenced: pt_igemm_plan is host only
    p.C0, p.ld0, p.ldo, p.ldv, p.N = 64, 64, 64, 64, 64
    p.Nimg, p.Hin, p.Win, p.Hout, p.Wout = 40, 1, 1, 1, 1
    p.KH, p.KW, p.stride = 1, 1, 1
    p.M, p.K, p.Kpad = 40, 64, 64
    p.vec_mode, p.vG, p.vFS, p.vS, p.vB = 3, 2, 10, 5, 4
    for k, v in kw.items():
        setattr(p, k, v)
    L = hip.lib()
    rc = L.pt_igemm_plan(ctypes.byref(p), None, None, None)
    ws = L.pt_igemm_splitk_ws_bytes(ctypes.byref(p))
    return rc, L.pt_last_error().decode(), ws


def test_library_checks_the_arguments_of_mode3_on_the_host():
    """``pt_igemm_plan`` / ``pt_igemm_splitk_ws_bytes`` share ``pt_igemm_f16``'s checks: vG >= 1, vB % vG == 0, vFS, vS, vB > 0, with a
    message that names the entry point and the mode."""
    assert _plan()[0] == 0
    assert _plan(vG=1)[0] == 0 and _plan(vG=4, vB=4)[0] == 0                               # mode 2 by algebra; a batch without halves
    for bad in (dict(vG=0), dict(vG=-1), dict(vB=3), dict(vB=0), dict(vFS=0), dict(vS=0), dict(vS=-5)):
        rc, said, ws = _plan(**bad)
        assert rc != 0 and "pt_igemm_f16" in said and "vec_mode 3" in said and ws == 0, (bad, said)
    assert _plan(vec_mode=2, vG=0)[0] == 0                                                  # vG stays unused in mode 2
    assert _plan(vec=None)[0] != 0                                                           # "vec_mode without vec", as for every mode


# ------------------------------------------------------------------------------------------------- the GPU tests' inputs discriminate
@pytest.mark.parametrize("Bc,F,h,w", IC.FORWARD_CASES)
def test_inputs_of_the_gpu_forward_test_separate_coupled_from_independent(Bc, F, h, w):
    """A condition on the inputs, not a measurement: on the fp32 oracle the REFERENCE's coupled batch prediction lies at least 10 x the
    GPU test's widest tolerance for that prediction (``IC.CHAINED_BOUND``, rel-L2 2.2e-3) from what every clip gets alone.  With it,
    tests/test_independent_clips_gpu.py cannot pass on a coupled result."""
    from tests import parity
    cn_o, unet_o = parity.build_oracle_nets(0)
    batch = IC.clip_batch(Bc, F, h, w)
    coupled = IC.oracle_prediction(cn_o, unet_o, batch)
    for c in range(Bc):
        alone = IC.oracle_prediction(cn_o, unet_o, IC.one_clip(batch, c))
        d = IC.rel_l2(IC.clip_rows(coupled, c), alone)
        print(f"Bc = {Bc}, F = {F}, {h} x {w}: clip {c} coupled vs alone rel-L2 {d:.3e} (needs >= {10 * IC.CHAINED_BOUND:.1e})")
        assert d >= 10 * IC.CHAINED_BOUND
    # and the changed clip of the no-leak test really is another clip, while the others are the same bits
    other = IC.clip_batch(Bc, F, h, w, change_clip=1)
    for k in ("sample", "ehs", "cond"):
        rows = [r for r in range(2 * Bc) if r % Bc != 1]
        assert torch.equal(other[k][rows], batch[k][rows])
    assert not torch.equal(other["ehs"][Bc + 1], batch["ehs"][Bc + 1]) and not torch.equal(other["sample"][1], batch["sample"][1])
    assert not torch.equal(other["cond"][1], batch["cond"][1])


# ------------------------------------------------------------------------------------------------- host logic
def _key(**kw):
    from posetraj_amd.step_graphs import GraphKey
    base = dict(Bc=2, F=4, hw=(8, 8), cond_shape=(4, 4, 3, 64, 64), cam_shape=None, kind="plain", scale=1.0, unet=1, controlnet=2, unet_gen=0,
                controlnet_gen=0, overlap=False, networks_name=None)
    independent = kw.pop("independent", False)
    return GraphKey(**dict(base, dispatch=(True, False) + (("independent_clips", independent),), **kw))


def test_graph_key_separates_the_two_modes():
    """``denoise`` puts the flag into the key's ``dispatch`` tuple, behind ``ops.dispatch_key()``."""
    from posetraj_amd.step_graphs import StepGraphs
    a, b = _key(), _key(independent=True)
    assert ("independent_clips", False) in a.dispatch and a != b and a.geometry() != b.geometry() and hash(a) != hash(b)
    graphs = StepGraphs()
    graphs.insert(a, types.SimpleNamespace(graph=None))
    assert graphs.get(b) is None and graphs.get(a) is not None
    graphs.insert(b, types.SimpleNamespace(graph=None))          # another geometry: the coupled graph is dropped, never replayed for it
    assert list(graphs) == [b]


def test_flag_defaults_and_documentation():
    from posetraj_amd import StableVideoDiffusionPipelineControlNet as Pipe
    from posetraj_amd.pipeline_stable_video_diffusion_controlnet_cam import StableVideoDiffusionPipelineControlNet as CamPipe
    from posetraj_amd.training import ControlNetTrainer
    for fn in (Pipe.denoise, Pipe.__call__, ControlNetTrainer.__init__):
        assert inspect.signature(fn).parameters["independent_clips"].default is False
    for doc in (Pipe.denoise.__doc__, Pipe.__call__.__doc__, CamPipe.__call__.__doc__, ControlNetTrainer.__doc__):
        assert "independent_clips" in doc
    for doc in (Pipe.denoise.__doc__, ControlNetTrainer.__doc__):
        assert "departure from the reference" in doc or "departs from the reference" in doc


def _host_pipe(num_frames=4):
    from posetraj_amd import StableVideoDiffusionPipelineControlNet as Pipe
    unet = types.SimpleNamespace(config=types.SimpleNamespace(num_frames=num_frames), device=torch.device("cpu"))
    return Pipe(unet=unet, controlnet=None, scheduler=None)


def test_call_checks_the_requests_before_any_stage_runs():
    """Every mismatch is a ``ValueError`` naming the argument; the stub pipeline has no network, encoder or scheduler to run."""
    pipe, F = _host_pipe(), 4
    img = [torch.zeros(3, 64, 64)] * 2
    maps = [torch.zeros(F, 3, 64, 64)] * 2
    gens = [torch.Generator().manual_seed(i) for i in range(2)]
    call = lambda **kw: pipe(**dict(dict(image=img, controlnet_condition=maps, height=64, width=64, generator=gens, independent_clips=True), **kw))
    for name, kw in (("image", dict(image=torch.zeros(2, 3, 64, 64))),
                     ("image", dict(image=[])),
                     ("controlnet_condition", dict(controlnet_condition=maps[:1])),
                     ("controlnet_condition", dict(controlnet_condition=torch.zeros(3, F, 3, 64, 64))),
                     ("controlnet_condition", dict(controlnet_condition=torch.zeros(F, 3, 64, 64))),
                     ("generator", dict(generator=gens + gens[:1])),
                     ("camera_cond", dict(camera_cond=torch.zeros(3, F, 12))),
                     ("camera_cond", dict(camera_cond=torch.zeros(F, 12))),
                     ("latents", dict(latents=torch.zeros(1, F, 4, 8, 8))),
                     ("image_embeddings", dict(image_embeddings=torch.zeros(2, 1, 64))),
                     ("image_latents", dict(image_latents=torch.zeros(2, 4, 8, 8))),
                     ("num_videos_per_prompt", dict(num_videos_per_prompt=2)),
                     ("control_weight", dict(control_weight=torch.ones(3, F, 8, 8)))):
        with pytest.raises(ValueError, match=name):
            call(**kw)
    # well-formed requests pass the checks (and fail later, at the first stage the stub lacks)
    with pytest.raises(Exception) as e:
        call(camera_cond=torch.zeros(2, F, 12), control_weight=torch.ones(2, F, 8, 8))
    assert not isinstance(e.value, ValueError)


def test_flag_is_refused_with_the_ab_schedule_hook_and_the_split_forward():
    from posetraj_amd import blocks
    pipe = _host_pipe()
    with pytest.raises(ValueError, match="independent_clips.*_networks"):
        pipe.denoise(None, None, None, None, _networks=lambda *a: None, independent_clips=True)
    t = torch.zeros(2, 8)
    with pytest.raises(ValueError, match="independent_clips"):
        blocks.Ctx(B=1, F=4, temb=t, xattn=t, half=0, xattn_full=t, clips=1, independent=True)
    with pytest.raises(ValueError, match="clips"):
        blocks.Ctx(B=4, F=4, temb=t, xattn=t, clips=3, independent=True)
    assert blocks.Ctx(B=4, F=4, temb=t, xattn=t).independent is False


def test_captured_training_step_still_refuses_a_batch_with_the_flag():
    """``loss_and_grads`` refuses before anything reaches a device; the trainer here is a shell with the attributes that path reads."""
    from posetraj_amd import training as T
    tr = object.__new__(T.ControlNetTrainer)
    tr.unet, tr.device, tr.config = None, torch.device("cpu"), {}
    tr.scaling_factor, tr.dropout, tr.use_graph, tr.independent_clips = 0.18215, None, True, True
    B, F, h, w = 2, 4, 8, 8
    with pytest.raises(ValueError, match="use_graph.*one clip"):
        tr.loss_and_grads(torch.zeros(B, F, 4, h, w), torch.zeros(B, 1, 16), torch.tensor([127.0, 60.0]), torch.zeros(B, F, 3, 8 * h, 8 * w),
                          use_spatial=False, noise=torch.zeros(B, F, 4, h, w), sigmas=torch.tensor([0.7, 1.9]), ran_idx=1)


# ------------------------------------------------------------------------------------------------- the kernels' register allocation
def test_kernels_that_existed_before_mode3_keep_their_resources():
    """igemm_tail.h (vec_index) and igemm.hip (launch, plan) as a check on the build's own report (hipcc's kernel-resource-usage
    remarks, posetraj_amd/build_resources.json): every kernel that existed before vec_mode 3 is compiled without its branch; mode 3 has
    one instance of its own per plain-loop kernel and of the split-K reducer, and none of a pipelined kernel.  Pinned: the figures of the
    two plain-loop kernels that sit on a register cliff (with the branch compiled in: 96 B of scratch and 14 spills, 127 VGPRs) and of
    the feed-forward kernels.  A compiler that allocates differently fails here instead of slowing the default path silently: a mismatch
    after a compiler change does not say the code is wrong - re-measure (resources of the parent commit and of the tree with that
    compiler, then clip time) and pin the new figures."""
    import json
    import os
    from posetraj_amd import hip
    if not os.path.exists(hip.RESOURCES_PATH):
        pytest.skip("library was built elsewhere (no resource report next to it)")
    res = json.load(open(hip.RESOURCES_PATH))
    plain = {k: v for k, v in res.items() if "igemm_kernelINS_3Cfg" in k}
    pick = lambda cfg, fast, clip: plain[f"_ZN12_GLOBAL__N_112igemm_kernelINS_3CfgI{cfg}EEELb{fast}ELb{clip}EEEvNS_7KParamsE"]
    big, n32 = "Li4ELi2ELi4ELi8ELi147456", "Li4ELi1ELi4ELi2ELi147456"
    figures = lambda v: (v["VGPRs"], v["AGPRs"], v["ScratchSize"], v["Occupancy"], v["VGPRs Spill"])
    assert figures(pick(big, 0, 0)) == (255, 0, 64, 2, 8)            # 256 x 256, generic K
    assert figures(pick(n32, 0, 0)) == (126, 0, 48, 4, 0)            # 256 x 32, generic K
    assert figures(pick(big, 0, 1))[3] == 2 and figures(pick(n32, 0, 1))[3] == 4         # mode 3's own instances: the same occupancy
    assert len(plain) == 9 + 9 and sum(k.endswith("ELb1EEEvNS_7KParamsE") for k in plain) == 9, sorted(plain)
    assert sum("splitk_reduce_kernel" in k for k in res) == 2
    assert sum("igemm8_kernel" in k or "igemm10_kernel" in k for k in res) == 9 + 10
    ffn = {k: figures(v) for k, v in res.items() if "ffn320_kernel" in k}
    name = lambda var, pre, st: f"_ZN12_GLOBAL__N_113ffn320_kernelILi{var}ELb{pre}ELb{st}EEEvNS_7FParamsE"
    assert ffn == {name(0, 0, 0): (251, 0, 0, 2, 0), name(1, 0, 0): (251, 0, 48, 2, 0), name(2, 0, 0): (251, 0, 48, 2, 0),
                   name(0, 1, 0): (256, 0, 92, 2, 22), name(1, 1, 0): (256, 0, 128, 2, 21), name(2, 1, 0): (256, 0, 128, 2, 21),
                   name(1, 0, 1): (256, 0, 80, 2, 9)}, ffn
