"""CPU-side checks of the product: the C-ABI library loads (its contract with the headers: tests/test_abi_cpu.py), host-side
scheduler tables equal the reference goldens bit for bit, weight packing layouts, parameter inventory, error
behaviour without a GPU.  No compute kernel is called here."""
import json
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from posetraj_amd import hip
    hip.build()
    return hip.lib()


@pytest.mark.parametrize("struct, mirror", [("pt_igemm_params", "IgemmParams"), ("pt_ffn_params", "FfnParams"), ("pt_lnlin_params", "LnLinParams"),
                                            ("pt_conv_f32_params", "ConvF32Params"), ("pt_gemm_params", "GemmParams")])
def test_param_structs_match_header(struct, mirror):
    import ctypes
    from posetraj_amd import hip
    hdr = open(os.path.join(ROOT, "include", "posetraj_hip.h")).read()
    body = hdr[hdr.index("typedef struct %s {" % struct):hdr.index("} %s;" % struct)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split("{", 1)[1].split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ = re.match(r"(const\s+void\*|void\*|int32_t|int64_t|float)\s*(.*)", decl, flags=re.S)
        for n in typ.group(2).split(","):
            names.append(n.strip().lstrip("*").strip())
    assert names == [f[0] for f in getattr(hip, mirror)._fields_]
    assert ctypes.sizeof(getattr(hip, mirror)) % 8 == 0


def test_checked_handle_raises_where_the_raw_one_returns(lib):
    """hip.checked(): the status of every entry point that returns one is checked by ctypes itself (errcheck), with hip.check's
    message; entry points that return something else, and the raw handle hip.lib(), are untouched (which entry points carry
    errcheck: tests/test_abi_cpu.py)."""
    from posetraj_amd import hip
    L = hip.checked()
    bad = (None, 4, 64, None, 0, 0, 0, None, None, 1e-5, None, None)
    with pytest.raises(RuntimeError, match=r"^libposetraj_hip: pt_layernorm_f16 failed \(-?\d+\): .*null pointer"):
        L.pt_layernorm_f16(*bad)
    assert lib.pt_layernorm_f16(*bad) != 0
    assert L.pt_abi_version() == 10
    assert L.pt_prof_enable(0) == 0
    assert L.pt_groupnorm_scratch_floats(4096, 320, 2) == lib.pt_groupnorm_scratch_floats(4096, 320, 2) > 0


def test_header_parser_fails_loudly():
    """A declaration or type outside the subset raises, names the header it was told it reads and quotes the text; nothing is skipped."""
    from posetraj_amd import hip
    good = "#define PT_ABI_VERSION 3\nint pt_a(const float* x, void* stream);\n"
    core = hip.ABIS["core"]
    row = hip._parse_header(good, core, {})
    assert row.version == 3 and row.structs == {} and row.prototypes == {"pt_a": ("int", ["const float*", "void*"])} and row[:5] == core[:5]
    for bad, quoted in (("unsigned int pt_b(int32_t n);", "unsigned int pt_b"), ("int pt_b(int32_t);", "int32_t"), ("int pt_b(size_t n);", "size_t"),
                        ("typedef struct pt_x_params { int32_t n; } pt_x_params;", "pt_x_params"), ("int pt_b(int32_t n) { return pt_a(0, 0); }", "pt_b")):
        with pytest.raises(ValueError, match=r"^posetraj_hip\.h: .*" + re.escape(quoted)):
            hip._parse_header(good + bad + "\n", core, {})
    with pytest.raises(ValueError, match=r"^posetraj_det\.h: .*size_t"):          # ... whichever header that is
        hip._parse_header(good.replace("PT_ABI_VERSION", "PT_DET_ABI_VERSION") + "int ptd_b(size_t n);\n", hip.ABIS["det"], core.structs)
    with pytest.raises(ValueError, match=r"^posetraj_sampler\.h: no `#define PT_SAMPLER_ABI_VERSION n`"):
        hip._parse_header(good, hip.ABIS["sampler"], {})


def test_error_reporting_without_gpu(lib):
    from posetraj_amd import hip
    rc = lib.pt_layernorm_f16(None, 4, 64, None, 0, 0, 0, None, None, 1e-5, None, None)
    assert rc != 0 and b"null pointer" in lib.pt_last_error()
    with pytest.raises(RuntimeError):
        hip.check(rc, "pt_layernorm_f16")


def test_product_refuses_cpu_tensors():
    from posetraj_amd import EulerDiscreteScheduler, SVD_SCHEDULER_CONFIG, ops
    s = EulerDiscreteScheduler(**SVD_SCHEDULER_CONFIG)
    s.set_timesteps(2)
    with pytest.raises(RuntimeError):
        s.scale_model_input(torch.zeros(1, 2, 4, 4, 4), s.timesteps[0])
    with pytest.raises(RuntimeError):
        ops.silu(torch.zeros(4, dtype=torch.float16))
    from posetraj_amd.unet_spatio_temporal_condition_controlnet import UNetSpatioTemporalConditionControlNetModel as U
    u = U(block_out_channels=(64, 128, 256, 256), num_attention_heads=(1, 2, 4, 4))
    with pytest.raises(RuntimeError):
        u.load_state_dict({}, device="cpu")
    assert "oracle" not in "".join(open(os.path.join(ROOT, "posetraj_amd", f)).read()
                                   for f in os.listdir(os.path.join(ROOT, "posetraj_amd")) if f.endswith(".py")).replace(
        "CPU oracle", "")


SCHED_CFGS = {
    "eps_linspace": dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                         prediction_type="epsilon", timestep_spacing="linspace"),
    "v_trailing_karras": dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                              prediction_type="v_prediction", timestep_spacing="trailing", use_karras_sigmas=True),
}


@pytest.mark.parametrize("name", ["svd", "eps_linspace", "v_trailing_karras"])
@pytest.mark.parametrize("n", [2, 25])
def test_product_scheduler_tables_bit_exact(golden, name, n):
    from posetraj_amd import EulerDiscreteScheduler, SVD_SCHEDULER_CONFIG
    g = golden("sched")
    cfg = SVD_SCHEDULER_CONFIG if name == "svd" else SCHED_CFGS[name]
    k = f"{name}_n{n}_"
    s = EulerDiscreteScheduler(**cfg)
    assert np.array_equal(s.sigmas.numpy(), g[k + "init_sigmas"])
    assert np.array_equal(s.timesteps.numpy(), g[k + "init_timesteps"])
    assert float(s.init_noise_sigma) == float(g[k + "init_noise_sigma_before"])
    s.set_timesteps(n)
    assert np.array_equal(s.sigmas.numpy(), g[k + "sigmas"])
    assert np.array_equal(s.timesteps.numpy(), g[k + "timesteps"])
    assert float(s.init_noise_sigma) == float(g[k + "init_noise_sigma"])
    assert len(s) == 1000 and s.order == 1 and s.step_index is None


def test_scheduler_unknown_options_raise():
    from posetraj_amd import EulerDiscreteScheduler
    with pytest.raises(NotImplementedError):
        EulerDiscreteScheduler(beta_schedule="nope")
    s = EulerDiscreteScheduler(timestep_spacing="nope")
    with pytest.raises(ValueError):
        s.set_timesteps(3)


def test_param_inventory_matches_oracle_keys():
    """The product's parameter inventory (used to validate checkpoints) == the oracle modules' state-dict keys/shapes."""
    import contextlib, io
    from oracle import nets as ON
    from posetraj_amd import spec
    from posetraj_amd.controlnet_sdv import ControlNetSDVModel
    from posetraj_amd.unet_spatio_temporal_condition_controlnet import UNetSpatioTemporalConditionControlNetModel
    for cfg in (ON.tiny_config(), ON.svd_config()):
        with torch.device("meta"), contextlib.redirect_stdout(io.StringIO()):
            uo = ON.UNetSpatioTemporalConditionControlNetModel(**cfg)
            co = ON.ControlNetSDVModel(**cfg)
            cco = ON.ControlNetSDVModel(**cfg, camera=True)
        for prod, orc in ((UNetSpatioTemporalConditionControlNetModel(**cfg), uo), (ControlNetSDVModel(**cfg), co),
                          (ControlNetSDVModel(**cfg, camera=True), cco)):
            sp = prod.param_spec()
            sd = {k: tuple(v.shape) for k, v in orc.state_dict().items()}
            assert dict(sp) == sd
    assert spec.n_params(UNetSpatioTemporalConditionControlNetModel(**ON.svd_config()).param_spec()) == 1_524_623_082


def test_constructor_checks_match_reference_messages():
    from posetraj_amd.controlnet_sdv import ControlNetSDVModel
    with pytest.raises(ValueError, match="Must provide the same number of `block_out_channels`"):
        ControlNetSDVModel(block_out_channels=(320, 640))
    with pytest.raises(ValueError, match="Must provide the same number of `num_attention_heads`"):
        ControlNetSDVModel(num_attention_heads=(5, 10))


def test_packing_layouts():
    from posetraj_amd.packing import pack_conv2d, pack_conv_t3, pack_linear
    w = torch.arange(2 * 3 * 3 * 3, dtype=torch.float32).reshape(2, 3, 3, 3) / 64
    p = pack_conv2d(w, torch.tensor([1.0, 2.0]), "cpu")
    assert p.w.shape == (128, 128) and p.cin == 8 and p.K == 72 and p.N == 2
    # K order is (ky, kx, ci) with ci padded to 8
    assert p.w[1, (1 * 3 + 2) * 8 + 2] == w[1, 2, 1, 2].half()
    assert torch.all(p.w[:, 72:] == 0) and torch.all(p.w[2:] == 0) and p.bias[1] == 2.0
    wt = torch.randn(8, 8, 3, 1, 1)
    pt = pack_conv_t3(wt, None, "cpu")
    assert (pt.KH, pt.KW, pt.pad_h, pt.pad_w, pt.K) == (3, 1, 1, 0, 24)
    assert pt.w[5, 2 * 8 + 3] == wt[5, 3, 2, 0, 0].half()
    wl = torch.arange(64 * 4, dtype=torch.float32).reshape(64, 4)       # GEGLU: value rows 0..31, gate rows 32..63
    pg = pack_linear(wl, torch.arange(64, dtype=torch.float32), "cpu", geglu=True)
    assert pg.N == 64 and pg.n_out == 32
    assert torch.equal(pg.w[0:16, :4], wl[0:16].half()) and torch.equal(pg.w[16:32, :4], wl[32:48].half())
    assert torch.equal(pg.w[32:48, :4], wl[16:32].half()) and torch.equal(pg.w[48:64, :4], wl[48:64].half())
    assert pg.bias[16] == 32.0


def test_pipeline_from_pretrained_reads_scheduler_config(tmp_path):
    """``StableVideoDiffusionPipelineControlNet.from_pretrained(dir, controlnet=, unet=)`` - the construction at
    scripts/run_inference_vipseg_json_repro.py:335-339 - takes the sampler from <dir>/scheduler/scheduler_config.json."""
    import json
    from posetraj_amd import (ControlNetSDVModel, StableVideoDiffusionPipelineControlNet, SVD_SCHEDULER_CONFIG,
                              UNetSpatioTemporalConditionControlNetModel)
    from oracle import nets as ON
    cfg = dict(SVD_SCHEDULER_CONFIG, sigma_max=300.0, _class_name="EulerDiscreteScheduler", _diffusers_version="0.24.0")
    (tmp_path / "scheduler").mkdir()
    (tmp_path / "scheduler" / "scheduler_config.json").write_text(json.dumps(cfg))
    unet = UNetSpatioTemporalConditionControlNetModel(**ON.tiny_config())
    cn = ControlNetSDVModel(**ON.tiny_config())
    pipe = StableVideoDiffusionPipelineControlNet.from_pretrained(str(tmp_path), controlnet=cn, unet=unet)
    assert pipe.unet is unet and pipe.controlnet is cn
    pipe.scheduler.set_timesteps(25)
    assert abs(float(pipe.scheduler.sigmas[0]) - 300.0) < 1e-3
    with pytest.raises(ValueError):
        StableVideoDiffusionPipelineControlNet.from_pretrained(str(tmp_path), unet=unet)
    # secondary no-op API of the reference classes
    assert unet.attn_processors == {} and cn.attn_processors == {}
    unet.set_attn_processor(object()); cn.set_default_attn_processor(); unet._set_gradient_checkpointing(None, False)
    with pytest.raises(ValueError):
        cn.set_attn_processor({"a": 1})


def test_condition_preprocessing():
    """pipeline...:500: PIL frames -> [F, 3, H, W] in [-1, 1] at the requested size; tensors in [-1, 1] pass through."""
    import numpy as np
    import PIL.Image
    import torch
    from posetraj_amd import StableVideoDiffusionPipelineControlNet as Pipe
    rng = np.random.default_rng(0)
    frames = [PIL.Image.fromarray(rng.integers(0, 256, size=(32, 48, 3), dtype=np.uint8)) for _ in range(3)]
    x = Pipe.preprocess_condition(frames, height=32, width=48)
    assert tuple(x.shape) == (3, 3, 32, 48) and x.dtype == torch.float32
    want = torch.from_numpy(np.stack([np.asarray(f, dtype=np.float32) for f in frames])).permute(0, 3, 1, 2) / 255.0 * 2 - 1
    assert torch.allclose(x, want, atol=1e-6)
    y = Pipe.preprocess_condition(frames, height=16, width=24)
    assert tuple(y.shape) == (3, 3, 16, 24) and float(y.min()) >= -1.0 and float(y.max()) <= 1.0
    t = torch.rand(3, 3, 32, 48) * 2 - 1
    assert torch.equal(Pipe.preprocess_condition(t, 32, 48), t)
    u = torch.rand(3, 3, 32, 48)
    assert torch.allclose(Pipe.preprocess_condition(u, 32, 48), 2 * u - 1)


def test_bench_power_sampler_is_never_fatal(tmp_path):
    """bench.PowerSampler reads hwmon sysfs files that may be absent (this container) or unreadable: it reports None
    instead of raising, and picks the highest-median card when it cannot match the device's PCI address."""
    import time
    import bench
    ps = bench.PowerSampler.__new__(bench.PowerSampler)
    bench.PowerSampler.__init__(ps)                          # no GPU here: the PCI lookup fails silently
    ps.start()
    time.sleep(0.05)
    assert ps.result() is None or isinstance(ps.result(), dict)
    # two fake cards: the busier one (by median) is reported
    for name, vals in (("a", "250000000"), ("b", "1290000000")):
        (tmp_path / name).mkdir()
        (tmp_path / name / "power1_input").write_text(vals)
        (tmp_path / name / "power1_cap").write_text("1400000000")
    ps2 = bench.PowerSampler.__new__(bench.PowerSampler)
    bench.PowerSampler.__init__(ps2)
    ps2.files, ps2.mine = [str(tmp_path / "a" / "power1_input"), str(tmp_path / "b" / "power1_input")], None
    ps2.rows = [[ps2._read(f) for f in ps2.files] for _ in range(6)]
    r = ps2.result()
    assert r["median"] == 1290 and r["cap"] == 1400 and r["card"].startswith("highest")


def test_bench_dump_outputs_writes_float32_within_its_budget(tmp_path, monkeypatch):
    """bench.py --dump-outputs: the latents as float32 .npy, whole when they fit; above the budget a seeded sample that
    is the same in every run."""
    import numpy as np
    import torch
    import bench
    x = torch.randn(1, 14, 4, 8, 8, generator=torch.Generator().manual_seed(0)).to(torch.float16)
    bench.dump_outputs(str(tmp_path / "a"), x, 0, 1)
    a = np.load(tmp_path / "a" / "latents.npy")
    assert a.dtype == np.float32 and np.array_equal(a, x.float().numpy())
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), x, 1, 2)
    b, c = np.load(tmp_path / "b" / "latents_rank1.npy"), np.load(tmp_path / "c" / "latents_rank1.npy")
    assert b.dtype == np.float32 and b.nbytes == 2048 and np.array_equal(b, c)
    assert np.isin(b, x.float().numpy().reshape(-1)).all()


def test_non_cfg_branch_fails_like_the_reference(golden):
    """max_guidance_scale <= 1 (pipeline...:438,532): the reference doubles the control maps and added_time_ids
    unconditionally (:501-503, :521) and its ControlNet raises in add_embedding; the oracle's loop reaches the same error
    the same way and the product raises the same RuntimeError (no NotImplementedError of its own)."""
    import contextlib, io, types
    import torch
    from oracle import init as OI, loop as OL, nets as ON, sched as OS
    from posetraj_amd import EulerDiscreteScheduler, StableVideoDiffusionPipelineControlNet, SVD_SCHEDULER_CONFIG
    g = golden("loop")
    assert int(g["base_noncfg_raises"]) == 1 and int(g["cam_noncfg_raises"]) == 1
    want = str(g["base_noncfg_error"])
    micro = dict(block_out_channels=(32, 32, 64, 64), num_attention_heads=(1, 1, 2, 2), cross_attention_dim=16,
                 addition_time_embed_dim=8, projection_class_embeddings_input_dim=24, layers_per_block=2, num_frames=4)
    with contextlib.redirect_stdout(io.StringIO()):
        cn = OI.seeded_init_(ON.ControlNetSDVModel(**micro, conditioning_embedding_out_channels=(4, 8, 8, 16)), seed=31).eval()
        unet = OI.seeded_init_(ON.UNetSpatioTemporalConditionControlNetModel(**micro), seed=33).eval()
    s = OS.OracleEulerDiscreteScheduler(**OS.SVD_SCHEDULER_CONFIG)
    lat = torch.from_numpy(g["latents"])
    with pytest.raises(RuntimeError) as e_or:
        OL.denoise(cn, unet, s, latents=lat, image_latents=torch.zeros(1, 4, 4, 8, 8), image_embeddings=torch.zeros(1, 1, 16),
                   controlnet_condition=torch.cat([torch.from_numpy(g["cond"]).unsqueeze(0)] * 2), num_inference_steps=2,
                   min_guidance_scale=1.0, max_guidance_scale=1.0)
    assert str(e_or.value).splitlines()[0] == want
    stub = types.SimpleNamespace(config=types.SimpleNamespace(**micro), device="cpu")
    pipe = StableVideoDiffusionPipelineControlNet(unet=stub, controlnet=stub, scheduler=EulerDiscreteScheduler(**SVD_SCHEDULER_CONFIG))
    with pytest.raises(RuntimeError) as e_hip:
        pipe.denoise(lat, torch.zeros(1, 4, 8, 8), torch.zeros(1, 1, 16), torch.zeros(2, 4, 3, 64, 64), num_inference_steps=2,
                     min_guidance_scale=1.0, max_guidance_scale=1.0)
    assert str(e_hip.value) == want


def test_pipelined_igemm_kernels_do_not_spill(lib):
    """the 256 x 320 / 256 x 256 pipelined kernels live at the 256-VGPR limit; a spill inside their K loop
    is a scratch reload behind the LDS-DMA queue (a vmcnt(0) drain per reload).  hip.build() records hipcc's
    kernel-resource-usage remarks in posetraj_amd/build_resources.json: every tail variant of both kernels must show 0 VGPR
    spills and no scratch beyond the compiler's own SGPR-spill slots (round 2 shipped 39 / 34 spills with 112 / 96 B of scratch)."""
    import json, os
    from posetraj_amd import hip
    if not os.path.exists(hip.RESOURCES_PATH):
        pytest.skip("library was built elsewhere (no resource report next to it)")
    res = json.load(open(hip.RESOURCES_PATH))
    pipelined = {k: v for k, v in res.items() if "igemm8_kernel" in k or "igemm10_kernel" in k}
    assert len(pipelined) == 9 + 10, sorted(pipelined)
    for k, v in pipelined.items():
        assert v["VGPRs Spill"] == 0, (k, v)
        assert v["VGPRs"] <= 256 and v["Occupancy"] == 2, (k, v)


def test_oracle_attention_equals_sdpa():
    """The one hand-rolled leaf of oracle/blocks.py: Attention's chunked softmax(QK^T / sqrt(d)) V against
    F.scaled_dot_product_attention (the function diffusers' AttnProcessor2_0 dispatches to), self- and cross-attention,
    single-block and query-chunked paths."""
    import torch.nn.functional as F
    from oracle import blocks as OB
    torch.manual_seed(0)
    for (b, s, c, heads, xdim) in ((3, 40, 128, 2, None), (2, 9, 64, 1, 32), (1, 1500, 64, 1, None)):
        att = OB.Attention(c, heads, c // heads, xdim).eval()
        x = torch.randn(b, s, c)
        ctx = None if xdim is None else torch.randn(b, 1, xdim)
        with torch.no_grad():
            y = att(x, ctx)
            kv = x if ctx is None else ctx
            sp = lambda t: t.view(b, -1, heads, c // heads).transpose(1, 2)
            o = F.scaled_dot_product_attention(sp(att.to_q(x)), sp(att.to_k(kv)), sp(att.to_v(kv)))
            ref = att.to_out[0](o.transpose(1, 2).reshape(b, s, c))
        assert float((y - ref).abs().max()) < 1e-6 * max(1.0, float(ref.abs().max())), (b, s, c)


def test_randn_tensor_follows_the_diffusers_semantics():
    """one seeded generator must serve both the noise augmentation (CPU image) and prepare_latents (device latents):
    a CPU generator samples on the host (and the result is moved), a list of generators samples one batch entry each."""
    from posetraj_amd.pipeline_stable_video_diffusion_controlnet import randn_tensor
    a = randn_tensor((2, 3, 4), generator=torch.Generator().manual_seed(5), device="cpu", dtype=torch.float32)
    assert torch.equal(a, torch.randn((2, 3, 4), generator=torch.Generator().manual_seed(5)))
    gens = [torch.Generator().manual_seed(1), torch.Generator().manual_seed(2)]
    b = randn_tensor((2, 3, 4), generator=gens, device="cpu", dtype=torch.float32)
    assert torch.equal(b[0], torch.randn((1, 3, 4), generator=torch.Generator().manual_seed(1))[0])
    assert torch.equal(b[1], torch.randn((1, 3, 4), generator=torch.Generator().manual_seed(2))[0])
    c = randn_tensor((1, 5), generator=[torch.Generator().manual_seed(7)], device="cpu", dtype=torch.float32)
    assert torch.equal(c, torch.randn((1, 5), generator=torch.Generator().manual_seed(7)))


def test_track_file_format_round_trip(tmp_path):
    """The reference's trajectory file (dataset/VIPSeg/output_cotracker_all/*.json): {id: [[x, y], ...]}, key order = draw order."""
    import json
    from posetraj_amd import trajectory as T
    d = {"15": [[1085, 384], [1079, 381]], "0": [[3, 4], [5, 6]]}
    p = tmp_path / "t.json"
    p.write_text(json.dumps(d))
    got = T.load_tracks(str(p))
    assert list(got) == ["15", "0"] and got["15"][1] == [1079, 381]
    (tmp_path / "bad.json").write_text("[1, 2]")
    with pytest.raises(ValueError):
        T.load_tracks(str(tmp_path / "bad.json"))
    with pytest.raises(RuntimeError, match="ROCm device"):
        T.trajectory_maps(d, [32, 48], (64, 96, 3), num_frames=2, device="cpu")


def test_preprocess_condition_and_unit_tensor_scaling():
    """pil_to_numpy always divides by 255 (no data-dependent scaling); uint8 arrays are pixels, float arrays
    are already [0, 1] (VaeImageProcessor.preprocess)."""
    import numpy as np
    import PIL.Image
    from posetraj_amd import StableVideoDiffusionPipelineControlNet as Pipe
    dark = np.zeros((8, 8, 3), dtype=np.uint8); dark[0, 0] = 1                     # a near-black image whose maximum is 1
    t = Pipe._to_unit_tensor(PIL.Image.fromarray(dark))
    assert abs(float(t.max()) - 1 / 255) < 1e-9
    c = Pipe.preprocess_condition([dark], 8, 8)
    assert abs(float(c.max()) - (2 / 255 - 1)) < 1e-6 and float(c.min()) == -1.0
    f = Pipe.preprocess_condition([np.full((8, 8, 3), 0.5, dtype=np.float32)], 8, 8)
    assert float(f.abs().max()) == 0.0
    neg = torch.full((2, 3, 8, 8), -0.25)
    assert torch.equal(Pipe.preprocess_condition(neg, 8, 8), neg)                  # a tensor that already is in [-1, 1] passes through


def test_pipeline_call_signatures_keep_the_reference_positional_order():
    """Callers pass positionally: scripts/run_inference_vipseg_json_repro.py:451 `pipeline(image, maps, decode_chunk_size=...)`,
    infer/run_inference_vipseg_json_cam_concat_repro.py:496 `pipeline(image, maps, cam_parameter[:14], ...)` - camera_cond is
    the THIRD positional parameter of the _cam twin (..._cam.py:316-340) and absent from the base class's list (:316-340)."""
    import inspect
    from posetraj_amd.pipeline_stable_video_diffusion_controlnet import StableVideoDiffusionPipelineControlNet as Base
    from posetraj_amd.pipeline_stable_video_diffusion_controlnet_cam import StableVideoDiffusionPipelineControlNet as Cam
    ref = ["image", "controlnet_condition", "height", "width", "num_frames", "num_inference_steps", "min_guidance_scale",
           "max_guidance_scale", "fps", "motion_bucket_id", "noise_aug_strength", "decode_chunk_size", "num_videos_per_prompt",
           "generator", "latents", "output_type", "callback_on_step_end", "callback_on_step_end_tensor_inputs", "return_dict",
           "controlnet_cond_scale", "batch_size"]
    base = [p for p in inspect.signature(Base.__call__).parameters][1:]
    assert base[:len(ref)] == ref
    cam = [p for p in inspect.signature(Cam.__call__).parameters][1:]
    assert cam[:len(ref) + 1] == ref[:2] + ["camera_cond"] + ref[2:]
    d = {k: v.default for k, v in inspect.signature(Base.__call__).parameters.items()}
    assert (d["height"], d["width"], d["num_inference_steps"], d["max_guidance_scale"], d["fps"], d["motion_bucket_id"],
            d["output_type"], d["controlnet_cond_scale"]) == (576, 1024, 25, 3.0, 7, 127, "pil", 1.0)
    with pytest.raises(TypeError, match="must be real number, not NoneType"):
        Cam()(None, None)                                   # the reference's torch.tensor(None, dtype=torch.float32) (..._cam.py:505)


def test_param_store_layout_views_and_spans():
    """The trainer's flat parameter store (host logic only): tap-major convolution weights behind torch-shaped views, adjacent
    projections as one stacked matrix, 16-byte aligned spans, the fp16 mirror and the one-copy scalar cache."""
    from posetraj_amd import autodiff as AD
    g = torch.Generator().manual_seed(0)
    sd = {"conv.weight": torch.randn(6, 4, 3, 3, generator=g), "conv.bias": torch.randn(6, generator=g),
          "t.weight": torch.randn(8, 8, 3, 1, 1, generator=g), "q.weight": torch.randn(8, 16, generator=g), "k.weight": torch.randn(8, 16, generator=g),
          "v.weight": torch.randn(8, 16, generator=g), "mix": torch.tensor([0.25]), "zero.weight": torch.randn(8, 8, 1, 1, generator=g)}
    P = AD.ParamStore(sd, "cpu")
    for k, v in sd.items():
        assert tuple(P.value(k).shape) == tuple(v.shape) and torch.equal(P.value(k), v)
    assert P.layout("conv.weight") == (9, 6, 4) and P.layout("t.weight") == (3, 8, 8) and P.layout("q.weight") == (1, 8, 16) and P.layout("mix") is None
    raw = P.raw(P.flat, "conv.weight").view(9, 6, 4)                                         # tap-major: one [Co, Ci] matrix per tap
    assert torch.equal(raw[5], sd["conv.weight"][:, :, 1, 2]) and not P.value("conv.weight").is_contiguous()
    assert torch.equal(P.stacked(("q.weight", "k.weight", "v.weight")), torch.cat([sd["q.weight"], sd["k.weight"], sd["v.weight"]], 0))
    with pytest.raises(RuntimeError):
        P.stacked(("q.weight", "v.weight"))
    spans = P.spans()
    assert all(s % 8 == 0 for s, _ in spans.values()) and spans["conv.weight"][1] == 216 and P.numel % 8 == 0
    P.gradient("conv.weight").add_(1.0)                                                    # a write through the view lands in the flat buffer
    assert float(P.grad.sum()) == 216.0
    P.zero_grad()
    assert float(P.grad.abs().max()) == 0.0
    assert abs(P.scalar("mix") - 0.25) < 1e-7 and abs(AD.Mix(P, "mix").alpha() - 1 / (1 + 2.718281828 ** -0.25)) < 1e-6
    assert torch.equal(P.half_view("conv.bias"), sd["conv.bias"].half())
    out = P.state_dict()
    assert all(torch.equal(out[k], sd[k]) and out[k].is_contiguous() for k in sd)
    P.flat.mul_(2.0); P.version += 1                                                        # "an optimizer step": mirror and scalars follow
    assert torch.equal(P.half_view("conv.bias"), (2 * sd["conv.bias"]).half()) and abs(P.scalar("mix") - 0.5) < 1e-7
    assert AD._split_k(1, 100) == 1 and AD._split_k(4, 40320) == 78 and AD._split_k(2000, 40320) == 1 and AD._split_k(9, 2580480) == 455 and AD._split_k(81, 40320) == 12


# ------------------------------------------------------------------------------------------------- training loop host side
@pytest.mark.parametrize("name", ["constant", "constant_with_warmup", "linear", "cosine", "cosine_with_restarts", "polynomial"])
def test_lr_schedule_matches_the_published_lambda_schedules(name):
    """``train_state.get_scheduler`` against the same-named schedules of ``transformers.optimization`` (the formulas
    ``diffusers.optimization.get_scheduler`` - reference ``scripts/train_svd_traj_VIPSeg_14.py:1109`` - shares with it), stepped
    the way the loop steps them: one ``scheduler.step()`` after every ``optimizer.step()``."""
    topt = pytest.importorskip("transformers.optimization")
    from posetraj_amd import train_state
    W, T, base = 5, 40, 3e-4
    prm = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.AdamW([prm], lr=base)
    ref = topt.get_scheduler(name, opt, num_warmup_steps=W, num_training_steps=T)
    lam = train_state.get_scheduler(name, W, T, lr_init=base)
    for k in range(T + 6):
        assert base * lam(k) == pytest.approx(ref.get_last_lr()[0], rel=1e-12, abs=1e-18), (name, k)
        opt.step()
        ref.step()
    with pytest.raises(ValueError):
        train_state.get_scheduler("exponential")
    if name not in ("constant", "constant_with_warmup"):
        with pytest.raises(ValueError):
            train_state.get_scheduler(name, W)


def test_checkpoint_directory_rotation_and_resume_position(tmp_path):
    """``--checkpoints_total_limit`` / ``--resume_from_checkpoint`` bookkeeping (reference ``:1224-1247``, ``:1440-1462``)."""
    from posetraj_amd import train_state as TS
    out = str(tmp_path / "run")
    assert TS.list_checkpoints(out) == [] and TS.resolve_resume(out, "latest") is None and TS.resolve_resume(out, None) is None
    for step in (2000, 10000, 4000):
        os.makedirs(os.path.join(out, f"checkpoint-{step}"))
    os.makedirs(os.path.join(out, "logs"))
    assert TS.list_checkpoints(out) == ["checkpoint-2000", "checkpoint-4000", "checkpoint-10000"]      # numeric, not lexical
    assert TS.rotate_checkpoints(out, None) == [] and TS.rotate_checkpoints(out, 4) == []
    assert TS.rotate_checkpoints(out, 2) == ["checkpoint-2000", "checkpoint-4000"]                      # room for the one about to be written
    assert TS.list_checkpoints(out) == ["checkpoint-10000"] and os.path.isdir(os.path.join(out, "logs"))
    assert TS.resolve_resume(out, "latest") == os.path.join(out, "checkpoint-10000")
    assert TS.resolve_resume(out, "/elsewhere/checkpoint-10000/") == os.path.join(out, "checkpoint-10000")
    assert TS.resolve_resume(out, "checkpoint-77") is None
    # start_ft.sh: accumulation 2; say 3 500 optimizer steps per epoch
    assert TS.resume_position(os.path.join(out, "checkpoint-10000"), 2, 3500) == (10000, 2, 6000)


def test_trainer_state_files_round_trip(tmp_path):
    """``save_state`` / ``load_state`` over a CPU-resident parameter store (no kernels involved): file set, torch-layout
    tensors under the reference's names, strictness of the loader, counters."""
    import types
    from safetensors.torch import load_file
    from posetraj_amd import optim, train_state as TS
    from posetraj_amd.autodiff import ParamStore
    g = torch.Generator().manual_seed(0)
    sd = {"conv_in.weight": torch.randn(6, 5, 3, 3, generator=g), "conv_in.bias": torch.randn(6, generator=g),
          "mid.proj.weight": torch.randn(7, 6, generator=g), "mid.mix_factor": torch.tensor([0.25])}

    def trainer():
        P = ParamStore(sd, "cpu")
        opt = optim.AdamW(P, lr=1e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
        return types.SimpleNamespace(params=P, optimizer=opt, config={"in_channels": 5, "_name_or_path": "x"}, optimizer_steps=0, skipped_steps=0, loss_scale=65536.0,
                                     _clean=0, growth_interval=2000, _micro=0, _accum_scale=None, lr=1e-5, betas=(0.9, 0.999), weight_decay=1e-2,
                                     eps=1e-8, accumulation=2)
    a = trainer()
    a.optimizer.exp_avg.copy_(torch.randn(a.params.numel, generator=g))
    a.optimizer.exp_avg_sq.copy_(torch.rand(a.params.numel, generator=g))
    a.params.flat.mul_(1.5)
    a.optimizer_steps, a.skipped_steps, a.loss_scale, a._clean = 4000, 3, 32768.0, 17
    ck = str(tmp_path / "checkpoint-4000")
    TS.save_state(a, ck)
    w = load_file(os.path.join(ck, "controlnet", "diffusion_pytorch_model.safetensors"))
    assert set(w) == set(sd) and torch.equal(w["conv_in.weight"], sd["conv_in.weight"] * 1.5) and w["conv_in.weight"].is_contiguous()
    cfg = json.load(open(os.path.join(ck, "controlnet", "config.json")))
    assert cfg == {"in_channels": 5, "_class_name": "ControlNetSDVModel"}
    m = load_file(os.path.join(ck, "optimizer.safetensors"))
    assert set(m) == {f"{kind}.{k}" for kind in ("exp_avg", "exp_avg_sq") for k in sd}
    b = trainer()
    state = TS.load_state(b, ck)
    assert state["hyperparameters"]["gradient_accumulation_steps"] == 2
    assert (b.optimizer_steps, b.skipped_steps, b.loss_scale, b._clean, b._micro) == (4000, 3, 32768.0, 17, 0) and b.params.version == 1
    for k in sd:                                                  # padding between parameters is not part of the state
        for buf_a, buf_b in ((a.params.flat, b.params.flat), (a.optimizer.exp_avg, b.optimizer.exp_avg), (a.optimizer.exp_avg_sq, b.optimizer.exp_avg_sq)):
            assert torch.equal(a.params.raw(buf_a, k), b.params.raw(buf_b, k))
    a._micro = 1
    with pytest.raises(RuntimeError, match="accumulation cycle"):
        TS.save_state(a, str(tmp_path / "mid"))
    os.remove(os.path.join(ck, "trainer_state.json"))             # an interrupted save has no state file and does not load
    with pytest.raises(FileNotFoundError):
        TS.load_state(trainer(), ck)
    with pytest.raises(KeyError):
        b.params.load(b.params.flat, {k: v for k, v in sd.items() if k != "conv_in.bias"})
    with pytest.raises(ValueError):
        b.params.load(b.params.flat, dict(sd, **{"conv_in.bias": torch.zeros(7)}))


def test_the_librarys_tile_plan_on_the_committed_sweeps(lib):
    """tools/cfg_model_check.py asks the built library's own planner (pt_igemm_plan: choose_cfg + plan_splits, host only) for every
    shape of the committed sweeps: it picks the fastest measured configuration for all but one of the 60 shapes."""
    import contextlib, importlib.util, io
    spec = importlib.util.spec_from_file_location("cfg_model_check", os.path.join(ROOT, "tools", "cfg_model_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        mod.main([os.path.join(ROOT, "profiles", "r06", f"igemm_cfg_sweep_{w}_r06c.txt") for w in ("L", "M")])
    out = buf.getvalue()
    assert out.count("<- best") == 1, out[-2000:]


def test_igemm_plan_and_workspace_query_agree_without_a_gpu(lib):
    """pt_igemm_splitk_ws_bytes and pt_igemm_f16 share one planner: the workspace asked for is exactly what the plan splits into, and
    a call that offers none (ops.igemm(..., splitk=False)) runs un-split.  Host only, fake pointers: nothing is dereferenced."""
    import ctypes
    from posetraj_amd import hip
    p = hip.IgemmParams()
    p.x0 = p.w = p.out = 1 << 20
    M, N, K = 4032, 1280, 11520                                  # level 3's long reduction: split-K (profiles/r06)
    p.C0, p.ld0, p.Nimg, p.Hin, p.Win, p.Hout, p.Wout, p.KH, p.KW, p.stride = K, K, M, 1, 1, 1, 1, 1, 1, 1
    p.M, p.N, p.K, p.Kpad, p.ldo, p.out_scale = M, N, K, K, N, 1.0
    cfg, splits, gm = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    plan = lambda: hip.check(lib.pt_igemm_plan(ctypes.byref(p), ctypes.byref(cfg), ctypes.byref(splits), ctypes.byref(gm)), "pt_igemm_plan")
    plan()
    assert splits.value == 1 and gm.value >= 1
    need = lib.pt_igemm_splitk_ws_bytes(ctypes.byref(p))
    p.splitk_ws, p.splitk_ws_bytes = 1 << 20, need
    plan()
    assert cfg.value == 3 and splits.value > 1 and need == splits.value * M * N * 4
    p.splitk_ws_bytes = need - 1                                 # too small a workspace: un-split
    plan()
    assert splits.value == 1
    p.Kpad = K + 8                                               # invalid: reported, no plan, no workspace
    assert lib.pt_igemm_plan(ctypes.byref(p), None, None, None) != 0 and b"Kpad" in lib.pt_last_error()
    assert lib.pt_igemm_splitk_ws_bytes(ctypes.byref(p)) == 0


def test_product_behaviour_does_not_depend_on_the_environment():
    """Which kernels run is chosen by explicit library hooks and module constants (ops.dispatch_key is part of the pipeline's graph
    key), never by environment variables: a captured graph could not see those."""
    csrc = os.path.join(ROOT, "posetraj_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        if os.path.isfile(os.path.join(csrc, f)):
            assert "getenv" not in open(os.path.join(csrc, f)).read(), f
    for f in ("posetraj_amd/ops.py", "posetraj_amd/blocks.py", "oracle/quant.py"):
        assert "os.environ" not in open(os.path.join(ROOT, f)).read(), f
