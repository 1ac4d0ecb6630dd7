"""Overlapping frame windows (``posetraj_amd.windows``, include/posetraj_window.h), the host side: the plan, the refusals, the add-on
library's header, build and exports, and a numpy model of the two kernels held to the direct formulas and to four planted faults.
No GPU: the library's entry points are called only with arguments they refuse before any launch."""
import ctypes
import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from tests import windows as TW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ the plan
@pytest.mark.parametrize("case,starts", TW.PLAN_CASES, ids=[str(c) for c, _ in TW.PLAN_CASES])
def test_plan_starts_cover_every_frame_and_weights_sum_to_one(case, starts):
    from posetraj_amd.windows import window_plan
    Ft, Fw, s = case
    plan = window_plan(Ft, Fw, s)
    assert list(plan.starts) == starts and plan.K == len(starts) == -(-(Ft - Fw) // s) + 1
    assert (plan.num_frames, plan.window_frames, plan.window_stride) == case
    assert plan.starts[-1] + Fw == Ft and plan.starts[0] == 0
    assert plan.weights.dtype == np.float32 and plan.weights.shape == (plan.K, Fw)
    assert np.array_equal(plan.weights, TW.direct_weights(Ft, Fw, starts))
    assert (plan.weights > 0).all()
    cover = TW.covering(Ft, Fw, starts)
    for f, ks in enumerate(cover):
        assert ks, f"frame {f} is not covered"
        total = sum(np.float64(plan.weights[k, f - starts[k]]) for k in ks)
        assert abs(total - 1.0) <= 2.0 ** -23 * len(ks), (f, ks, total)
        if len(ks) == 1:
            assert plan.weights[ks[0], f - starts[ks[0]]] == np.float32(1.0)
    if case == (9, 4, 2):                                                   # frames covered by 1, 2 and 3 windows
        assert sorted(set(len(ks) for ks in cover)) == [1, 2, 3]


def test_plan_refusals_name_the_argument():
    from posetraj_amd.windows import resolve, window_plan
    for name, args in (("window_frames", (7, 0, 1)), ("window_frames", (7, 8, 1)), ("window_frames", (7, 3.5, 1)), ("window_stride", (7, 4, 0)),
                       ("window_stride", (7, 4, 5)), ("window_stride", TW.TOO_MANY), ("num_frames", (7.5, 4, 2))):
        with pytest.raises(ValueError, match=name):
            window_plan(*args)
    assert window_plan(64, 1, 1).K == 64 and window_plan(*TW.LAST_ACCEPTED).K == 64      # K = 64 is the last one accepted
    with pytest.raises(ValueError, match="64"):
        window_plan(*TW.TOO_MANY)
    # defaults of the arguments: stride Fw // 2, at least 1; batch K; a batch must divide K
    plan, G = resolve(28, 14)
    assert (plan.window_stride, list(plan.starts), G) == (7, [0, 7, 14], 3)
    assert resolve(3, 1)[0].window_stride == 1
    assert resolve(9, 4, 2, 2)[1] == 2 and resolve(9, 4, 2, 1)[1] == 1
    for bad in (3, 0, -1, 8):
        with pytest.raises(ValueError, match="window_batch"):
            resolve(9, 4, 2, bad)


def _host_pipe(num_frames=7):
    from posetraj_amd import StableVideoDiffusionPipelineControlNet as Pipe
    unet = types.SimpleNamespace(config=types.SimpleNamespace(num_frames=num_frames), device=torch.device("cpu"))
    return Pipe(unet=unet, controlnet=None, scheduler=None)


def test_denoise_and_call_refuse_before_any_stage_runs():
    """The stub pipeline has no network, encoder or scheduler to run: whatever is not refused first fails at one of them."""
    pipe = _host_pipe()
    lat = torch.zeros(1, 7, 4, 8, 8)
    den = lambda latents=lat, **kw: pipe.denoise(latents, torch.zeros(2, 4, 8, 8), torch.zeros(2, 1, 64), torch.zeros(2, 7, 3, 64, 64), **kw)
    for name, kw in (("window_frames", dict(window_stride=2)), ("window_frames", dict(window_batch=1)),
                     ("independent_clips", dict(window_frames=4, independent_clips=True)),
                     ("_networks", dict(window_frames=4, _networks=lambda *a: None)),
                     ("latents", dict(window_frames=4, latents=torch.zeros(2, 7, 4, 8, 8))),
                     ("window_frames", dict(window_frames=8)), ("window_frames", dict(window_frames=0)),
                     ("window_stride", dict(window_frames=4, window_stride=5)), ("window_stride", dict(window_frames=4, window_stride=0)),
                     ("window_batch", dict(window_frames=4, window_stride=1, window_batch=3))):
        with pytest.raises(ValueError, match=name):
            den(**kw)
    with pytest.raises(ValueError, match="controlnet_condition"):
        pipe.denoise(lat, torch.zeros(2, 4, 8, 8), torch.zeros(2, 1, 64), torch.zeros(2, 6, 3, 64, 64), window_frames=4)
    with pytest.raises(ValueError, match="camera_cond"):
        den(window_frames=4, camera_cond=torch.zeros(2, 4, 12))
    with pytest.raises(ValueError, match="control_weight"):
        den(window_frames=4, control_weight=torch.ones(4, 8, 8))                           # [Ft, h, w] is wanted, not [Fw, h, w]
    with pytest.raises(Exception) as e:                                                    # well-formed: fails later, at the stub
        den(window_frames=4, window_stride=3, window_batch=1, control_weight=torch.ones(7, 8, 8))
    assert not isinstance(e.value, ValueError)
    call = lambda **kw: pipe(**dict(dict(image=torch.zeros(1, 3, 64, 64), controlnet_condition=torch.zeros(7, 3, 64, 64), height=64, width=64,
                                         window_frames=4), **kw))
    for name, kw in (("batch_size", dict(batch_size=2)), ("num_videos_per_prompt", dict(num_videos_per_prompt=2)),
                     ("independent_clips", dict(independent_clips=True)), ("window_frames", dict(window_frames=9)),
                     ("window_stride", dict(window_stride=5)), ("window_batch", dict(window_batch=5)),
                     ("window_frames", dict(window_frames=None, window_stride=2)),
                     ("window_stride", dict(num_frames=TW.TOO_MANY[0], window_frames=2, window_stride=1)),
                     ("control_weight", dict(control_weight=torch.ones(4, 8, 8)))):
        with pytest.raises(ValueError, match=name):
            call(**kw)
    with pytest.raises(Exception) as e:
        call(control_weight=torch.ones(7, 8, 8))
    assert not isinstance(e.value, ValueError)


def test_defaults_are_off_and_documented():
    from posetraj_amd import StableVideoDiffusionPipelineControlNet as Pipe
    from posetraj_amd.pipeline_stable_video_diffusion_controlnet_cam import StableVideoDiffusionPipelineControlNet as CamPipe
    for fn in (Pipe.denoise, Pipe.__call__):
        p = inspect.signature(fn).parameters
        assert [p[n].default for n in ("window_frames", "window_stride", "window_batch")] == [None, None, None]
        assert list(p)[-3:] == ["window_frames", "window_stride", "window_batch"]          # appended
        assert "window_frames" in fn.__doc__ and "same first image" in fn.__doc__
    assert "kw" in inspect.signature(CamPipe.__call__).parameters and "window_frames" in CamPipe.__call__.__doc__
    assert CamPipe.denoise is Pipe.denoise


def test_step_state_without_a_plan_is_what_it_was():
    from posetraj_amd.step_graphs import StepState
    st = StepState("plain", None)
    assert st.windows is None and list(inspect.signature(StepState.__init__).parameters) == ["self", "kind", "run", "key", "windows"]
    assert inspect.signature(StepState.__init__).parameters["windows"].default is None


# ------------------------------------------------------------------------------------------------------------------ the library
@pytest.fixture(scope="module")
def hip():
    from posetraj_amd import hip
    hip.build()
    return hip


NAMES = {"ptw_abi_version", "ptw_last_error", "ptw_scale_concat_windows", "ptw_cfg_window_merge"}


def test_the_header_reads_into_exactly_the_four_entry_points(hip):
    text = open(os.path.join(ROOT, "include", "posetraj_window.h")).read()
    abi = hip._parse_header(text, hip._WINDOW_ROW, {})
    assert set(abi.signatures) == set(abi.prototypes) == NAMES == set(hip.WINDOW_ABI.signatures)
    assert (abi.version, abi.prefix, abi.macro, abi.structs) == (1, "ptw_", "PT_WINDOW_ABI_VERSION", {})
    assert re.search(r"^#define\s+PT_WINDOW_ABI_VERSION\s+1\s*$", text, flags=re.M)
    assert abi.prototypes["ptw_last_error"] == ("const char*", []) and abi.signatures["ptw_last_error"][0] is ctypes.c_char_p
    assert abi.prototypes["ptw_scale_concat_windows"][1] == ["const float*", "const void*", "float", "const int32_t*", "int32_t", "int32_t", "int32_t",
                                                             "int32_t", "int32_t", "void*", "void*"]
    assert abi.prototypes["ptw_cfg_window_merge"][1] == ["const void*", "int32_t", "int32_t", "const float*", "const float*", "const int32_t*",
                                                         "int32_t", "int32_t", "int32_t", "int32_t", "int32_t", "float*", "void*"]


def test_the_main_librarys_tables_do_not_know_the_window_library(hip):
    assert "window" not in hip.ABIS and all(a.prefix != "ptw_" for a in hip.ABIS.values())
    assert not any("window" in os.path.basename(p) for p in hip.header_paths())
    assert not any("window" in s for s in hip.SOURCES) and hip.WINDOW_SOURCE == "window.hip"
    assert os.path.exists(os.path.join(hip.CSRC, hip.WINDOW_SOURCE))
    assert not any(n.startswith("ptw_") for a in hip.ABIS.values() for n in a.signatures)


def test_the_built_library_loads_and_exports_only_its_own_names(hip):
    assert os.path.exists(hip.WINDOW_LIB_PATH) and os.path.basename(hip.WINDOW_LIB_PATH) == "libposetraj_window.so"
    assert os.path.dirname(hip.WINDOW_LIB_PATH) == os.path.dirname(hip.LIB_PATH)
    L = hip.window()
    assert L.ptw_abi_version() == 1 == hip.WINDOW_ABI.version
    out = subprocess.run(["nm", "-D", "--defined-only", hip.WINDOW_LIB_PATH], capture_output=True, text=True, check=True).stdout
    named = {ln.split()[-1] for ln in out.splitlines() if ln.split() and re.match(r"^pt[a-z]?_", ln.split()[-1])}
    assert named == NAMES
    undefined = subprocess.run(["nm", "-D", "--undefined-only", hip.WINDOW_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not re.search(r"\bpt[a-z]?_\w+", undefined)                                     # nothing of the main library is needed
    main = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "ptw_" not in main


def test_invalid_plans_are_refused_with_the_entry_points_name_before_any_launch(hip):
    """The checked handle raises ``RuntimeError`` with the library's message; the raw status is non-zero.  Pointers are dummies: a
    refused call dereferences none of them and launches nothing."""
    L = hip.window()
    raw = ctypes.CDLL(hip.WINDOW_LIB_PATH)
    for name, (res, args) in hip.WINDOW_ABI.signatures.items():
        getattr(raw, name).restype, getattr(raw, name).argtypes = res, args
    arr = lambda v: (ctypes.c_int32 * len(v))(*v)
    bad = [([1, 3], 4, 7), ([0, 4], 4, 7), ([0, 5], 4, 9), ([0, 3, 3], 4, 7), ([0, 2], 4, 7), ([0], 0, 7), ([0], 8, 7), ([0] * 65, 4, 7), ([], 4, 7)]
    for starts, Fw, Ft in bad:
        a = arr(starts or [0])
        rc = raw.ptw_scale_concat_windows(256, 256, 1.0, a, len(starts), Fw, Ft, 8, 8, 256, None)
        assert rc != 0 and "ptw_scale_concat_windows" in raw.ptw_last_error().decode(), (starts, Fw, Ft)
        rc = raw.ptw_cfg_window_merge(256, 1, 4, 256, 256, a, len(starts), Fw, Ft, 8, 8, 256, None)
        assert rc != 0 and "ptw_cfg_window_merge" in raw.ptw_last_error().decode(), (starts, Fw, Ft)
        with pytest.raises(RuntimeError, match="ptw_cfg_window_merge"):
            L.ptw_cfg_window_merge(256, 1, 4, 256, 256, a, len(starts), Fw, Ft, 8, 8, 256, None)
    assert raw.ptw_cfg_window_merge(256, 1, 3, 256, 256, arr([0, 3]), 2, 4, 7, 8, 8, 256, None) != 0 and "ldn" in raw.ptw_last_error().decode()
    assert raw.ptw_cfg_window_merge(None, 1, 4, 256, 256, arr([0, 3]), 2, 4, 7, 8, 8, 256, None) != 0
    assert raw.ptw_scale_concat_windows(256, 256, 1.0, None, 2, 4, 7, 8, 8, 256, None) != 0
    assert raw.ptw_scale_concat_windows(256, 256, 1.0, arr([0, 3]), 2, 4, 7, 0, 8, 256, None) != 0
    assert raw.ptw_scale_concat_windows(256, 256, float("nan"), arr([0, 3]), 2, 4, 7, 8, 8, 256, None) != 0


# ------------------------------------------------------------------------------------------------------------------ the kernels' model
def _merge_case(case, starts, f16, ldn, seed, h=2, w=3):
    Ft, Fw, _ = case
    rng = np.random.default_rng(seed)
    K = len(starts)
    pred = rng.standard_normal((2 * K, Fw, h, w, ldn)).astype(np.float32)
    pred = pred.astype(np.float16) if f16 else pred
    guidance = np.linspace(1.0, 3.0, Fw).astype(np.float32)
    return pred, guidance, TW.direct_weights(Ft, Fw, starts)


@pytest.mark.parametrize("case,starts", TW.PLAN_CASES, ids=[str(c) for c, _ in TW.PLAN_CASES])
def test_numpy_model_of_both_kernels_equals_the_direct_formulas(case, starts):
    Ft, Fw, _ = case
    rng = np.random.default_rng(Ft * 100 + Fw)
    lat = (rng.standard_normal((Ft, 4, 2, 3)) * 30).astype(np.float32)
    il = rng.standard_normal((2, 4, 2, 3)).astype(np.float16)
    for sigma in (700.0, 1.5, 0.002):
        assert np.array_equal(TW.gather_model(lat, il, sigma, starts, Fw), TW.gather_direct(lat, il, sigma, starts, Fw))
    for f16 in (False, True):
        for ldn in (4, 8):
            pred, g, wts = _merge_case(case, starts, f16, ldn, seed=ldn + f16)
            want = TW.merge_reference(torch.from_numpy(pred), torch.from_numpy(g), torch.from_numpy(wts), starts, Ft).numpy()
            assert np.array_equal(TW.merge_model(pred, g, wts, starts, Ft), want)


def test_four_planted_faults_are_each_noticed():
    """On the (9, 4, 2) plan (frames under 1, 2 and 3 windows): weights that are not normalised, the covering windows summed in
    descending order (fp32 addition does not commute over three terms of this data), the guidance indexed by the long video's frame,
    the two halves exchanged."""
    case, starts = TW.PLAN_CASES[2]
    Ft, Fw, _ = case
    pred, g, wts = _merge_case(case, starts, False, 4, seed=11)
    want = TW.merge_reference(torch.from_numpy(pred), torch.from_numpy(g), torch.from_numpy(wts), starts, Ft).numpy()
    assert np.array_equal(TW.merge_model(pred, g, wts, starts, Ft), want)
    tri = np.minimum(np.arange(Fw) + 1, Fw - np.arange(Fw)).astype(np.float32)
    raw_weights = np.stack([tri] * len(starts))
    assert not np.array_equal(TW.merge_model(pred, g, raw_weights, starts, Ft), want)
    desc = TW.merge_model(pred, g, wts, starts, Ft, descending=True)
    three = [f for f, ks in enumerate(TW.covering(Ft, Fw, starts)) if len(ks) == 3]
    assert three and not np.array_equal(desc[three], want[three])
    assert np.allclose(desc, want, rtol=0, atol=1e-5)                                    # ... and differs by rounding only
    assert not np.array_equal(TW.merge_model(pred, g, wts, starts, Ft, global_guidance=True), want)
    assert not np.array_equal(TW.merge_model(pred, g, wts, starts, Ft, swap_halves=True), want)
    # the gather's planted fault: halves exchanged shows in channels 4..7
    rng = np.random.default_rng(3)
    lat, il = rng.standard_normal((Ft, 4, 2, 3)).astype(np.float32), rng.standard_normal((2, 4, 2, 3)).astype(np.float16)
    good = TW.gather_direct(lat, il, 1.5, starts, Fw)
    assert not np.array_equal(TW.gather_model(lat, il[::-1].copy(), 1.5, starts, Fw), good)
