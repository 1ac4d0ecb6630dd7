"""Control window, per-step scale and spatial control weights, the host side (``posetraj_amd.control_schedule``): diffusers' window
rule, the validation of the three arguments, the pooling of a weight map to the ControlNet's tap sizes, and the control-weight
extension of the C ABI (include/posetraj_control.h) as ``posetraj_amd.hip`` reads it.  No device."""
import inspect

import pytest
import torch

from posetraj_amd import control_schedule as CS


def keep(n, start, end):
    """diffusers' ``controlnet_keep``, written out."""
    return [not (i / n < start or (i + 1) / n > end) for i in range(n)]


@pytest.mark.parametrize("n", [4, 5, 25])
@pytest.mark.parametrize("window", [(0.0, 1.0), (0.0, 0.5), (0.5, 1.0), (0.25, 0.75), (0.1, 0.15)])
def test_control_plan_follows_diffusers_window_rule(n, window):
    """Step i of N keeps the ControlNet iff ``not (i / N < start or (i + 1) / N > end)``.  (0.1, 0.15) is a window that contains no
    step at any of these N (a step is at least 1 / 25 wide and would have to start at or after 0.1 and end by 0.15: step 2 of 25
    starts at 0.08, step 3 ends at 0.16): every step is off."""
    plan = CS.control_plan(n, 0.9, *window)
    assert len(plan) == n and all(isinstance(on, bool) and s == 0.9 for on, s in plan)
    assert [on for on, _ in plan] == keep(n, *window)
    if window == (0.0, 1.0):
        assert all(on for on, _ in plan)
    if window == (0.1, 0.15):
        assert not any(on for on, _ in plan)
    hand = {(4, (0.0, 0.5)): [1, 1, 0, 0], (4, (0.5, 1.0)): [0, 0, 1, 1], (4, (0.25, 0.75)): [0, 1, 1, 0], (5, (0.0, 0.5)): [1, 1, 0, 0, 0],
            (5, (0.5, 1.0)): [0, 0, 0, 1, 1], (5, (0.25, 0.75)): [0, 0, 1, 0, 0]}
    if (n, window) in hand:
        assert [int(on) for on, _ in plan] == hand[(n, window)]


def test_control_plan_per_step_scales_and_zero_entries():
    plan = CS.control_plan(4, [0.3, 0.0, 0.5, 0.9])
    assert plan == [(True, 0.3), (False, 0.0), (True, 0.5), (True, 0.9)]             # scale exactly 0: like a step outside the window
    assert CS.control_plan(4, (0.3, 0.9, 0.5, 0.9), 0.0, 0.75) == [(True, 0.3), (True, 0.9), (True, 0.5), (False, 0.9)]
    assert CS.control_plan(4, torch.tensor([0.5, 0.5, 0.0, 1.0]), 0.5, 1.0) == [(False, 0.5), (False, 0.5), (False, 0.0), (True, 1.0)]
    assert CS.control_plan(3, 0.0) == [(False, 0.0)] * 3
    assert CS.control_plan(2, 1) == [(True, 1.0)] * 2 and CS.control_plan(2) == [(True, 1.0)] * 2
    assert CS.is_scale_sequence([1.0]) and CS.is_scale_sequence(torch.ones(3)) and not CS.is_scale_sequence(0.9)
    assert not CS.is_scale_sequence(torch.tensor(0.9)) and not CS.is_scale_sequence(1)


@pytest.mark.parametrize("args,name", [
    ((4, [0.9, 0.9, 0.9]), "controlnet_cond_scale"),                  # wrong length
    ((4, [0.9] * 5), "controlnet_cond_scale"),
    ((4, []), "controlnet_cond_scale"),
    ((4, float("nan")), "controlnet_cond_scale"),                     # non-finite
    ((4, [0.9, float("nan"), 0.9, 0.9]), "controlnet_cond_scale"),
    ((4, [0.9, float("inf"), 0.9, 0.9]), "controlnet_cond_scale"),
    ((4, 0.9, 0.5, 0.5), "control_guidance_start"),                   # start >= end
    ((4, 0.9, 0.75, 0.25), "control_guidance_start"),
    ((4, 0.9, -0.1, 1.0), "control_guidance_start"),                  # start < 0
    ((4, 0.9, 0.0, 1.5), "control_guidance_end"),                     # end > 1
    ((4, 0.9, 0.0, float("nan")), "control_guidance_end"),
    ((4, 0.9, None, 1.0), "control_guidance_start"),
    ((0, 0.9), "num_inference_steps"),
])
def test_control_plan_refuses_bad_arguments_by_name(args, name):
    with pytest.raises(ValueError, match=name):
        CS.control_plan(*args)


def test_control_weight_validation():
    F, h, w = 14, 8, 8
    one = CS.check_control_weight(torch.rand(F, h, w), 1, F, h, w)
    assert one.dtype == torch.float32 and tuple(one.shape) == (1, F, h, w)
    two = CS.check_control_weight(torch.rand(F, h, w).double(), 2, F, h, w)                   # [F, h, w]: every clip gets the map
    assert tuple(two.shape) == (2, F, h, w) and torch.equal(two[0], two[1])
    per_clip = torch.rand(2, F, h, w)
    assert torch.equal(CS.check_control_weight(per_clip, 2, F, h, w), per_clip)
    assert CS.check_control_weight(None, 1, F, h, w) is None
    assert tuple(CS.check_control_weight(torch.rand(F, h, w).numpy(), 1, F, h, w).shape) == (1, F, h, w)
    s = torch.linspace(0, 1, F)                                                                # per-frame strength, the documented form
    pf = CS.check_control_weight(s[:, None, None].expand(F, h, w), 1, F, h, w)
    assert torch.equal(pf[0, :, 3, 5], s)
    assert float(CS.check_control_weight(torch.full((F, h, w), -2.5), 1, F, h, w).min()) == -2.5      # any finite value is allowed
    bad = [torch.rand(h, w), torch.rand(1, 1, F, h, w), torch.rand(F + 1, h, w), torch.rand(F, h, w + 1), torch.rand(2, F, h, w),
           torch.rand(F, 8 * h, 8 * w)]
    for cw in bad:                                                                             # wrong rank / wrong size (1 clip)
        with pytest.raises(ValueError, match="control_weight"):
            CS.check_control_weight(cw, 1, F, h, w)
    for v in (float("nan"), float("inf"), float("-inf")):
        cw = torch.ones(F, h, w)
        cw[3, 2, 1] = v
        with pytest.raises(ValueError, match="control_weight.*finite"):
            CS.check_control_weight(cw, 1, F, h, w)
    with pytest.raises(ValueError, match="control_weight"):
        CS.check_control_weight("a map", 1, F, h, w)


@pytest.mark.parametrize("h,w", [(8, 8), (9, 16)])
def test_level_pooling_is_the_block_mean_where_sizes_divide(h, w):
    """A tap of size (hh, ww) uses ``adaptive_avg_pool2d(control_weight, (hh, ww))``; the 2^l x 2^l block mean where h, w divide.  The
    vectors are laid out like the level's channels-last rows and repeated for the two CFG halves (uncond clips first)."""
    Bc, F = 2, 3
    cw = torch.rand(Bc, F, h, w, generator=torch.Generator().manual_seed(h * w))
    sizes = CS.tap_sizes(h, w, 4)
    assert sizes == ([(8, 8), (4, 4), (2, 2), (1, 1)] if (h, w) == (8, 8) else [(9, 16), (5, 8), (3, 4), (2, 2)])
    lv = CS.pool_control_weight(cw, sizes)
    assert set(lv) == set(sizes)
    for level, (hh, ww) in enumerate(sizes):
        v = lv[(hh, ww)]
        assert v.dtype == torch.float32 and v.is_contiguous() and tuple(v.shape) == (2 * Bc * F * hh * ww,)
        halves = v.view(2, Bc, F, hh, ww)
        assert torch.equal(halves[0], halves[1])                                               # both CFG halves: the same weights
        assert torch.equal(halves[0], torch.nn.functional.adaptive_avg_pool2d(cw, (hh, ww)))
        k = 2 ** level
        if h % k == 0 and hh == h // k:                                                         # rows divide: mean over k rows
            rows = cw.view(Bc, F, hh, k, w).mean(3)
            if w % k == 0 and ww == w // k:                                                     # both divide: the k x k block mean
                block = cw.view(Bc, F, hh, k, ww, k).mean((3, 5))
                assert torch.allclose(halves[0], block, rtol=0, atol=1e-6)
                by_hand = sum(cw[1, 2, k * 1 + a, k * 0 + b] for a in range(k) for b in range(k)) / (k * k) if hh > 1 else cw[1, 2].mean()
                assert abs(float(halves[0][1, 2, min(1, hh - 1), 0]) - float(by_hand)) < 1e-6
            else:
                assert tuple(rows.shape) == (Bc, F, hh, w)
    assert torch.equal(lv[sizes[0]].view(2, Bc, F, h, w)[1], cw)                               # level 0: the map itself
    ones = CS.pool_control_weight(torch.ones(1, F, h, w), sizes)
    assert all(bool((v == 1).all()) for v in ones.values())
    # the taps of the last two levels share a size in the SVD nets (no downsampler after the last block): one buffer per distinct size
    assert len(CS.pool_control_weight(cw, sizes + [sizes[-1]])) == len(sizes)


def test_denoise_signature_and_defaults():
    from posetraj_amd import StableVideoDiffusionPipelineControlNet as Pipe
    from posetraj_amd.pipeline_stable_video_diffusion_controlnet_cam import StableVideoDiffusionPipelineControlNet as CamPipe
    for fn in (Pipe.denoise, Pipe.__call__):
        p = inspect.signature(fn).parameters
        assert p["control_guidance_start"].default == 0.0 and p["control_guidance_end"].default == 1.0 and p["control_weight"].default is None
        assert p["controlnet_cond_scale"].default == 1.0
        for word in ("control_guidance_start", "control_guidance_end", "control_weight", "s[:, None, None].expand(F, h, w)", "[0, 1]"):
            assert word in fn.__doc__, word
    assert "kw" in inspect.signature(CamPipe.__call__).parameters
    assert all(word in CamPipe.__call__.__doc__ for word in ("control_guidance_start", "control_guidance_end", "control_weight"))


def test_control_entry_point_prototype_and_host_refusals():
    """The exact prototype ``hip`` read from include/posetraj_control.h (the header's contract with the library: tests/test_abi_cpu.py),
    and the host refuses bad arguments before any launch."""
    from posetraj_amd import hip
    assert hip.ABIS["control"].prototypes["ptc_weighted_residual_add_f16"] == (
        "int", ["const float*", "int64_t", "const float*", "float", "void*", "const void*", "int64_t", "int64_t", "int32_t", "void*"])
    assert "control.hip" in hip.SOURCES
    L, C = hip.lib(), hip.checked()
    assert L.ptc_weighted_residual_add_f16(None, 64, None, 1.0, None, None, 64, 8, 64, None) != 0 and b"null pointer" in L.pt_last_error()
    assert L.ptc_weighted_residual_add_f16(256, 64, 256, 1.0, 256, None, 64, 8, 12, None) != 0 and b"ptc_weighted_residual_add_f16" in L.pt_last_error()
    assert L.ptc_weighted_residual_add_f16(256, 60, 256, 1.0, 256, None, 64, 8, 64, None) != 0 and b"pitch" in L.pt_last_error()
    assert L.ptc_weighted_residual_add_f16(256, 64, 256, 1.0, 264, None, 64, 8, 64, None) != 0 and b"aligned" in L.pt_last_error()
    with pytest.raises(RuntimeError, match="ptc_weighted_residual_add_f16"):
        C.ptc_weighted_residual_add_f16(None, 64, None, 1.0, None, None, 64, 8, 64, None)
