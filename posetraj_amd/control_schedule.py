"""Control strength over the denoise loop of ``StableVideoDiffusionPipelineControlNet``: which steps run the ControlNet
(``control_guidance_start`` / ``control_guidance_end``, diffusers' rule), with which scale (a float or one per step), and with which
weight per frame and latent pixel (``control_weight``).  Pure host-side planning and validation - nothing here needs a device or the
HIP library; the pipeline turns the plan into its three kinds of step (plain / weighted / off).

The reference has none of these arguments: a call that gives none of them is planned as before."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch


def check_control_window(control_guidance_start: float, control_guidance_end: float) -> Tuple[float, float]:
    """diffusers' ``check_inputs`` for the two window arguments; a ``ValueError`` names the offending one."""
    for name, v in (("control_guidance_start", control_guidance_start), ("control_guidance_end", control_guidance_end)):
        try:
            ok = math.isfinite(float(v))
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"`{name}` must be a finite number; got {v!r}")
    start, end = float(control_guidance_start), float(control_guidance_end)
    if start < 0.0:
        raise ValueError(f"`control_guidance_start` cannot be smaller than 0; got {start}")
    if end > 1.0:
        raise ValueError(f"`control_guidance_end` cannot be larger than 1.0; got {end}")
    if start >= end:
        raise ValueError(f"`control_guidance_start` ({start}) cannot be larger than or equal to `control_guidance_end` ({end})")
    return start, end


def is_scale_sequence(controlnet_cond_scale) -> bool:
    """A per-step scale: anything that is not one plain number (list, tuple, numpy array, 1-D tensor)."""
    if isinstance(controlnet_cond_scale, (int, float)):
        return False
    if torch.is_tensor(controlnet_cond_scale):
        return controlnet_cond_scale.dim() > 0
    return hasattr(controlnet_cond_scale, "__len__")


def check_control_scale(num_steps: int, controlnet_cond_scale) -> List[float]:
    """One finite float per step: a number is repeated, a sequence must hold exactly ``num_steps`` of them."""
    if is_scale_sequence(controlnet_cond_scale):
        scales = [float(s) for s in controlnet_cond_scale]
        if len(scales) != num_steps:
            raise ValueError(f"`controlnet_cond_scale` has {len(scales)} entries for {num_steps} inference steps (one per step, or one float)")
    else:
        scales = [float(controlnet_cond_scale)] * num_steps
    for i, s in enumerate(scales):
        if not math.isfinite(s):
            raise ValueError(f"`controlnet_cond_scale` must be finite; entry {i} is {s}")
    return scales


def control_plan(num_steps: int, controlnet_cond_scale: Union[float, Sequence[float]] = 1.0, control_guidance_start: float = 0.0,
                 control_guidance_end: float = 1.0) -> List[Tuple[bool, float]]:
    """``[(on, scale)]`` per step.  With ``N = num_steps`` step ``i`` (0-based) keeps the ControlNet iff
    ``not (i / N < start or (i + 1) / N > end)`` (diffusers' ``controlnet_keep``) and its scale is not exactly 0.0 - a step that would
    add nothing skips the network.  A window narrower than a step, such as ``(0.1, 0.15)`` at any ``N`` up to 20, contains no step:
    every entry is off and the loop runs the U-Net alone."""
    if int(num_steps) != num_steps or num_steps < 1:
        raise ValueError(f"`num_inference_steps` must be a positive integer; got {num_steps!r}")
    num_steps = int(num_steps)
    start, end = check_control_window(control_guidance_start, control_guidance_end)
    scales = check_control_scale(num_steps, controlnet_cond_scale)
    plan = []
    for i, s in enumerate(scales):
        keep = not (i / num_steps < start or (i + 1) / num_steps > end)
        plan.append((bool(keep and s != 0.0), s))
    return plan


def check_control_weight(control_weight, clips: int, frames: int, h: int, w: int) -> Optional[torch.Tensor]:
    """``control_weight`` as fp32 ``[clips, frames, h, w]`` (on the device it came on): ``[F, h, w]`` serves every clip,
    ``[Bc, F, h, w]`` one map per clip, both at LATENT resolution.  Wrong rank / size or a non-finite value is a ``ValueError``."""
    if control_weight is None:
        return None
    try:
        cw = torch.as_tensor(control_weight).to(torch.float32)
    except (TypeError, ValueError, RuntimeError) as e:
        raise ValueError(f"`control_weight` must be convertible to an fp32 tensor: {e}") from None
    if cw.dim() not in (3, 4):
        raise ValueError(f"`control_weight` must be [F, h, w] or [Bc, F, h, w] at latent resolution; got {cw.dim()} dimensions {tuple(cw.shape)}")
    want = (frames, h, w) if cw.dim() == 3 else (clips, frames, h, w)
    if tuple(cw.shape) != want:
        raise ValueError(f"`control_weight` has shape {tuple(cw.shape)}; expected {want} ({clips} clip(s), {frames} frames, {h} x {w} latent pixels)")
    if not bool(torch.isfinite(cw).all()):
        raise ValueError("`control_weight` must be finite (it holds NaN or inf)")
    if cw.dim() == 3:
        cw = cw.unsqueeze(0).expand(clips, frames, h, w)
    return cw


def tap_sizes(h: int, w: int, levels: int) -> List[Tuple[int, int]]:
    """Spatial sizes of the ControlNet taps: the latent size, then one stride-2 convolution (padding 1, kernel 3: ``ceil(n / 2)``) per
    further level."""
    sizes = [(int(h), int(w))]
    for _ in range(levels - 1):
        hh, ww = sizes[-1]
        sizes.append(((hh + 1) // 2, (ww + 1) // 2))
    return sizes


def pool_control_weight(control_weight: torch.Tensor, sizes: Sequence[Tuple[int, int]]) -> Dict[Tuple[int, int], torch.Tensor]:
    """``{(hh, ww): fp32 [2 * Bc * F * hh * ww]}``: ``adaptive_avg_pool2d`` of the ``[Bc, F, h, w]`` map to each tap size (where the sizes
    divide, the block mean), laid out like the rows of that level's channels-last activations, and repeated for the two
    classifier-free-guidance halves of the batch (all unconditional clips first, then all conditional ones: same weights)."""
    Bc, F = control_weight.shape[:2]
    out = {}
    for hh, ww in sizes:
        if (hh, ww) not in out:
            p = torch.nn.functional.adaptive_avg_pool2d(control_weight.reshape(Bc * F, 1, *control_weight.shape[2:]), (hh, ww))
            out[(hh, ww)] = torch.cat([p.reshape(-1)] * 2).contiguous()
    return out
