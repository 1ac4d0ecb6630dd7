"""Long videos from a short-clip model: the long latent video is denoised as overlapping windows of the trained length, each window one
ordinary clip evaluation, and the predictions of the windows that cover a frame are blended at every step.  Here: the
plan (host), and the loop's two passes over device tensors - the prologue that cuts the windows out of the long latent and the
epilogue that guides and blends the K predictions - through ``libposetraj_window.so`` (include/posetraj_window.h), an add-on library
of its own that ``posetraj_amd.hip.build`` makes beside the main one.  No CPU or PyTorch fallback: a missing library is an error."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import hip
from .ops import _need, _stream

MAX_WINDOWS = 64                     # the kernels take the starts by value


class WindowPlan(NamedTuple):
    """``num_frames`` frames as ``K = len(starts)`` windows of ``window_frames``; ``weights`` fp32 ``[K, window_frames]``."""
    num_frames: int
    window_frames: int
    window_stride: int
    starts: Tuple[int, ...]
    weights: np.ndarray

    @property
    def K(self) -> int:
        return len(self.starts)


def _whole(name: str, v) -> int:
    if isinstance(v, bool) or int(v) != v:
        raise ValueError(f"`{name}` must be an integer; got {v!r}")
    return int(v)


def window_plan(num_frames: int, window_frames: int, window_stride: int) -> WindowPlan:
    """The windows of a ``num_frames`` video: ``K = ceil((Ft - Fw) / s) + 1`` windows, window ``i`` starts at ``min(i s, Ft - Fw)`` (the
    last one ends on the last frame; ``Ft == Fw`` is one window).  Needs ``1 <= Fw <= Ft``, ``1 <= s <= Fw`` (no gap) and ``K <= 64``;
    a violation is a ``ValueError`` that names the argument.

    Blend weights: window-local triangle ``t(j) = min(j + 1, Fw - j)``; per frame the weights of the covering windows are normalised
    to sum 1 in fp64 and then rounded to fp32.  A frame that one window covers gets exactly 1.0."""
    Ft, Fw, s = _whole("num_frames", num_frames), _whole("window_frames", window_frames), _whole("window_stride", window_stride)
    if Fw < 1 or Fw > Ft:
        raise ValueError(f"`window_frames` must be in 1 .. num_frames = {Ft}; got {Fw}")
    if s < 1 or s > Fw:
        raise ValueError(f"`window_stride` must be in 1 .. window_frames = {Fw} (a larger stride leaves frames uncovered); got {s}")
    K = -(-(Ft - Fw) // s) + 1
    if K > MAX_WINDOWS:
        raise ValueError(f"`window_stride` = {s} cuts {Ft} frames into {K} windows of {Fw}; at most {MAX_WINDOWS} are supported")
    starts = tuple(min(i * s, Ft - Fw) for i in range(K))
    tri = np.minimum(np.arange(Fw) + 1, Fw - np.arange(Fw)).astype(np.float64)
    total = np.zeros(Ft, dtype=np.float64)
    for st in starts:
        total[st:st + Fw] += tri
    weights = np.stack([tri / total[st:st + Fw] for st in starts]).astype(np.float32)
    return WindowPlan(Ft, Fw, s, starts, weights)


def resolve(num_frames: int, window_frames, window_stride=None, window_batch=None) -> Tuple[WindowPlan, int]:
    """The plan and the number of windows per network evaluation from the arguments of ``denoise`` / ``__call__``: the stride defaults
    to ``window_frames // 2`` (at least 1), ``window_batch`` to K and must divide K."""
    Fw = _whole("window_frames", window_frames)
    plan = window_plan(num_frames, Fw, max(Fw // 2, 1) if window_stride is None else window_stride)
    G = plan.K if window_batch is None else _whole("window_batch", window_batch)
    if G < 1 or plan.K % G:
        raise ValueError(f"`window_batch` must divide the number of windows K = {plan.K}; got {G}")
    return plan, G


def _host_starts(starts):
    return (C.c_int32 * len(starts))(*starts)


def scale_concat_windows(latents: torch.Tensor, image_latents: torch.Tensor, sigma: float, starts, window_frames: int,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 ``latents [Ft, 4, h, w]`` (or ``[1, Ft, 4, h, w]``), contiguous, + fp16 ``image_latents [2, 4, h, w]`` -> fp16
    ``[2K, Fw, h, w, 8]``, halves-major: the rows of window k are ``ops.scale_concat_input`` of frames ``starts[k] .. + Fw``, bit for
    bit.  ``starts`` must be a plan of their own over the ``Ft`` frames given (first 0, no gap, last ``Ft - Fw``)."""
    _need(latents, "latents", torch.float32); _need(image_latents, "image_latents")
    if not (latents.is_contiguous() and image_latents.is_contiguous()) or tuple(image_latents.shape[:2]) != (2, 4):
        raise RuntimeError(f"posetraj_amd.scale_concat_windows: latents {tuple(latents.shape)} / image_latents {tuple(image_latents.shape)} "
                           "must be contiguous, image_latents [2, 4, h, w]")
    Ft, _, h, w = latents.shape[-4:]
    K, Fw = len(starts), int(window_frames)
    if out is None:
        out = torch.empty((2 * K, Fw, h, w, 8), dtype=torch.float16, device=latents.device)
    elif out.dtype != torch.float16 or out.numel() != 2 * K * Fw * h * w * 8 or not out.is_contiguous():
        raise RuntimeError(f"posetraj_amd.scale_concat_windows: out {tuple(out.shape)} {out.dtype} for {K} windows of {Fw} x {h} x {w}")
    hip.window().ptw_scale_concat_windows(latents.data_ptr(), image_latents.data_ptr(), float(sigma), _host_starts(starts), K, Fw, Ft, h, w,
                                          out.data_ptr(), _stream())
    return out


def cfg_window_merge(pred: torch.Tensor, guidance: torch.Tensor, weights: torch.Tensor, starts, num_frames: int,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``pred`` fp16 or fp32 channels-last ``[2K, Fw, h, w, ld]``, halves-major; ``guidance`` fp32 ``[Fw]`` (window-local);
    ``weights`` fp32 ``[K, Fw]`` -> fp32 ``[Ft, 4, h, w]``: per window guidance, then the weighted sum of the covering windows in
    ascending window order, every operation one fp32 rounding (include/posetraj_window.h)."""
    f32 = pred.dtype == torch.float32
    _need(pred, "pred", pred.dtype if f32 else torch.float16)
    _need(guidance, "guidance", torch.float32); _need(weights, "weights", torch.float32)
    K, Ft = len(starts), int(num_frames)
    rows, Fw, h, w, _ = pred.shape
    ld = pred.stride(-2) if w > 1 else pred.shape[-1]                      # pixels densely packed at a pitch of ld >= 4 channels
    dense = all(n == 1 or s == t for n, s, t in zip(pred.shape, pred.stride(), (Fw * h * w * ld, h * w * ld, w * ld, ld, 1)))
    if rows != 2 * K or not dense or guidance.numel() != Fw or tuple(weights.shape) != (K, Fw) or not (guidance.is_contiguous() and weights.is_contiguous()):
        raise RuntimeError(f"posetraj_amd.cfg_window_merge: pred {tuple(pred.shape)} (strides {pred.stride()}) / guidance {tuple(guidance.shape)} / "
                           f"weights {tuple(weights.shape)} for {K} windows")
    if out is None:
        out = torch.empty((Ft, 4, h, w), dtype=torch.float32, device=pred.device)
    elif out.dtype != torch.float32 or out.numel() != Ft * 4 * h * w or not out.is_contiguous():
        raise RuntimeError(f"posetraj_amd.cfg_window_merge: out {tuple(out.shape)} {out.dtype} for {Ft} x 4 x {h} x {w}")
    hip.window().ptw_cfg_window_merge(pred.data_ptr(), 1 if f32 else 0, ld, guidance.data_ptr(), weights.data_ptr(),
                                      _host_starts(starts), K, Fw, Ft, h, w, out.data_ptr(), _stream())
    return out


class WindowStaging:
    """What a ``StepState`` needs of the plan: the shape of the networks' input for one group of ``batch`` windows and the call that
    stages it.  A group is a plan of its own over the frames it spans (its first window's start .. its last window's end), so the
    kernel is handed that span of the long latent and the starts relative to it.  ``select(g)`` picks the group the next step runs."""

    def __init__(self, plan: WindowPlan, batch: int):
        self.plan, self.batch, self.group = plan, int(batch), 0

    def select(self, group: int) -> None:
        self.group = int(group)

    def windows(self, group: Optional[int] = None) -> range:
        g = self.group if group is None else group
        return range(g * self.batch, (g + 1) * self.batch)

    def input_shape(self, h: int, w: int) -> tuple:
        return (2 * self.batch, self.plan.window_frames, h, w, 8)

    def stage(self, x: torch.Tensor, il: torch.Tensor, sigma: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Latents ``x`` ``[1, Ft, 4, h, w]`` -> the selected group's input ``[2 batch, Fw, h, w, 8]`` (into ``out`` when given)."""
        starts = [self.plan.starts[k] for k in self.windows()]
        lo, hi = starts[0], starts[-1] + self.plan.window_frames
        return scale_concat_windows(x[0, lo:hi], il, sigma, [s - lo for s in starts], self.plan.window_frames, out=out)
