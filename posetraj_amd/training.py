"""The reference's ControlNet training step on the MI355X path (SURVEY 8f4;
``/root/reference/scripts/train_svd_traj_VIPSeg_14.py:1264-1425``): sigma sampling, noising + EDM preconditioning
(``pt_edm_train_input``), the training-time ``added_time_ids``, conditioning dropout, ControlNet + frozen U-Net forward, the
sigma-weighted MSE and the single-frame "spatial" loss (``pt_edm_loss``) - ``controlnet_training_loss``, the objective alone on the
inference kernels - and the whole step: ``ControlNetTrainer`` runs the forward on the tape of ``autodiff.py`` /
``train_graph.py``, the reverse pass through the frozen U-Net's up path into every ControlNet parameter, and ``torch.optim.AdamW``'s
update (``pt_adamw_f32``) with fp16-mixed-precision loss scaling and gradient accumulation as ``accelerate`` does them for
``start_ft.sh``.  The VAE encode (``tensor_to_vae_latent``, ``:495-503``) and the CLIP embedding of the first frame are this
package's own models; their outputs are the step's inputs.  The camera twin (``controlnet_sdv_cam``, ``scripts/train_svd_traj_VIPSeg_14_cam_concat.py``: the same step with
``camera_cond`` and without the spatial loss) trains through the same class.  ``--use_ema`` (off in the launch scripts) is
``ControlNetTrainer(use_ema=True)``: diffusers' ``EMAModel`` over the ControlNet's parameters (``training_utils.py``), stepped inside
the optimizer's pass.  ``--use_8bit_adam`` (``:1041-1049``, bitsandbytes' ``AdamW8bit``; off in the launch scripts) is
``ControlNetTrainer(use_8bit_adam=True)``: block-quantised moments, updated by ``pto_adamw8_f32``; either way ``trainer.optimizer``
(``optim.py``) owns the moments, the update's launch and the optimizer's part of a checkpoint.  ``--gradient_checkpointing``
(``:1025-1026``, ON in every launch script) is ``ControlNetTrainer(gradient_checkpointing=True)``: every residual block and transformer
of the ControlNet is a checkpointed segment of the tape (``autodiff.checkpoint``) - its activations are dropped after the forward and
recomputed, by the same kernels, in the reverse pass.  Not here: the data loader.
"""
from __future__ import annotations

import gc
import math
import time
from typing import Optional

import torch

from . import hip, ops, optim

# scripts/train_svd_traj_VIPSeg_14.py:314-319, :1288
MIN_VALUE, MAX_VALUE, IMAGE_D, NOISE_D_LOW, NOISE_D_HIGH, SIGMA_DATA = 0.002, 700, 64, 32, 64, 0.5
TRAIN_NOISE_AUG = 0.02


def stratified_uniform(shape, group=0, groups=1, dtype=None, device=None, generator=None):
    """``:273-282``."""
    if groups <= 0:
        raise ValueError(f"groups must be positive, got {groups}")
    if group < 0 or group >= groups:
        raise ValueError(f"group must be in [0, {groups})")
    n = shape[-1] * groups
    offsets = torch.arange(group, n, groups, dtype=dtype, device=device)
    u = torch.rand(shape, dtype=dtype, device=device, generator=generator)
    return (offsets + u) / n


def rand_cosine_interpolated(shape, image_d=IMAGE_D, noise_d_low=NOISE_D_LOW, noise_d_high=NOISE_D_HIGH, sigma_data=SIGMA_DATA,
                             min_value=MIN_VALUE, max_value=MAX_VALUE, device="cpu", dtype=torch.float32, generator=None):
    """``:285-312``: one sigma per clip from the interpolated, shifted cosine log-SNR schedule.  A handful of scalars: host maths,
    identical to the reference's expression order."""
    def cosine(t, lo, hi):
        t_min = math.atan(math.exp(-0.5 * hi))
        t_max = math.atan(math.exp(-0.5 * lo))
        return -2 * torch.log(torch.tan(t_min + t * (t_max - t_min)))

    def shifted(t, noise_d, lo, hi):
        shift = 2 * math.log(noise_d / image_d)
        return cosine(t, lo - shift, hi - shift) + shift

    logsnr_min = -2 * math.log(min_value / sigma_data)
    logsnr_max = -2 * math.log(max_value / sigma_data)
    t = stratified_uniform(shape, group=0, groups=1, dtype=dtype, device=device, generator=generator)
    logsnr = torch.lerp(shifted(t, noise_d_low, logsnr_min, logsnr_max), shifted(t, noise_d_high, logsnr_min, logsnr_max), t)
    return torch.exp(-logsnr / 2) * sigma_data


def train_add_time_ids(fps, motion_bucket_ids, noise_aug_strength, dtype, batch_size, unet=None, device=None):
    """``:1177-1220``: rows ``[fps, noise_aug_strength, motion_bucket_id]`` (the training order - the inference pipeline's is
    ``[fps, motion_bucket_id, noise_aug_strength]``), with the reference's consistency checks."""
    target = device if device is not None else "cpu"
    m = motion_bucket_ids.to(device=target) if torch.is_tensor(motion_bucket_ids) else torch.tensor(motion_bucket_ids, dtype=dtype, device=target)
    if m.dim() == 1:
        m = m.view(-1, 1)
    if m.size(0) != batch_size:
        raise ValueError("The length of motion_bucket_ids must match the batch_size.")
    ids = torch.cat([torch.tensor([fps, noise_aug_strength], dtype=dtype, device=target).repeat(batch_size, 1), m.to(dtype)], dim=1)
    if unet is not None:
        passed = unet.config.addition_time_embed_dim * ids.size(1)
        expected = unet.add_embedding.linear_1.in_features
        if expected != passed:
            raise ValueError(f"Model expects an added time embedding vector of length {expected}, but a vector of {passed} was created. "
                             "The model has an incorrect config. Please check `unet.config.time_embedding_type` and `text_encoder_2.config.projection_dim`.")
    return ids


def _edm_loss(pred: torch.Tensor, noisy: torch.Tensor, target: torch.Tensor, sigmas: torch.Tensor) -> torch.Tensor:
    """``pred`` ``[B, F, 4, h, w]`` as the U-Net returns it (a view of a channels-last buffer) -> per-sample losses ``[B]``."""
    B, F, Cc, h, w = pred.shape
    cl = pred.permute(0, 1, 3, 4, 2)
    if not cl.is_contiguous():
        cl = cl.contiguous()
    if cl.dtype not in (torch.float16, torch.float32):
        cl = cl.float()
    out = torch.empty(B, dtype=torch.float32, device=pred.device)
    hip.checked().pt_edm_loss(cl.data_ptr(), 1 if cl.dtype == torch.float32 else 0, Cc, noisy.data_ptr(), target.data_ptr(),
                              sigmas.data_ptr(), B, F, h * w, out.data_ptr(), ops._stream())
    return out


def _check_batch(B, F, *, encoder_hidden_states, motion_values, trajectories, noise, sigmas, random_p, camera_cond, noise_shape) -> None:
    """The per-clip arguments of a step against the batch size of ``latents``: ``ValueError`` naming the argument."""
    def lead(name, t, want):
        if t is not None and (t.dim() < len(want) or tuple(t.shape[:len(want)]) != want):
            raise ValueError(f"{name} must lead with {list(want)} (latents hold {B} clip(s) of {F} frames); got {tuple(t.shape)}")

    def count(name, t):
        n = None if t is None else (t.numel() if torch.is_tensor(t) else len(t) if hasattr(t, "__len__") else 1)
        if n is not None and n != B:
            raise ValueError(f"{name} must hold one value per clip ({B}); got {n}")

    lead("encoder_hidden_states", encoder_hidden_states, (B,))
    lead("trajectories", trajectories, (B, F))
    count("motion_values", motion_values)
    count("sigmas", sigmas)
    count("random_p", random_p)
    if noise is not None and tuple(noise.shape) != noise_shape:
        raise ValueError(f"noise must have the shape of latents {noise_shape}; got {tuple(noise.shape)}")
    if camera_cond is not None:
        cam = torch.as_tensor(camera_cond)
        if cam.dim() != 3 or tuple(cam.shape) != (B, F, 12):
            raise ValueError(f"camera_cond must be [{B}, {F}, 12] (R|T per frame of every clip); got {tuple(cam.shape)}")


def _step_inputs(dev, latents, encoder_hidden_states, motion_values, trajectories, unet, *, scaling_factor, conditioning_dropout_prob, use_spatial,
                 noise, sigmas, random_p, ran_idx, generator, kernel: bool = True, lazy_traj: bool = False, camera_cond=None):
    """``:1275-1345``: the step's random draws (sampled here when not given), noising, EDM preconditioning, conditioning dropout,
    ``added_time_ids``.  Returns a dict of device tensors; ``x`` is the network input channels-last ``[B, F, h, w, 8]``.  Every per-clip
    argument must lead with the batch size of ``latents`` (``ValueError`` naming the argument); ``ran_idx`` is one frame index per step.
    ``camera_cond`` ``[B, F, 12]`` is only checked and passed on (``cam``, fp32 on the host)."""
    if latents.dim() != 5 or latents.shape[2] != 4:
        raise ValueError(f"latents must be [batch, frames, 4, h, w]; got {tuple(latents.shape)}")
    lat = latents.to(device=dev, dtype=torch.float32).contiguous()
    B, F, Cz, h, w = lat.shape
    _check_batch(B, F, encoder_hidden_states=encoder_hidden_states, motion_values=motion_values, trajectories=trajectories, noise=noise,
                 sigmas=sigmas, random_p=random_p, camera_cond=camera_cond, noise_shape=tuple(lat.shape))
    if noise is None:
        noise = torch.randn(lat.shape, generator=generator, dtype=torch.float32)                 # torch.randn_like(latents)
    if sigmas is None:
        sigmas = rand_cosine_interpolated([B], generator=generator)
    if conditioning_dropout_prob is not None and random_p is None:
        random_p = torch.rand(B, generator=generator)
    if ran_idx is None:
        ran_idx = int(torch.randint(0, F, (1,), generator=generator).item())
    noise = noise.to(device=dev, dtype=torch.float32).contiguous()
    sig_host = sigmas.detach().to("cpu", torch.float32).reshape(B)
    ehs = encoder_hidden_states
    mask = torch.ones(B, dtype=torch.float32)
    if conditioning_dropout_prob is not None:                                                    # :1317-1339
        p, rp = conditioning_dropout_prob, random_p.detach().to("cpu", torch.float32)
        ehs = torch.where((rp < 2 * p).reshape(B, 1, 1).to(ehs.device), torch.zeros_like(ehs), ehs)
        mask = 1 - ((rp >= p).to(torch.float32) * (rp < 3 * p).to(torch.float32))
    sig = sig_host.to(dev)
    cond_scale = (mask / scaling_factor).to(dev)
    timesteps = torch.Tensor([0.25 * s.log() for s in sig_host])                                 # :1295-1296
    ids = train_add_time_ids(6, motion_values, TRAIN_NOISE_AUG, torch.float32, B, unet, device=dev)
    I = dict(lat=lat, noise=noise, sig=sig, cond_scale=cond_scale, sig_host=sig_host, timesteps=timesteps, ids=ids, ehs=ehs,
             ran_idx=ran_idx, dims=(B, F, h, w))
    if camera_cond is not None:
        I["cam_host"] = torch.as_tensor(camera_cond, dtype=torch.float32)
    if lazy_traj:                                             # the largest input (15 MB at 320 x 576; a host-side cast + copy of ~6 ms): the trainer
        I["traj_src"] = trajectories                          # stages it AFTER it has launched the frozen encoder, which does not read it
    else:
        I["traj"] = trajectories.to(dev, torch.float16)
    if kernel:
        _edm_train_input(I)
    return I


def _edm_train_input(I: dict) -> dict:
    """The device half of ``_step_inputs``: ``noisy`` latents and the network input ``x`` (EDM preconditioning + image-latent concat)."""
    lat, (B, F, h, w) = I["lat"], I["dims"]
    I["noisy"] = torch.empty_like(lat)
    I["x"] = torch.empty((B, F, h, w, 8), dtype=torch.float16, device=lat.device)
    hip.checked().pt_edm_train_input(lat.data_ptr(), I["noise"].data_ptr(), I["sig"].data_ptr(), I["cond_scale"].data_ptr(), TRAIN_NOISE_AUG,
                                     B, F, h * w, I["noisy"].data_ptr(), I["x"].data_ptr(), ops._stream())
    return I


@torch.no_grad()
def controlnet_training_loss(controlnet, unet, latents: torch.Tensor, encoder_hidden_states: torch.Tensor, motion_values,
                             trajectories: torch.Tensor, *, scaling_factor: float = 0.18215,
                             conditioning_dropout_prob: Optional[float] = None, use_spatial: bool = True,
                             noise: Optional[torch.Tensor] = None, sigmas: Optional[torch.Tensor] = None,
                             random_p: Optional[torch.Tensor] = None, ran_idx: Optional[int] = None,
                             generator: Optional[torch.Generator] = None) -> dict:
    """One training step's forward and loss (``:1275-1407``) on the inference kernels, for ``latents`` ``[B, F, 4, h, w]`` (VAE
    latents x scaling_factor), ``encoder_hidden_states`` ``[B, 1, D]`` (CLIP embedding of the first frame), ``motion_values``
    ``[B]``, ``trajectories`` ``[B, F, 3, H, W]`` in [-1, 1].  ``noise`` / ``sigmas`` / ``random_p`` / ``ran_idx``: the step's random
    draws, sampled here (``generator``) when not given.  Returns ``loss`` (= temporal + 0.5 spatial), ``loss_temporal``,
    ``loss_spatial`` as floats and the intermediate tensors; the losses are means over the clips.  ``use_spatial`` follows the
    reference's hard-wired ``True``.  For a batch the spatial loss is taken PER CLIP - clip b's own residual rows of frame ``ran_idx``, its
    own sigma, noisy latent and target, then the mean over the clips - where the reference's expression, written for one clip, takes
    clip 0's residuals for every clip and a B x B cross product of predictions and sigmas; one clip: the same
    computation.  For the step WITH its backward see ``ControlNetTrainer``."""
    dev = unet.device
    if dev is None:
        raise RuntimeError("controlnet_training_loss: the U-Net has no weights loaded")
    I = _step_inputs(dev, latents, encoder_hidden_states, motion_values, trajectories, unet, scaling_factor=scaling_factor,
                     conditioning_dropout_prob=conditioning_dropout_prob, use_spatial=use_spatial, noise=noise, sigmas=sigmas,
                     random_p=random_p, ran_idx=ran_idx, generator=generator)
    lat, noisy, sig, timesteps, ehs, ids, ran_idx = I["lat"], I["noisy"], I["sig"], I["timesteps"], I["ehs"], I["ids"], I["ran_idx"]
    inp = I["x"].permute(0, 1, 4, 2, 3)                                                          # [B, F, 8, h, w] view
    down, mid = controlnet(inp, timesteps, ehs, added_time_ids=ids, controlnet_cond=I["traj"], return_dict=False)
    pred = unet(inp, timesteps, ehs, added_time_ids=ids, down_block_additional_residuals=list(down),
                mid_block_additional_residual=mid, return_dict=False)[0]
    per_sample = _edm_loss(pred, noisy, lat, sig)
    loss_t = float(per_sample.mean())
    out = dict(loss=loss_t, loss_temporal=loss_t, loss_spatial=None, model_pred=pred, inp_noisy_latents=inp, timesteps=timesteps,
               added_time_ids=ids, encoder_hidden_states=ehs, noise=I["noise"], sigmas=I["sig_host"], ran_idx=ran_idx)
    if use_spatial:                                                                              # :1388-1407
        B, F = I["dims"][:2]
        frame = (lambda d: d[ran_idx].unsqueeze(0)) if B == 1 else (lambda d: d[ran_idx::F])    # frame ran_idx of every clip: rows b F + ran_idx
        pred_s = unet(inp[:, ran_idx].unsqueeze(1), timesteps, ehs, added_time_ids=ids,
                      down_block_additional_residuals=[frame(d) for d in down],
                      mid_block_additional_residual=frame(mid), return_dict=False)[0]
        ls = _edm_loss(pred_s, noisy[:, ran_idx:ran_idx + 1].contiguous(), lat[:, ran_idx:ran_idx + 1].contiguous(), sig)
        out["loss_spatial"] = float(ls.mean())
        out["loss"] = loss_t + 0.5 * out["loss_spatial"]
    return out


import contextlib

_null = contextlib.nullcontext


class ControlNetTrainer:
    """The reference's optimisation step for the ControlNet (``:1040-1076`` set-up, ``:1264-1425`` step): fp32 master parameters in
    one flat buffer, the frozen U-Net, ``torch.optim.AdamW`` semantics (``lr``, ``betas``, ``weight_decay``, ``eps`` = the script's
    ``--learning_rate`` / ``--adam_*`` arguments), ``accelerate``'s fp16 handling (loss scaled by ``loss_scale`` before the reverse
    pass, the step skipped and the scale halved when a gradient overflowed, doubled after ``growth_interval`` clean steps) and
    gradient accumulation (``--gradient_accumulation_steps``: each micro-batch's loss is divided by it).  Under
    ``torch.distributed`` (one process per GPU) the ranks train data-parallel like accelerate's DDP: parameters broadcast from rank 0,
    gradients averaged by bucketed all-reduces overlapped with the reverse pass (``grad_sync.py``).

    ``wgrad_stream`` (default on): every layer's weight / bias gradient runs on a second HIP stream beside its data gradient -
    the low-resolution layers fill a fraction of the chip each, and nobody waits for a weight gradient before the optimizer.
    ``spatial_stream`` (default on): the one-frame decoder pass of the spatial loss runs, forward and backward, on a third stream
    beside the temporal pass (its ~1 500 launches over a few hundred rows each are latency, not throughput).

    ``lr_scheduler``: the multiplier of ``learning_rate`` as a function of the optimizer steps taken so far, e.g.
    ``train_state.get_scheduler(args.lr_scheduler, args.lr_warmup_steps, args.max_train_steps)`` (``:1109-1114``, ``:1424``); None = constant.
    ``save_state`` / ``load_state`` / ``save_pretrained``: ``accelerator.save_state`` / ``load_state`` and ``controlnet.save_pretrained``
    (``train_state.py``).

    ``freeze_gc`` (opt-in; a process-wide side effect, undone by ``unfreeze_gc()``): ``gc.freeze()`` once the trainer is built and
    again after its first optimizer step.  A step
    allocates ~10^5 short-lived Python objects that stay alive until its reverse pass has run, which promotes them to the oldest
    generation and triggers a full collection every six or seven steps; each one walks the whole process (torch's modules, this
    package's layer and pack objects) for ~45 ms and frees nothing (profiles/r04/train_step_host_gc.txt).  Frozen, the
    long-lived objects are out of the collector's way; cyclic garbage among them would no longer be reclaimed (there is none).

    ``use_ema`` (``--use_ema``; ``ema_*``: the arguments of diffusers' ``EMAModel``, ``:970-974``): ``trainer.ema`` is a
    ``training_utils.EMAModel`` over the parameters - one more flat fp32 buffer - and ``optimizer_step`` OWNS its step: the loop does not
    call ``ema.step`` (``:1430``) as well.  The reference steps the EMA under ``accelerator.sync_gradients``, i.e. once per accumulation
    cycle whether or not the GradScaler skipped the optimizer: on a taken step the update is part of the AdamW launch
    (``pt_adamw_ema_f32``: the shadow follows the new parameter while it is in a register), on a skipped one it is ``pt_ema_update_f32``
    toward the unchanged parameters.  ``ema_state_dict()``: the averaged weights, for a validation pipeline or the final export.
    Data parallel: every rank keeps its own, identical shadow.  ``None`` (the default): no buffer, no launch, nothing in a checkpoint.

    ``use_8bit_adam`` (``--use_8bit_adam``): AdamW's two moments are kept as 8-bit codes into two 256-entry books with one fp32
    absmax per block of 256 stored elements (parameters under 4096 elements keep fp32 moments) - 2.03 bytes per parameter instead of
    8; ``trainer.optimizer`` is then an ``optim.AdamW8bit`` instead of an ``optim.AdamW``, and no full-size moment buffer is
    allocated.  Its ``step`` runs ``pto_adamw8_f32`` - torch's AdamW statements on the dequantised moments,
    the fp16 mirror, the gradient's zeroing and the fused EMA in one launch, as the fp32 pass does - under the same GradScaler rules,
    schedule and pack stream.  The format restates bitsandbytes' published blockwise quantisation; parity with the package is not
    pinned.  Data parallel needs nothing new: the update is a deterministic function of the averaged gradients, so every
    rank computes the same state.  Checkpoints of the two optimizer kinds do not load into each other.

    ``gradient_checkpointing`` (``--gradient_checkpointing`` / ``controlnet.enable_gradient_checkpointing()``): ``False`` (the default)
    keeps every activation, launch for launch the step as it was; ``True`` is the reference's flag - each ``ResBlock`` / ``Transformer``
    of the ControlNet runs as ``autodiff.checkpoint``: only its output survives the forward, and the reverse pass re-runs it (the forward
    kernels are bit-reproducible, so the recomputed activations are the dropped ones) before reversing it; ``"all"`` does the same to the
    frozen decoder's blocks in the temporal pass and in the one-frame spatial pass, whose recomputation stays on the spatial stream -
    which the reference, differentiating through an un-checkpointed U-Net, cannot.  Losses are the same launches in every mode;
    gradients differ by the order of the backward's fp32 atomics only.  The price is one more ControlNet forward per step
    (``"all"``: and one more decoder forward); what it buys is in DESIGN 4.13.  Accumulation, the GradScaler skip, ``use_ema``,
    ``use_8bit_adam``, data parallel and the side streams are untouched - the segments' weight gradients and ``grad_ready`` calls
    happen in the same order, once per micro-batch - and a checkpoint file knows nothing of the mode.  Not with ``use_graph``.

    ``deterministic`` (the script's ``--seed`` "for reproducible training" made to hold): ``False`` (the default) is the step as it was,
    launch for launch - its reverse pass accumulates with fp32 atomics, so two identical steps differ in the last bits.  ``True``: the
    gradients, the losses, ``grad_norm()`` and the parameters after ``optimizer_step()`` are a pure function of the trainer's inputs
    and state, on one GPU and for one build of the library - whatever the workgroup scheduling, whichever side streams are live (the
    first step of a fresh trainer and a later one agree), under every ``gradient_checkpointing`` mode (whose gradients then EQUAL the
    plain step's), under accumulation, ``use_ema`` and ``use_8bit_adam``.  Every reduction of the reverse pass that used atomics -
    GroupNorm's statistics and parameter gradients, LayerNorm's parameter gradients, bias / row-vector column sums, the AlphaBlender's
    ``mix_factor`` gradient, the gradient norm, split-K weight gradients - runs in two launches instead (``include/posetraj_det.h``): the
    same kernel storing one partial per workgroup into a workspace of its own, and a fold that adds them in ascending order; no atomics,
    no waiting between workgroups.  The forward and the attention backward were bit-reproducible already.  Under ``torch.distributed``
    the flag is accepted, but nothing is claimed across ranks: the all-reduce's order is the collective library's.  Nor across library
    builds or tile-plan changes.  A checkpoint file knows nothing of the mode.  Not with ``use_graph``.  Cost: DESIGN 4.13.

    Batches of clips (``--per_gpu_batch_size``): ``loss_and_grads`` / ``step`` take ``B`` clips at once - ``latents [B, F, 4, h, w]``,
    ``encoder_hidden_states [B, 1, D]``, ``motion_values [B]``, ``trajectories [B, F, 3, H, W]``, ``camera_cond [B, F, 12]``, ``noise``,
    ``sigmas [B]``, ``random_p [B]`` and ONE ``ran_idx`` - in one pass of the tape over ``B F`` frames; a mismatched batch dimension is a
    ``ValueError`` naming the argument.  The losses are the means over the clips (``:1381-1386``), so each clip's gradient carries 1 / B;
    under accumulation and data parallel a batch counts like one micro-batch (each rank's gradient is that of its local batch mean).
    As in the reference, the clips of a batch are not independent: the temporal blocks' cross-attention hands token ``(b, f, s)`` the
    context of clip ``(b S + s) mod B`` (``autodiff.add_rowvec_interleaved``, include/posetraj_batch.h), so a batch of two is
    not two accumulated micro-batches.  The spatial loss is taken PER CLIP - clip b's own residual rows of frame ``ran_idx``, its own
    sigma, noisy latent and target, the mean over clips - where the reference's expression, written for one clip, broadcasts clip 0's
    residuals and crosses every prediction with every sigma.  ``B == 1`` issues the launches it always did.  Every
    mode above works on a batch without code of its own, ``deterministic`` included (the new reduction has its two-launch form);
    ``use_graph=True`` refuses a batch with a ``ValueError``.  What a batch buys at 14 x 320 x 576: DESIGN 4.13.

    ``independent_clips`` (default ``False`` = the reference's batch, launch for launch): ``True`` departs from the reference on purpose
    and gives a batch the standard meaning - every clip's temporal cross-attention reads that clip's own context (``autodiff.add_rowvec``,
    one row per clip, the op ``B == 1`` uses, on both tapes; ``vec_mode=3`` in the frozen encoder's inference kernels), so a batch of
    ``B`` clips is the mean of ``B`` one-clip steps: losses and gradients equal those of ``B`` accumulated micro-batches up to rounding.
    ``B == 1`` is untouched.  Every mode above works as it does on a batch; ``use_graph=True`` still refuses a batch; a checkpoint file
    knows nothing of the flag.  What the mode does to a trained model's quality has not been measured (no trained checkpoint at hand).

    ``unet`` must have been loaded with ``keep_source=True`` (its up-path weights are re-packed for the data gradients).
    ``controlnet_state_dict``: the parameters to train, e.g. ``ControlNetSDVModel.from_unet(unet).state_dict()`` (``:935-938``)."""

    def __init__(self, controlnet_config, controlnet_state_dict, unet, *, learning_rate: float = 1e-4, adam_beta1: float = 0.9,
                 adam_beta2: float = 0.999, adam_weight_decay: float = 1e-2, adam_epsilon: float = 1e-8,
                 gradient_accumulation_steps: int = 1, loss_scale: float = 65536.0, growth_interval: int = 2000,
                 scaling_factor: float = 0.18215, conditioning_dropout_prob: Optional[float] = None, process_group=None,
                 bucket_mb: int = 256, wgrad_stream: bool = True, spatial_stream: bool = True, freeze_gc: bool = False,
                 lr_scheduler=None, use_graph: bool = False, device_scalars: Optional[bool] = None, encoder_stream: bool = True,
                 pack_stream: bool = True, use_ema: bool = False, ema_decay: float = 0.9999, ema_min_decay: float = 0.0,
                 ema_update_after_step: int = 0, use_ema_warmup: bool = False, ema_inv_gamma: float = 1.0, ema_power: float = 2 / 3,
                 use_8bit_adam: bool = False, gradient_checkpointing=False, deterministic: bool = False, independent_clips: bool = False):
        from . import autodiff as AD
        from . import grad_sync
        from . import train_graph as TG
        dev = unet.device
        if dev is None:
            raise RuntimeError("ControlNetTrainer: the U-Net has no weights loaded")
        if not any(gradient_checkpointing is v for v in (False, True)) and gradient_checkpointing != "all":
            raise ValueError(f"ControlNetTrainer: gradient_checkpointing must be False, True or \"all\"; got {gradient_checkpointing!r}")
        if use_graph and gradient_checkpointing:
            raise ValueError("ControlNetTrainer(use_graph=True) does not take gradient_checkpointing: the captured step exists to cut host "
                             "time, which the recomputation's launches add to, and it holds its buffers in one pool for the graph's "
                             "lifetime anyway, so dropping activations frees nothing")
        if use_graph and deterministic:
            raise ValueError("ControlNetTrainer(use_graph=True) does not take deterministic=True: the deterministic reductions take a workspace "
                             "per call from the allocator of the calling stream, and the captured step is out of the mode's scope")
        self.gradient_checkpointing = gradient_checkpointing
        self.independent_clips = bool(independent_clips)
        self._ckpt_cn, self._ckpt_dec = bool(gradient_checkpointing), gradient_checkpointing == "all"
        cfg = dict(controlnet_config)
        self.unet, self.device, self.config = unet, dev, cfg
        self.use_8bit_adam = bool(use_8bit_adam)
        self.params = AD.ParamStore(controlnet_state_dict, dev)
        self.lr, self.betas, self.weight_decay, self.eps = learning_rate, (adam_beta1, adam_beta2), adam_weight_decay, adam_epsilon
        self.optimizer = (optim.AdamW8bit if self.use_8bit_adam else optim.AdamW)(self.params, lr=self.lr, betas=self.betas, eps=self.eps,
                                                                                 weight_decay=self.weight_decay)
        self.deterministic = self.params.deterministic = bool(deterministic)
        self.controlnet = TG.ControlNetGraph(self.params, cfg)
        self._frozen = AD.FrozenParams({k: v for k, v in unet.state_dict().items() if k.startswith(("up_blocks.", "conv_norm_out.", "conv_out."))}, dev)
        self.decoder = TG.UNetDecoderGraph(self._frozen, dict(unet.config))
        self.accumulation, self.loss_scale, self.growth_interval = int(gradient_accumulation_steps), float(loss_scale), int(growth_interval)
        self.scaling_factor, self.dropout = scaling_factor, conditioning_dropout_prob
        self.optimizer_steps, self.skipped_steps, self._micro, self._clean = 0, 0, 0, 0
        self.lr_scheduler, self.last_lr = lr_scheduler, learning_rate
        self._accum_scale = None
        self.wgrad_stream, self._side = bool(wgrad_stream), None
        self.spatial_stream, self._sp_stream, self._packs_built = bool(spatial_stream), None, False
        self.encoder_stream, self._enc_stream = bool(encoder_stream), None
        self.pack_stream, self._pk_stream, self._packs_pending = bool(pack_stream), None, False
        # data parallel (accelerate's DDP, :1117-1119): one process per GPU, every rank its own clips; all ranks start from rank
        # 0's parameters and average their gradients - bucketed all-reduces over the flat buffer, overlapped with the backward
        grad_sync.broadcast_parameters(self.params.flat, process_group)
        self.buckets = grad_sync.GradientBuckets(self.params.grad, self.params.spans(), process_group, bucket_bytes=bucket_mb << 20)
        self.world = self.buckets.world
        self.ema = None                                   # (after the broadcast: the shadow starts as a clone of rank 0's parameters everywhere)
        if use_ema:
            from .training_utils import EMAModel
            self.ema = EMAModel(self.params, decay=ema_decay, min_decay=ema_min_decay, update_after_step=ema_update_after_step,
                                use_ema_warmup=use_ema_warmup, inv_gamma=ema_inv_gamma, power=ema_power, model_config=cfg)
        if self.world > 1:
            self.params.on_grad_ready = self.buckets.mark_ready
        # use_graph: forward + backward of a step replayed as ONE hipGraph (see loss_and_grads); device_scalars (implied by it): the
        # AlphaBlender weights of the trainable network are read from device memory instead of being passed as host floats
        self.use_graph = bool(use_graph)
        if self.use_graph and (self.world > 1 or self.accumulation != 1):
            raise ValueError("ControlNetTrainer(use_graph=True): one rank and gradient_accumulation_steps = 1 (the captured step holds no "
                             "collective and ends with complete gradients)")
        self.params.device_scalars = self.use_graph if device_scalars is None else bool(device_scalars)
        self._graphs, self._static, self._graph_pool = {}, None, None
        self._freeze_gc = 2 if freeze_gc else 0
        self._freeze()

    def _freeze(self) -> None:
        if self._freeze_gc > 0:
            self._freeze_gc -= 1
            gc.collect()
            gc.freeze()

    def unfreeze_gc(self) -> None:
        """Hand the objects ``freeze_gc`` moved to the permanent generation back to the collector (process-wide, like the freeze)."""
        gc.unfreeze()

    # -- forward + backward of one micro-batch; gradients ACCUMULATE in self.params.grad: after a whole cycle they are
    #    loss_scale x the gradient of the mean micro-batch loss
    def loss_and_grads(self, latents, encoder_hidden_states, motion_values, trajectories, *, use_spatial: bool = True, noise=None,
                       sigmas=None, random_p=None, ran_idx=None, generator=None, camera_cond=None) -> dict:
        """A micro-batch of ``B`` clips (``--per_gpu_batch_size``): ``latents`` ``[B, F, 4, h, w]``, ``encoder_hidden_states``
        ``[B, 1, D]``, ``motion_values`` ``[B]``, ``trajectories`` ``[B, F, 3, H, W]``, ``noise`` like ``latents``, ``sigmas`` / ``random_p``
        ``[B]``, ONE ``ran_idx`` (the reference draws one per step); a mismatched batch dimension is a ``ValueError`` naming the argument.
        The losses are the means over the clips, so every clip's gradient carries 1 / B.  ``camera_cond`` ``[B, F, 12]``: the camera twin's
        per-frame R|T (``scripts/train_svd_traj_VIPSeg_14_cam_concat.py:1393,1409``; that script has no spatial loss:
        ``use_spatial=False``)."""
        unet, dev = self.unet, self.device
        t_host = time.perf_counter()
        if camera_cond is not None and not self.config.get("camera"):
            raise ValueError("camera_cond given to a ControlNet without the camera branch (config camera=False)")
        I = _step_inputs(dev, latents, encoder_hidden_states, motion_values, trajectories, unet, scaling_factor=self.scaling_factor,
                         conditioning_dropout_prob=self.dropout, use_spatial=use_spatial, noise=noise, sigmas=sigmas, random_p=random_p,
                         ran_idx=ran_idx, generator=generator, kernel=False, lazy_traj=True, camera_cond=camera_cond)
        B, F, h, w = I["dims"]
        if B != 1 and self.use_graph:
            raise ValueError("ControlNetTrainer(use_graph=True) takes one clip per step: the captured step has not been verified for a batch "
                             f"(got {B} clips); build the trainer with use_graph=False for per_gpu_batch_size > 1")
        if self._accum_scale is None:                    # the loss scale of this accumulation cycle (it only changes between cycles)
            self._accum_scale = self.loss_scale
        scale = self._accum_scale / self.accumulation    # accelerate divides each micro-batch's loss by the number of micro-batches
        cam = I.pop("cam_host", None)
        if cam is not None:
            cam = cam.reshape(B * F, 12)
        ran_idx = I["ran_idx"]
        I["timesteps"] = I["timesteps"].to(device=dev, dtype=torch.float32)
        I["ehs"] = I["ehs"].to(device=dev, dtype=torch.float32)
        if cam is not None:
            I["cam"] = cam.to(device=dev, dtype=torch.float32).contiguous()
        # the step as a hipGraph: everything from the EDM preconditioning kernel to the last gradient is captured ONCE per (spatial frame
        # index, loss scale, input shapes) over static input buffers and replayed - ~6 000 launches, 60-70 ms of host enqueue time,
        # become one.  The first steps run eagerly: they build the packs, the side streams and take the first optimizer step.
        graphed = self.use_graph and self._packs_built and (self.optimizer_steps + self.skipped_steps) >= 1 and self._micro == 0 and self.accumulation == 1
        if graphed:
            I["traj"] = I.pop("traj_src").to(dev, torch.float16)              # (a replay reads every input from its static buffer)
            lt, ls = self._replay(I, ran_idx, bool(use_spatial), float(scale))
        else:
            lt, ls = self._run(I, ran_idx, bool(use_spatial), float(scale))
        self._micro += 1
        self._packs_built = self._packs_built or bool(use_spatial)
        t_host = time.perf_counter() - t_host                 # everything is enqueued; reading the loss is the first wait for the device
        loss_t = float(lt) if B == 1 else float(lt.mean())    # (per-clip means, then the mean over the clips: :1381-1386)
        out = dict(loss=loss_t, loss_temporal=loss_t, loss_spatial=None, grad_scale=scale, ran_idx=ran_idx, sigmas=I["sig_host"],
                   host_enqueue_ms=1000.0 * t_host, graph_replay=bool(graphed))
        if ls is not None:
            out["loss_spatial"] = float(ls) if B == 1 else float(ls.mean())
            out["loss"] = loss_t + 0.5 * out["loss_spatial"]
        return out

    _STATIC_KEYS = ("lat", "noise", "sig", "cond_scale", "timesteps", "ids", "ehs", "traj", "cam")

    def _replay(self, I: dict, ran_idx: int, use_spatial: bool, scale: float):
        """Copy the step's inputs into the static buffers of its graph (captured on first use) and replay it."""
        names = [k for k in self._STATIC_KEYS if k in I]
        key = (ran_idx, use_spatial, scale) + tuple((k, tuple(I[k].shape), I[k].dtype) for k in names)
        if self._static is None or any(k not in self._static or self._static[k].shape != I[k].shape or self._static[k].dtype != I[k].dtype for k in names):
            self._static = {k: torch.empty_like(I[k]) for k in names}          # (new shapes: the graphs over the old buffers are dropped)
            self._graphs = {}
        for k in names:
            self._static[k].copy_(I[k], non_blocking=True)
        entry = self._graphs.get(key)
        if entry is None:
            S = dict(I)
            S.update(self._static)
            self.params.version += 1                      # every version-keyed refresh (fp16 mirror, weight packs) is part of the capture: the
            torch.cuda.synchronize()                      # replayed step always follows an optimizer step, whatever this one follows
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=self._graph_pool):
                lt, ls = self._run(S, ran_idx, use_spatial, scale)
            if self._graph_pool is None:
                self._graph_pool = g.pool()               # one memory pool for all graphs of this trainer: they never run concurrently
            entry = self._graphs[key] = (g, lt, ls)
        entry[0].replay()
        return entry[1], entry[2]

    def warm_graphs(self, latents, encoder_hidden_states, motion_values, trajectories, *, use_spatial: bool = True, **draws) -> int:
        """Capture the step's graph for every spatial frame index (``ran_idx`` is drawn per step: 0 .. F - 1) WITHOUT training on them: the
        gradients each capture's first replay accumulates are discarded.  Returns the number of graphs held.  (A capture costs about
        one eager step; a training run that does not call this captures each index the first time it is drawn.)"""
        if not self.use_graph:
            return 0
        F = latents.shape[1]
        micro, accum = self._micro, self._accum_scale
        for r in range(F):
            d = dict(draws)
            d["ran_idx"] = r
            self.loss_and_grads(latents, encoder_hidden_states, motion_values, trajectories, use_spatial=use_spatial, **d)
            self._micro, self._accum_scale = micro, accum
        torch.cuda.synchronize()
        self.params.zero_grad()
        return len(self._graphs)

    def _run(self, I: dict, ran_idx: int, use_spatial: bool, scale: float):
        """Forward and backward of one micro-batch from device-resident inputs ``I`` - the part of the step that a hipGraph can hold: no
        host value that changes between steps is passed to a launch (the AlphaBlender weights come from ``ParamStore.alphas``, the loss
        scale and the spatial frame index are part of the graph's key).  Returns the two loss tensors (spatial: None)."""
        from . import autodiff as AD
        unet, dev = self.unet, self.device
        B, F, h, w = I["dims"]
        if self.params.device_scalars:
            self.params.refresh_alphas()
        _edm_train_input(I)
        lat, noisy, sig, timesteps, ids = I["lat"], I["noisy"], I["sig"], I["timesteps"], I["ids"]
        ehs16 = I["ehs"].to(dtype=torch.float16).reshape(B, -1).contiguous()
        inp = I["x"].permute(0, 1, 4, 2, 3)
        L = hip.checked()
        # three tapes: the ControlNet's forward, the decoder pass of the temporal loss and the one-frame decoder pass of the spatial
        # loss.  The spatial pass is 1/14 of the work in ~1 500 launches over 180 ... 2 880 rows - latency, not throughput - and
        # depends on the temporal pass nowhere between the ControlNet's outputs and the join of the residual gradients: it runs on
        # a stream of its own beside the temporal pass, forward and backward.
        tape_cn, tape, tape_sp = AD.Tape(), AD.Tape(), AD.Tape()
        # independent_clips on a batch: the frozen encoder (inference kernels: vec_mode 3 over B rows, no CFG halves) and the two tapes
        # (add_rowvec, one row per clip) give every clip its own temporal context; B = 1 and the default add no argument to any call
        ind = self.independent_clips and B > 1
        ind_enc = dict(independent_clips=B) if ind else {}
        ind_tape = dict(independent_clips=True) if ind else {}
        cam = I.get("cam")
        main = torch.cuda.current_stream()
        # the frozen U-Net's encoder half (inference kernels, no tape) depends on the ControlNet nowhere: it runs on a stream of its own
        # beside the ControlNet's forward, as in the inference loop (round 6; the step is device-bound - as a hipGraph it takes what it
        # takes eagerly - and at 320 x 576 no launch of the two encoders fills the chip)
        state = None
        if self.encoder_stream:
            if self._enc_stream is None:
                self._enc_stream = torch.cuda.Stream()
            with torch.no_grad():
                state = unet._encode_on(self._enc_stream, inp, timesteps, I["ehs"], ids, **ind_enc)
        if "traj" not in I:                                   # staged here, behind the encoder's launches: the device is busy meanwhile
            I["traj"] = I.pop("traj_src").to(dev, torch.float16)
        if self._packs_pending:                               # the packs re-written behind the last optimizer step (their own stream)
            main.wait_stream(self._pk_stream)
            self._packs_pending = False
        traj = I["traj"][0] if B == 1 else I["traj"].reshape((B * F,) + tuple(I["traj"].shape[2:]))
        outs, mid = self.controlnet.run(tape_cn, I["x"].view(B * F * h * w, 8), (B * F, h, w), timesteps, ehs16, ids, traj, camera_cond=cam,
                                        checkpoint=self._ckpt_cn, **ind_tape)
        with torch.no_grad():
            emb_silu = unet.time.run(timesteps, ids, B)

        def loss_of(p: AD.Var, nz, tg, frames, weight):      # per-clip losses [B]; the gradient is that of their mean (the kernel divides by B)
            out = torch.empty(B, dtype=torch.float32, device=dev)
            L.pt_edm_loss(p.v.data_ptr(), 0, p.v.shape[-1], nz.data_ptr(), tg.data_ptr(), sig.data_ptr(), B, frames, h * w,
                          out.data_ptr(), ops._stream())
            g = torch.empty((p.v.shape[0], 8), dtype=torch.float16, device=dev)
            L.pt_edm_loss_bwd(p.v.data_ptr(), 0, p.v.shape[-1], nz.data_ptr(), tg.data_ptr(), sig.data_ptr(), B, frames, h * w,
                              float(scale * weight), g.data_ptr(), ops._stream())
            p.g = g
            return out

        ls, deferred = None, []
        spatial_stream = None
        if use_spatial:                                                                          # :1388-1407
            # the frozen decoder's weight packs (forward, transposed, split) are built lazily by whichever pass touches a layer
            # first - device kernels on THAT pass's stream - and both passes read them: until every pack exists (the first step with
            # a spatial pass) the two passes share the main stream, so that no pack is read across streams without an event
            if self.spatial_stream and self._packs_built:
                if self._sp_stream is None:
                    self._sp_stream = torch.cuda.Stream()
                spatial_stream = self._sp_stream
                spatial_stream.wait_stream(main)                                                # ControlNet outputs, emb_silu, inputs
            with torch.cuda.stream(spatial_stream) if spatial_stream is not None else _null():
                with torch.no_grad():
                    state_s = unet._encode(inp[:, ran_idx].unsqueeze(1), timesteps, I["ehs"], ids, **ind_enc)
                mult_s = unet._multiplicity(state_s, len(outs))
                def frame(o):                                # clip b's own rows of frame ran_idx, b = 0 .. B - 1 (a batch of B one-frame clips)
                    n = o.v.shape[0] // (B * F)
                    parts = [AD.rows(tape_sp, o, (b * F + ran_idx) * n, (b * F + ran_idx + 1) * n, defer=deferred) for b in range(B)]
                    return parts[0] if B == 1 else AD.concat_rows(tape_sp, parts)

                res_s = [frame(o) for o in outs]
                mid_s = frame(mid)
                pred_s = self.decoder.run(tape_sp, state_s, mult_s, res_s, mid_s, emb_silu, ehs16, checkpoint=self._ckpt_dec, **ind_tape)
                ls = loss_of(pred_s, noisy[:, ran_idx:ran_idx + 1].contiguous(), lat[:, ran_idx:ran_idx + 1].contiguous(), 1, 0.5)
        if state is None:
            with torch.no_grad():
                state = unet._encode(inp, timesteps, I["ehs"], ids, **ind_enc)
        else:
            unet._join_encoded(state, self._enc_stream)
        mult = unet._multiplicity(state, len(outs))
        pred = self.decoder.run(tape, state, mult, outs, mid, emb_silu, ehs16, checkpoint=self._ckpt_dec, **ind_tape)
        lt = loss_of(pred, noisy, lat, F, 1.0)
        sync = self._micro + 1 >= self.accumulation          # inside an accumulation cycle only the last micro-batch synchronises
        if sync:
            self.buckets.begin(signature=(bool(use_spatial), cam is not None))
        if self.wgrad_stream and self._side is None:
            self._side = torch.cuda.Stream()
        AD.WGRAD_STREAM = self._side if self.wgrad_stream else None
        self.buckets.streams = [main, AD.WGRAD_STREAM]
        AD.DETERMINISTIC = self.params.deterministic         # (every reduction with atomics lies in the reverse pass: the tapes' closures)
        try:
            if use_spatial:                                   # the frozen decoder has no weight gradients: nothing of this pass leaves its stream
                with torch.cuda.stream(spatial_stream) if spatial_stream is not None else _null():
                    tape_sp.backward()
            tape.backward()                                   # temporal pass: the decoder's reverse, on the main stream
            if spatial_stream is not None:
                main.wait_stream(spatial_stream)
            for x_, r0_, r1_, dy_ in deferred:                # join: the spatial pass's residual gradients land in frame ran_idx's rows
                AD.add_rows(x_, r0_, r1_, dy_)
            tape_cn.backward()
        finally:
            AD.WGRAD_STREAM, AD.DETERMINISTIC = None, False
        if self.wgrad_stream:
            main.wait_stream(self._side)                      # every weight gradient is in before anyone reads the buffer
        if sync:
            self.buckets.finish()                             # the gradients are now the SUM over ranks
        return lt, ls

    def gradients(self) -> dict:
        """The accumulated gradients, un-scaled (and averaged over the ranks once synchronised), by parameter name (fp32)."""
        inv = 1.0 / ((self._accum_scale or 1.0) * (self.world if self._micro >= self.accumulation else 1))
        return {k: self.params.gradient(k) * inv for k in self.params.names}

    def grad_norm(self) -> float:
        """Global L2 norm of the (un-scaled) gradients; ``inf`` / ``nan`` when an fp16 gradient overflowed."""
        acc = torch.zeros(1, dtype=torch.float64, device=self.device)
        L, P = hip.checked(), self.params
        if P.deterministic:
            ws = torch.empty(L.ptd_sumsq_ws_floats(P.numel), dtype=torch.float32, device=self.device)
            L.ptd_sumsq_f32(P.grad.data_ptr(), P.numel, acc.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream())
        else:
            L.pt_sumsq_f32(P.grad.data_ptr(), P.numel, acc.data_ptr(), ops._stream())
        return math.sqrt(float(acc)) / ((self._accum_scale or 1.0) * self.world) if math.isfinite(float(acc)) else float(acc)

    def optimizer_step(self, grad_norm: Optional[float] = None) -> bool:
        """``optimizer.step(); optimizer.zero_grad()`` (``:1423-1425``) under the GradScaler's rules.  Returns whether the
        parameters moved.  ``grad_norm``: the value of ``grad_norm()`` if the caller already has it."""
        if self._accum_scale is None:
            raise RuntimeError("ControlNetTrainer.optimizer_step: no gradients accumulated since the last step")
        norm = self.grad_norm() if grad_norm is None else grad_norm
        took = math.isfinite(norm)
        ema = self.ema
        omd = ema.begin_step() if ema is not None else None          # EMAModel.step's counter and decay: taken or skipped (:1428-1430)
        if took:
            if self.lr_scheduler is not None:            # LambdaLR: the rate of step k (0-based) is base x lambda(k); a skipped step
                self.last_lr = self.lr * float(self.lr_scheduler(self.optimizer_steps))          # does not advance the schedule
            else:
                self.last_lr = self.lr
            self.optimizer_steps += 1
            P = self.params
            inv_scale = 1.0 / (self._accum_scale * self.world)
            # AdamW + the fp16 mirror of the new parameters + the gradient's zeroing in ONE pass over the buffers - and the EMA of the
            # new parameters in the same pass, when it is fused
            fused = ema is not None and self.ema_fused
            self.optimizer.step(self.last_lr, self.optimizer_steps, inv_scale, ema.shadow if fused else None, omd if fused else 0.0)
            if ema is not None and not fused:
                ema.update(omd)
            P.moved_with_mirror()                         # (half_view() need not cast the buffer again)
            if self.pack_stream and self._packs_built and not self.use_graph:
                # the new weights' fp16 packs, all layers at once, on a stream of their own behind AdamW (the next step's ControlNet
                # forward waits for it; the frozen encoder, the input staging and the host's bookkeeping do not)
                if self._pk_stream is None:
                    self._pk_stream = torch.cuda.Stream()
                self._pk_stream.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(self._pk_stream):
                    P.refresh_packs()
                self._packs_pending = True
            self._clean += 1
            if self._clean >= self.growth_interval:
                self.loss_scale, self._clean = self.loss_scale * 2.0, 0
        else:
            self.skipped_steps += 1
            self.loss_scale, self._clean = self.loss_scale * 0.5, 0
            if ema is not None:                           # the shadow moves toward the unchanged parameters
                ema.update(omd)
        if not took:
            self.params.zero_grad()
        self._micro, self._accum_scale = 0, None
        self._freeze()                                   # the first step built the fp16 packs, the streams, the gradient-producing set
        return took

    def step(self, latents, encoder_hidden_states, motion_values, trajectories, **draws) -> dict:
        """One iteration of the training loop's body: forward, backward and - every ``gradient_accumulation_steps`` calls - the
        optimizer step."""
        out = self.loss_and_grads(latents, encoder_hidden_states, motion_values, trajectories, **draws)
        out["stepped"] = None
        if self._micro >= self.accumulation:
            out["grad_norm"] = self.grad_norm()
            out["stepped"] = self.optimizer_step(out["grad_norm"])
        return out

    # EMA on a taken step: inside the AdamW launch (True) or as pt_ema_update_f32 behind pt_adamw_fused_f32 (False) - the same numbers
    # either way; tools/train_step_bench.py --ema {fused,separate} runs both.  Measured at 682 M parameters: 6.00 ms against 4.84 + 1.69
    # (profiles/r07/train_step_ema_ab.txt)
    ema_fused = True

    def ema_state_dict(self) -> dict:
        """The averaged weights by parameter name (fp32): what a validation pipeline or the final export loads under ``--use_ema``."""
        if self.ema is None:
            raise RuntimeError("ControlNetTrainer.ema_state_dict: the trainer was built with use_ema=False")
        return self.ema.shadow_state_dict()

    def state_dict(self) -> dict:
        """The ControlNet's current fp32 parameters (``controlnet.save_pretrained`` of ``:1440-1470`` writes these)."""
        return self.params.state_dict()

    def save_pretrained(self, path: str) -> None:
        """``controlnet.save_pretrained(path)``: ``ControlNetSDVModel.from_pretrained(path)`` reads it back."""
        from . import train_state
        train_state.save_controlnet(self, path)

    def save_state(self, output_dir: str) -> None:
        """``accelerator.save_state(output_dir)`` (``:1464-1466``): parameters, AdamW moments, step count, loss-scale state."""
        from . import train_state
        train_state.save_state(self, output_dir)

    def load_state(self, input_dir: str) -> dict:
        """``accelerator.load_state(input_dir)`` (``:1241``)."""
        from . import train_state
        return train_state.load_state(self, input_dir)
