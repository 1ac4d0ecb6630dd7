"""MI355X-native ``StableVideoDiffusionPipelineControlNet`` - the denoise loop of
``/root/reference/pipeline/pipeline_stable_video_diffusion_controlnet.py:316-599`` (and of the ``_cam`` twin:
``camera_cond`` argument, ``..._cam.py:321,505-509,549``) behind the reference's ``__call__`` signature.

Scope: steps 4-8 of ``__call__`` - timesteps, latents, control tensor, guidance ramp, hard-coded
micro-conditioning, the 25-iteration loop - plus the stages either side of it: ``_encode_image`` (the
anti-aliased resize runs in ``pt_resize_antialias_f32``, the CLIP vision tower is ``posetraj_amd.clip_vision`` or any
callable with the ``transformers`` interface), ``_encode_vae_image`` with the noise augmentation of the first frame, and after
the loop ``decode_latents`` (``:225-251``) + ``tensor2vid`` (``:70-83``) over ``posetraj_amd.autoencoder_kl_temporal_decoder``,
so ``output_type`` "pil" / "np" / "pt" / "latent" all work as in the reference.  Without ``image_encoder`` / ``vae`` the
outputs of those stages can be passed in (``image_embeddings`` / ``image_latents``) and ``output_type`` must be "latent".

Per step the loop launches: one fused prologue (CFG duplicate + 1/sqrt(sigma^2+1) + image-latent concat, written
channels-last), ControlNet, U-Net, one fused epilogue (per-frame guidance + Euler update on fp32 latents).
"""
from __future__ import annotations

import json
import os
from typing import Callable, Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from . import ops
from .control_schedule import check_control_weight, control_plan, is_scale_sequence, pool_control_weight, tap_sizes
from .controlnet_sdv import ControlNetSDVModel
from .modeling import BaseOutput
from .scheduling_euler_discrete_karras_fix import PREDICTION_TYPES, EulerDiscreteScheduler
from .step_graphs import GraphKey, StepGraphs, StepState
from .unet_spatio_temporal_condition_controlnet import UNetSpatioTemporalConditionControlNetModel


class StableVideoDiffusionPipelineOutput(BaseOutput):
    """``frames`` (``pipeline...:85-96``)."""


def _append_dims(x, target_dims):
    """``pipeline...:62-67``."""
    dims_to_append = target_dims - x.ndim
    if dims_to_append < 0:
        raise ValueError(f"input has {x.ndim} dims but target_dims is {target_dims}, which is less")
    return x[(...,) + (None,) * dims_to_append]


def _get_add_time_ids(noise_aug_strength, dtype, batch_size, fps=4, motion_bucket_id=128, unet=None):
    """Module-level helper of the reference (``pipeline...:37-59``) including its config check."""
    add_time_ids = [fps, motion_bucket_id, noise_aug_strength]
    passed = unet.config.addition_time_embed_dim * len(add_time_ids)
    expected = unet.add_embedding.linear_1.in_features
    if expected != passed:
        raise ValueError(f"Model expects an added time embedding vector of length {expected}, but a vector of {passed} was created. The model has an incorrect config. Please check `unet.config.time_embedding_type` and `text_encoder_2.config.projection_dim`.")
    return torch.tensor([add_time_ids], dtype=dtype)


def randn_tensor(shape, generator=None, device=None, dtype=None, layout=None):
    """``diffusers.utils.torch_utils.randn_tensor`` (called at ``pipeline...:292,451``): N(0,1) of ``shape`` on ``device``.
    A generator on another device type (the usual seeded CPU generator) samples there and the result is moved; a list of
    generators samples one batch entry each."""
    device = torch.device(device) if device is not None else torch.device("cpu")
    batch = shape[0]

    def one(shp, g):
        gdev = g.device if g is not None else device
        if gdev.type != device.type and gdev.type != "cpu":
            raise ValueError(f"Cannot generate a {device} tensor from a generator of type {gdev.type}.")
        on = device if gdev.type == device.type else torch.device("cpu")
        return torch.randn(tuple(shp), generator=g, device=on, dtype=dtype).to(device)

    if isinstance(generator, list) and len(generator) == 1:
        generator = generator[0]
    if isinstance(generator, list):
        return torch.cat([one((1,) + tuple(shape[1:]), generator[i]) for i in range(batch)], dim=0)
    return one(shape, generator)


def postprocess(image: torch.Tensor, output_type: str = "pil"):
    """``VaeImageProcessor.postprocess`` (diffusers 0.24.0) for one clip ``[F, 3, H, W]`` in [-1, 1]:
    ``(x / 2 + 0.5).clamp(0, 1)`` then "pt": that tensor; "np": ``[F, H, W, 3]`` float32 on the host; "pil": a list of
    ``PIL.Image`` from ``round(255 x)``; "latent": the input.  Runs in ``pt_frames_postprocess``."""
    if output_type == "latent":
        return image
    if output_type not in ("pt", "np", "pil"):
        raise ValueError(f"output_type {output_type!r} is not supported; choose one of 'pil', 'np', 'pt', 'latent'")
    x = ops.frames_postprocess(image.to(torch.float32), output_type)
    if output_type == "pt":
        return x
    arr = x.cpu().numpy()
    if output_type == "np":
        return arr
    import PIL.Image
    return [PIL.Image.fromarray(a) for a in arr]


def tensor2vid(video: torch.Tensor, processor=None, output_type="np"):
    """``pipeline...:70-83``: ``video`` ``[batch, 3, frames, H, W]`` -> a list with one ``postprocess``-ed clip per batch entry."""
    post = processor.postprocess if processor is not None else postprocess
    outputs = []
    for batch_idx in range(video.shape[0]):
        outputs.append(post(video[batch_idx].permute(1, 0, 2, 3), output_type))
    return outputs


class _ImageProcessor:
    """The two ``VaeImageProcessor`` entry points the reference pipeline calls (``:143,454,588``)."""

    def __init__(self, vae_scale_factor=8):
        self.vae_scale_factor = vae_scale_factor

    def preprocess(self, image, height=None, width=None):
        return StableVideoDiffusionPipelineControlNet.preprocess_condition(image, height, width)

    @staticmethod
    def postprocess(image, output_type="pil"):
        return postprocess(image, output_type)


class StableVideoDiffusionPipelineControlNet:
    model_cpu_offload_seq = "image_encoder->unet->vae"
    _callback_tensor_inputs = ["latents"]

    def __init__(self, vae=None, image_encoder=None, unet: UNetSpatioTemporalConditionControlNetModel = None,
                 controlnet: ControlNetSDVModel = None, scheduler: EulerDiscreteScheduler = None, feature_extractor=None):
        self.vae, self.image_encoder, self.unet = vae, image_encoder, unet
        self.controlnet, self.scheduler, self.feature_extractor = controlnet, scheduler, feature_extractor
        self.vae_scale_factor = 8 if vae is None else 2 ** (len(vae.config.block_out_channels) - 1)
        self.image_processor = _ImageProcessor(self.vae_scale_factor)
        self._guidance_scale = None
        self._num_timesteps = 0
        self._step_graphs = StepGraphs()            # captured hipGraphs of the per-iteration networks (denoise(use_graph=True)), one per kind of step
        self._side_stream = None                    # second HIP stream of denoise(overlap_streams=True)

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path: str, controlnet: ControlNetSDVModel = None,
                        unet: UNetSpatioTemporalConditionControlNetModel = None, scheduler: EulerDiscreteScheduler = None,
                        vae=None, image_encoder=None, device="cuda", variant: Optional[str] = None, **kw):
        """The construction the reference's callers use (``scripts/run_inference_vipseg_json_repro.py:335-339``):
        ``from_pretrained(svd_dir, controlnet=controlnet, unet=unet)``.  Reads the diffusers directory layout of the SVD
        checkpoint: ``scheduler/scheduler_config.json`` for the sampler, ``unet/`` when no ``unet`` is passed, and - when the
        sub-directories exist and no module is passed - ``vae/`` (``AutoencoderKLTemporalDecoder``) and ``image_encoder/``
        (``CLIPVisionModelWithProjection``, transformers' ``config.json`` + ``model[.variant].safetensors``)."""
        from .autoencoder_kl_temporal_decoder import AutoencoderKLTemporalDecoder
        from .clip_vision import CLIPVisionModelWithProjection
        root = pretrained_model_name_or_path
        if scheduler is None:
            path = os.path.join(root, "scheduler", "scheduler_config.json")
            if os.path.exists(path):
                with open(path) as f:
                    cfg = {k: v for k, v in json.load(f).items() if not k.startswith("_")}
                scheduler = EulerDiscreteScheduler(**cfg)
            else:
                from .scheduling_euler_discrete_karras_fix import SVD_SCHEDULER_CONFIG
                scheduler = EulerDiscreteScheduler(**SVD_SCHEDULER_CONFIG)
        if unet is None:
            unet = UNetSpatioTemporalConditionControlNetModel.from_pretrained(root, subfolder="unet", device=device, variant=variant)
        if controlnet is None:
            raise ValueError("pass `controlnet=` (the reference always does: ControlNetSDVModel.from_pretrained(ckpt, subfolder='controlnet'))")
        if vae is None and os.path.exists(os.path.join(root, "vae", "config.json")):
            vae = AutoencoderKLTemporalDecoder.from_pretrained(root, subfolder="vae", device=device, variant=variant)
        if image_encoder is None and os.path.exists(os.path.join(root, "image_encoder", "config.json")):
            image_encoder = CLIPVisionModelWithProjection.from_pretrained(root, subfolder="image_encoder", device=device, variant=variant)
        return cls(vae=vae, image_encoder=image_encoder, unet=unet, controlnet=controlnet, scheduler=scheduler)

    @staticmethod
    def preprocess_condition(controlnet_condition, height: int, width: int) -> torch.Tensor:
        """``self.image_processor.preprocess(controlnet_condition, height=, width=)`` of ``pipeline...:500``
        (diffusers 0.24.0 ``VaeImageProcessor.preprocess`` [UNVERIFIED-MEMORY: diffusers is not in the tree]): a list of
        PIL images / ``[F, H, W, 3]`` [0,1] float (or uint8) arrays is resized to ``width x height`` (PIL lanczos), scaled to
        [0, 1], laid out ``[F, 3, H, W]`` and normalised to [-1, 1]; a ``[F, 3, H, W]`` tensor is resized with
        ``interpolate`` when its size differs and normalised only if it has no negative value (a tensor that already is
        in [-1, 1] passes through).  Host-side data formatting: a few MB once per clip."""
        c = controlnet_condition
        if torch.is_tensor(c):
            x = c.float()
            if x.dim() == 3:
                x = x.unsqueeze(0)
            if tuple(x.shape[-2:]) != (height, width):
                x = torch.nn.functional.interpolate(x, size=(height, width))
            return x if float(x.min()) < 0 else 2.0 * x - 1.0
        frames = list(c) if isinstance(c, (list, tuple)) else [c]
        out = []
        for fr in frames:
            if hasattr(fr, "resize") and hasattr(fr, "convert"):                       # PIL.Image
                import PIL.Image
                a = np.asarray(fr.convert("RGB").resize((width, height), resample=PIL.Image.LANCZOS), dtype=np.float32) / 255.0
            else:                                                                      # arrays are [0, 1] floats in diffusers;
                a = np.asarray(fr)                                                     # uint8 pixels are accepted as a convenience
                a = a.astype(np.float32) / 255.0 if a.dtype == np.uint8 else a.astype(np.float32)
                if a.shape[:2] != (height, width):
                    a = torch.nn.functional.interpolate(torch.from_numpy(a).permute(2, 0, 1)[None], size=(height, width))[0].permute(1, 2, 0).numpy()
            out.append(torch.from_numpy(np.ascontiguousarray(a)).permute(2, 0, 1))
        return 2.0 * torch.stack(out) - 1.0

    # -- no-op compatible surface of DiffusionPipeline used by the reference's callers
    def to(self, *a, **k):
        return self

    def enable_model_cpu_offload(self, *a, **k):
        pass

    def set_progress_bar_config(self, **k):
        pass

    def maybe_free_model_hooks(self):
        pass

    @property
    def guidance_scale(self):
        return self._guidance_scale

    @property
    def num_timesteps(self):
        return self._num_timesteps

    def check_inputs(self, image, height, width):
        """``pipeline...:253-265``."""
        if height % 8 != 0 or width % 8 != 0:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")

    @staticmethod
    def _check_independent_requests(image, controlnet_condition, generator, camera_cond, latents, image_embeddings, image_latents,
                                    num_videos_per_prompt, num_frames) -> int:
        """The arguments of ``__call__(independent_clips=True)`` -> K, the number of requests.  Host only; every mismatch is a
        ``ValueError`` that names the argument."""
        if image is None and image_embeddings is not None and image_latents is not None:      # both pre-loop stages done by the caller
            K = image_embeddings.shape[0] // 2
        elif not isinstance(image, (list, tuple)) or len(image) == 0:
            raise ValueError("independent_clips=True: `image` must be a list of K images, one per request")
        else:
            K = len(image)
        if num_videos_per_prompt not in (None, 1):
            raise ValueError(f"independent_clips=True: `num_videos_per_prompt` must be 1 (got {num_videos_per_prompt}); repeat the request in `image`")
        c = controlnet_condition
        if torch.is_tensor(c):
            if c.dim() != 5 or c.shape[0] != K:
                raise ValueError(f"independent_clips=True: `controlnet_condition` must be a list of {K} map sets or a [{K}, F, 3, H, W] "
                                 f"tensor; got a tensor of shape {tuple(c.shape)}")
        elif not isinstance(c, (list, tuple)) or len(c) != K:
            raise ValueError(f"independent_clips=True: `controlnet_condition` must hold {K} map sets, one per image; got "
                             f"{len(c) if isinstance(c, (list, tuple)) else type(c).__name__}")
        if isinstance(generator, (list, tuple)) and len(generator) != K:
            raise ValueError(f"independent_clips=True: `generator` must be one generator or a list of {K}; got a list of {len(generator)}")
        if camera_cond is not None:
            cam = torch.as_tensor(camera_cond)
            if cam.dim() != 3 or tuple(cam.shape[:2]) != (K, num_frames):
                raise ValueError(f"independent_clips=True: `camera_cond` must be [{K}, {num_frames}, 12]; got {tuple(cam.shape)}")
        for name, t, n in (("latents", latents, K), ("image_embeddings", image_embeddings, 2 * K), ("image_latents", image_latents, 2 * K)):
            if t is not None and t.shape[0] != n:
                raise ValueError(f"independent_clips=True: `{name}` must have {n} rows for {K} requests (uncond halves first); got {t.shape[0]}")
        return K

    def prepare_latents(self, batch_size, num_frames, num_channels_latents, height, width, dtype, device, generator,
                        latents=None):
        """``pipeline...:267-299``: N(0,1) * init_noise_sigma."""
        shape = (batch_size, num_frames, num_channels_latents // 2, height // self.vae_scale_factor,
                 width // self.vae_scale_factor)
        if isinstance(generator, list) and len(generator) != batch_size:
            raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an effective batch size of {batch_size}. Make sure the batch size matches the length of the generators.")
        if latents is None:
            latents = randn_tensor(shape, generator=generator, device=device, dtype=dtype)
        else:
            latents = latents.to(device)
        return latents * self.scheduler.init_noise_sigma.to(latents.device)

    # ------------------------------------------------------------------------------------------ pre-loop conditioning
    def _encode_image(self, image, device, num_videos_per_prompt, do_classifier_free_guidance):
        """``pipeline...:145-172``: resize to 224 x 224 with ``_resize_with_antialiasing`` (no CLIP mean / std
        normalisation: the reference skips the feature extractor), ``image_encoder(image).image_embeds``,
        ``[B, 1, D]``, repeated per prompt; the CFG-negative half is zeros, concatenated in front."""
        if not torch.is_tensor(image):
            image = self._to_unit_tensor(image)               # pil_to_numpy + numpy_to_pt: [B, 3, H, W] in [0, 1]
        image = ops.resize_with_antialiasing(image.to(device=device, dtype=torch.float32), (224, 224))
        dtype = getattr(self.image_encoder, "dtype", None)
        if dtype is None and hasattr(self.image_encoder, "parameters"):
            dtype = next(self.image_encoder.parameters()).dtype
        out = self.image_encoder(image.to(dtype=dtype or torch.float32))
        image_embeddings = (out.image_embeds if hasattr(out, "image_embeds") else out).unsqueeze(1)
        bs_embed, seq_len, _ = image_embeddings.shape
        image_embeddings = image_embeddings.repeat(1, num_videos_per_prompt, 1).view(bs_embed * num_videos_per_prompt, seq_len, -1)
        if do_classifier_free_guidance:
            image_embeddings = torch.cat([torch.zeros_like(image_embeddings), image_embeddings])
        return image_embeddings

    def _encode_vae_image(self, image: torch.Tensor, device, num_videos_per_prompt, do_classifier_free_guidance):
        """``pipeline...:174-195``: ``vae.encode(image).latent_dist.mode()`` - NOT multiplied by ``scaling_factor`` - zeros
        for the CFG-negative half, repeated per prompt."""
        image_latents = self.vae.encode(image.to(device=device)).latent_dist.mode()
        if do_classifier_free_guidance:
            image_latents = torch.cat([torch.zeros_like(image_latents), image_latents])
        return image_latents.repeat(num_videos_per_prompt, 1, 1, 1)

    @staticmethod
    def _to_unit_tensor(image) -> torch.Tensor:
        """``VaeImageProcessor.pil_to_numpy`` + ``numpy_to_pt`` (``pipeline...:148-150``): PIL image(s) / ``[H, W, 3]`` arrays
        -> ``[B, 3, H, W]`` fp32 in [0, 1]."""
        frames = list(image) if isinstance(image, (list, tuple)) else [image]
        out = []
        for fr in frames:
            a = np.asarray(fr.convert("RGB") if hasattr(fr, "convert") else fr).astype(np.float32) / 255.0   # pil_to_numpy: always
            out.append(torch.from_numpy(np.ascontiguousarray(a)).permute(2, 0, 1))
        return torch.stack(out)

    # ------------------------------------------------------------------------------------------ after the loop
    def decode_latents(self, latents: torch.Tensor, num_frames: int, decode_chunk_size: int = 14) -> torch.Tensor:
        """``pipeline...:225-251``: ``[B, F, 4, h, w]`` -> fp32 ``[B, 3, F, 8h, 8w]``.  ``1 / scaling_factor``, then
        ``decode_chunk_size`` frames per ``vae.decode`` call with ``num_frames`` = the frames in that call (each call is one
        clip for the decoder's temporal layers; a chunk may span two clips when B > 1), results in frame order.  With this
        package's VAE every call writes its frames straight into the final buffer (no ``torch.cat`` pass)."""
        import inspect
        from .autoencoder_kl_temporal_decoder import AutoencoderKLTemporalDecoder
        vae, inv = self.vae, 1 / self.vae.config.scaling_factor
        flat = latents.flatten(0, 1)                                               # [B*F, 4, h, w]
        total = flat.shape[0]
        takes_num_frames = "num_frames" in inspect.signature(vae.forward).parameters
        spans = [(i, min(i + decode_chunk_size, total)) for i in range(0, total, decode_chunk_size)]
        if isinstance(vae, AutoencoderKLTemporalDecoder):
            z = ops.scale(flat if flat.dtype in (torch.float16, torch.float32) else flat.float(), inv)
            up = 2 ** (len(vae.config.block_out_channels) - 1)
            decoded = torch.empty((total, vae.config.out_channels, z.shape[2] * up, z.shape[3] * up), dtype=torch.float32, device=z.device)
            for lo, hi in spans:                                                   # each call writes its frames in place
                vae.decode(z[lo:hi], num_frames=hi - lo, out=decoded[lo:hi])
        else:                                                                      # any module with the diffusers call shape
            z = inv * flat
            parts = [vae.decode(z[lo:hi], **({"num_frames": hi - lo} if takes_num_frames else {})).sample for lo, hi in spans]
            decoded = torch.cat(parts, dim=0)
        video = decoded.reshape(-1, num_frames, *decoded.shape[1:]).permute(0, 2, 1, 3, 4)    # [B, 3, F, H, W]
        return video.float()

    # ------------------------------------------------------------------------------------------ the hot loop
    def _networks_step(self, kind, sample, t, emb, cond, cam, ids, scale, level_w, overlap, _networks, independent_clips: int = 0):
        """ControlNet + U-Net of one iteration -> fp32 channels-last prediction [2Bc, F, h, w, 4].  The zero-convs' epilogues add the
        ControlNet residuals straight into the U-Net's skips (no residual tensors, no add passes); with ``overlap`` the U-Net's encoder
        half runs beside the ControlNet on a second HIP stream.  ``kind`` "plain": ``scale`` is a scalar of those epilogues; "weighted":
        the factors in ``level_w`` with the step's scale folded in, the scalar stays 1; "off": no ControlNet, nothing to fork or join.
        ``independent_clips``: 0, or the number of clips ``Bc`` when each is to read its own context rows (``denoise``)."""
        if _networks is not None:            # tools/variants/split_cfg.py: another schedule of the same two networks (A/B only)
            return _networks(self, sample, t, emb, cond, cam, ids, scale)
        unet, cn = self.unet, self.controlnet
        ind = dict(independent_clips=independent_clips) if independent_clips else {}
        if kind == "off":
            enc = unet._encode(sample, t, emb, ids, **ind)
        else:
            if overlap and (self._side_stream is None or self._side_stream.device != sample.device):
                self._side_stream = torch.cuda.Stream(device=sample.device)
            enc = unet._encode_on(self._side_stream, sample, t, emb, ids, **ind) if overlap else unet._encode(sample, t, emb, ids, **ind)
            taps, xm = cn._features(sample, t, emb, ids, cond, cam if cn.config.camera else None, **ind)
            if overlap:
                unet._join_encoded(enc, self._side_stream)
            mult = unet._multiplicity(enc, len(taps))
            if kind == "weighted":
                cn._accumulate_into_weighted(taps, xm, 1.0, level_w, enc["skips"], mult, enc["x"])
            else:
                cn._accumulate_into(taps, xm, scale, enc["skips"], mult, enc["x"])
        pred_cl = unet._decode(enc, None, None, return_dict=False, residuals_added=True, out_f32=True)[0].permute(0, 1, 3, 4, 2)
        return pred_cl if pred_cl.is_contiguous() else pred_cl.contiguous()

    @torch.no_grad()
    def denoise(self, latents: torch.Tensor, image_latents: torch.Tensor, image_embeddings: torch.Tensor,
                controlnet_condition: torch.Tensor, num_inference_steps: int = 25, min_guidance_scale: float = 1.0,
                max_guidance_scale: float = 3.0, controlnet_cond_scale: Union[float, Sequence[float]] = 1.0,
                camera_cond: Optional[torch.Tensor] = None, callback_on_step_end: Optional[Callable] = None,
                callback_on_step_end_tensor_inputs: List[str] = ["latents"], use_graph: bool = False,
                overlap_streams: bool = False, _networks=None, control_guidance_start: float = 0.0,
                control_guidance_end: float = 1.0, control_weight: Optional[torch.Tensor] = None,
                independent_clips: bool = False, window_frames: Optional[int] = None, window_stride: Optional[int] = None,
                window_batch: Optional[int] = None) -> torch.Tensor:
        """``pipeline...:481-583``.  ``latents`` ``[Bc, F, 4, h, w]`` already scaled by ``init_noise_sigma``;
        ``image_latents`` ``[2*Bc, 4, h, w]`` (uncond halves first, one frame - it is repeated over frames, ``:466``);
        ``image_embeddings`` ``[2*Bc, 1, D]``; ``controlnet_condition`` ``[2*Bc, F, 3, H, W]`` in [-1, 1].
        Returns the denoised latents in the dtype of ``latents``.

        Control strength beyond the reference (``posetraj_amd.control_schedule``; a call that gives none of these runs exactly the
        launches it always ran):

        ``control_guidance_start`` / ``control_guidance_end``: diffusers' window - with ``N`` steps, step ``i`` runs the ControlNet iff
        ``not (i / N < start or (i + 1) / N > end)``; the other steps run the U-Net alone (no ControlNet launch at all).
        ``controlnet_cond_scale``: one float, or ``num_inference_steps`` floats, one per step; a step whose scale is exactly 0.0 is
        skipped like a step outside the window.
        ``control_weight``: ``[F, h, w]`` or ``[Bc, F, h, w]`` at latent resolution, finite, intended range [0, 1]: multiplies every
        ControlNet residual per frame and latent pixel (a tap of size ``(hh, ww)`` uses ``adaptive_avg_pool2d(control_weight, (hh, ww))``,
        pooled once per call); both classifier-free-guidance halves of a clip get the same weights.  Per-frame strength ``s [F]`` is
        the special case ``s[:, None, None].expand(F, h, w)``.
        A ``control_weight`` or a per-step scale sends the ControlNet steps through ``ControlNetSDVModel._accumulate_into_weighted``,
        whose factors live in device buffers: one captured graph serves every scale and every weight map.

        ``independent_clips`` (a departure from the reference, made on purpose; default ``False`` = the reference's batch): like the
        reference, a batch of ``Bc > 1`` clips is NOT ``Bc`` independent clips - the temporal blocks' cross-attention hands token
        ``(b, f, s)`` the image context of batch element ``(b S + s) mod 2 Bc`` (``models/modified_svd.py:152-159``), so one
        clip's video depends on another clip's image.  ``True``: every clip reads the two context rows, uncond and cond, that it reads in a
        call of its own, in the same interleave (``vec_mode=3``, include/posetraj_hip.h) - clip ``c`` of the batch is what a one-clip call
        computes for it, up to the summation order of batched launches; every other operator is per clip already.  Same tensors, same
        launches but for that index; graphs of the two modes are never shared.  ``Bc = 1`` is untouched: the flag then changes no launch.
        Not with ``_networks``.  No trained checkpoint is at hand to measure what the mode does to quality.

        ``window_frames`` (beyond the reference; default ``None`` = this loop as it always ran, launch for launch): a long video from a
        short-clip model.  ``latents`` is ONE request ``[1, Ft, 4, h, w]``; it is denoised as ``K`` overlapping windows of
        ``window_frames`` frames, ``window_stride`` apart (default ``window_frames // 2``; the last window ends on the last frame -
        ``posetraj_amd.windows.window_plan``), each window one ordinary clip evaluation on the slices a call on that window would get
        (``controlnet_condition [2, Ft, 3, H, W]``, ``camera_cond [2, Ft, 12]``, ``control_weight [Ft, h, w]``) with the request's own
        image latents, embedding and time ids; the guidance ramp runs over the frames of a window.  At every step the predictions of the
        windows that cover a frame are blended with normalised triangular weights, and the blended prediction takes the scheduler's
        step.  ``window_batch`` windows (a divisor of K; default K) go through the networks per evaluation as independent clips - the
        captured graph is that of an ``independent_clips`` batch of ``window_batch`` clips of ``window_frames`` frames, shared by all
        groups; fewer windows per evaluation save memory and reload each group's condition every step.  Every window is conditioned on
        the same first image.  Not with ``independent_clips`` or ``_networks``; a refusal is a ``ValueError`` naming the argument.  No
        trained checkpoint is at hand to measure quality."""
        if independent_clips and _networks is not None:
            raise ValueError("`independent_clips` does not go with `_networks` (another schedule of the two networks, A/B only): its split-CFG "
                             "forward takes one clip")
        if window_frames is None:
            if window_stride is not None or window_batch is not None:
                raise ValueError("`window_stride` / `window_batch` need `window_frames` (the windowed loop is off without it)")
        else:
            if independent_clips or _networks is not None:
                raise ValueError("`window_frames` serves one request through the loop's own networks: it does not go with "
                                 f"`{'independent_clips' if independent_clips else '_networks'}`")
            return self._denoise_windows(latents, image_latents, image_embeddings, controlnet_condition, num_inference_steps, min_guidance_scale,
                                         max_guidance_scale, controlnet_cond_scale, camera_cond, callback_on_step_end, use_graph, overlap_streams,
                                         control_guidance_start, control_guidance_end, control_weight, window_frames, window_stride, window_batch)
        plan = control_plan(num_inference_steps, controlnet_cond_scale, control_guidance_start, control_guidance_end)
        (Bc, F, _, h, w), dev, out_dtype = latents.shape, latents.device, latents.dtype
        control_weight = check_control_weight(control_weight, Bc, F, h, w)
        weighted = control_weight is not None or is_scale_sequence(controlnet_cond_scale)
        scheduled = weighted or (float(control_guidance_start), float(control_guidance_end)) != (0.0, 1.0)
        if scheduled and _networks is not None:
            raise ValueError("`_networks` (another schedule of the two networks, A/B only) serves the plain loop: no control window, per-step scale or weight")
        if max_guidance_scale <= 1.0:
            # The reference's non-CFG branch (:438, :532) cannot run: latents / embeddings stay [Bc, ...] but the control
            # maps (:501-503) and added_time_ids (:521) are doubled unconditionally, so ControlNetSDVModel.forward reshapes
            # the time ids to [Bc, 2 * 3 * D] and add_embedding's Linear raises (reference run: tests/golden/loop.npz,
            # `base_noncfg_error`).  Same exception type and message here.
            c = self.unet.config
            raise RuntimeError(f"mat1 and mat2 shapes cannot be multiplied ({Bc}x{2 * 3 * c.addition_time_embed_dim} and "
                               f"{c.projection_class_embeddings_input_dim}x{c.block_out_channels[0] * 4})")
        self.scheduler.set_timesteps(num_inference_steps, device=dev)
        self._num_timesteps, self.scheduler._step_index = len(self.scheduler.timesteps), None
        # per-frame guidance ramp (:506-511)
        g = torch.linspace(min_guidance_scale, max_guidance_scale, F).unsqueeze(0).to(dev, out_dtype).repeat(Bc, 1)
        self._guidance_scale = _append_dims(g, latents.ndim)
        guidance = g.to(torch.float32).contiguous()
        # micro-conditioning is hard-coded to fps 6 / bucket 128 / aug 0.02 whatever the caller asked (:513-523, Q4)
        added_time_ids = _get_add_time_ids(0.02, torch.float32, Bc, 6, 128, unet=self.unet).repeat(2 * Bc, 1).to(dev)   # torch.cat([ids] * 2)
        x = latents.to(torch.float32).contiguous().clone()
        il = image_latents.to(dev, torch.float16).contiguous()
        emb = image_embeddings.to(dev, torch.float16).contiguous()
        cond = controlnet_condition.to(dev, torch.float16)
        cam = None if camera_cond is None else camera_cond.to(dev, torch.float16)
        ptype, sig = PREDICTION_TYPES[self.scheduler.config.prediction_type], self.scheduler._sigmas_host
        # The three kinds of step (control_schedule): "plain" - the loop as the reference runs it, one scalar scale in the zero-convs'
        # epilogues; "weighted" - the residuals times a per-(frame, pixel) factor read from device buffers (control_weight, per-step
        # scales); "off" - outside the control window or scale 0: the U-Net alone.  Without the new arguments every step is plain.
        kinds = ["plain"] * len(plan) if not scheduled else [("weighted" if weighted else "plain") if on else "off" for on, _ in plan]
        step_scales = [s for _, s in plan]
        level_base = None                    # weighted: {(hh, ww): fp32 [2 Bc F hh ww]} pooled weights, pooled once per call on the device
        if "weighted" in kinds:
            cw = torch.ones((Bc, F, h, w), dtype=torch.float32, device=dev) if control_weight is None else control_weight.to(dev)
            level_base = pool_control_weight(cw, tap_sizes(h, w, len(self.controlnet.config.block_out_channels)))
        # One StepState per kind this call uses: with ``use_graph`` found in, or captured into, ``self._step_graphs`` under its key.
        independent = Bc if independent_clips and Bc > 1 else 0          # one clip: the launches it always ran
        run = lambda st, sample, t_: self._networks_step(st.kind, sample, t_, st.emb, st.cond, st.cam, st.ids, controlnet_cond_scale,
                                                         st.wbuf, overlap_streams, _networks, independent)
        geometry = GraphKey(Bc=Bc, F=F, hw=(h, w), cond_shape=tuple(cond.shape), cam_shape=None if cam is None else tuple(cam.shape),
                            kind=None, scale=None, unet=id(self.unet), controlnet=id(self.controlnet), unet_gen=self.unet._generation,
                            controlnet_gen=self.controlnet._generation, overlap=bool(overlap_streams),
                            networks_name=getattr(_networks, '__name__', None),
                            dispatch=ops.dispatch_key() + (("independent_clips", bool(independent)),)) if use_graph else None
        live = {}
        # The sampler: a scheduler of order 2 (DPMPP2MDiscreteScheduler) takes the multistep kernel with its own host-computed
        # coefficients and one more latent-sized tensor, the previous denoised estimate; any other takes the Euler kernel.  Both run
        # after the networks, outside the captured graphs: one graph serves both schedulers.
        multistep = getattr(self.scheduler, "order", 1) == 2
        d_prev = torch.empty_like(x) if multistep else None
        for i in range(self._num_timesteps):
            t = self.scheduler._timesteps_host[i]
            if self.scheduler._step_index is None:
                self.scheduler._init_step_index(t)
            k = self.scheduler._step_index
            kind = kinds[i]
            st = live.get(kind)
            if st is None:                   # the first step of its kind in this call
                key = geometry and geometry._replace(kind=kind, scale=float(controlnet_cond_scale) if kind == "plain" else None)
                st = live[kind] = (key and self._step_graphs.get(key)) or StepState(kind, run, key)
                st.load(emb, added_time_ids, cond, cam, level_base, self.controlnet)
                if use_graph and st.graph is None:
                    st.capture(self._step_graphs.pool_for(key), x, il, sig[k], t)
                    self._step_graphs.insert(key, st)
            st.fold(step_scales[i])
            pred_cl = st.step(x, il, sig[k], t)                                            # [2Bc, F, h, w, 4] fp32
            if multistep:                    # DPM-Solver++(2M): this call's first step has no previous estimate (c = 0: d_prev is written, not read)
                ops.cfg_multistep_step(pred_cl, guidance, self.scheduler.coefficients(k, first=i == 0), x, d_prev)
            else:
                ops.cfg_euler_step(pred_cl, guidance, sig[k], sig[k + 1], ptype, x)
            self.scheduler._step_index += 1
            self.scheduler.is_scale_input_called = True
            if callback_on_step_end is not None:
                cb_latents = x.to(out_dtype)
                outs = callback_on_step_end(self, i, t, {"latents": cb_latents})
                new = outs.pop("latents", cb_latents)
                # always take what the callback hands back - it may have edited `latents` in place and returned the same
                # object.  For fp16 latents this rounds the state through fp16 once per step, as the reference does.
                if new is not x:
                    x = new.to(torch.float32).contiguous().clone()
        return x.to(out_dtype)

    def _denoise_windows(self, latents, image_latents, image_embeddings, controlnet_condition, num_inference_steps, min_guidance_scale,
                         max_guidance_scale, controlnet_cond_scale, camera_cond, callback_on_step_end, use_graph, overlap_streams,
                         control_guidance_start, control_guidance_end, control_weight, window_frames, window_stride, window_batch):
        """``denoise(window_frames=...)``.  Per step and group of ``G = window_batch`` windows: the window prologue into the
        state's input, the networks as ``G`` independent clips of ``Fw`` frames (the state, key and graph of such a batch); then, once
        per step, guidance + blend of the K predictions into one ``[Ft, 4, h, w]`` prediction and the scheduler's flat step kernel."""
        from . import windows as W
        if latents.dim() != 5 or latents.shape[0] != 1:
            raise ValueError(f"`window_frames` serves one request: `latents` must be [1, num_frames, 4, h, w]; got {tuple(latents.shape)}")
        (_, Ft, _, h, w), dev, out_dtype = latents.shape, latents.device, latents.dtype
        wplan, G = W.resolve(Ft, window_frames, window_stride, window_batch)
        K, Fw, groups = wplan.K, wplan.window_frames, wplan.K // G
        for name, t, want in (("image_latents", image_latents, (2,)), ("image_embeddings", image_embeddings, (2,)),
                              ("controlnet_condition", controlnet_condition, (2, Ft)), ("camera_cond", camera_cond, (2, Ft))):
            if t is not None and tuple(t.shape[:len(want)]) != want:
                raise ValueError(f"`window_frames` serves one request of {Ft} frames: `{name}` must begin {list(want)} (uncond half first); "
                                 f"got {tuple(t.shape)}")
        plan = control_plan(num_inference_steps, controlnet_cond_scale, control_guidance_start, control_guidance_end)
        control_weight = check_control_weight(control_weight, 1, Ft, h, w)
        weighted = control_weight is not None or is_scale_sequence(controlnet_cond_scale)
        scheduled = weighted or (float(control_guidance_start), float(control_guidance_end)) != (0.0, 1.0)
        if max_guidance_scale <= 1.0:            # as in denoise: the reference's non-CFG branch cannot run
            c = self.unet.config
            raise RuntimeError(f"mat1 and mat2 shapes cannot be multiplied (1x{2 * 3 * c.addition_time_embed_dim} and "
                               f"{c.projection_class_embeddings_input_dim}x{c.block_out_channels[0] * 4})")
        self.scheduler.set_timesteps(num_inference_steps, device=dev)
        self._num_timesteps, self.scheduler._step_index = len(self.scheduler.timesteps), None
        g = torch.linspace(min_guidance_scale, max_guidance_scale, Fw).unsqueeze(0).to(dev, out_dtype)    # window-local: a window is a clip
        self._guidance_scale = _append_dims(g, latents.ndim)
        guidance = g.to(torch.float32).contiguous()
        added_time_ids = _get_add_time_ids(0.02, torch.float32, G, 6, 128, unet=self.unet).repeat(2 * G, 1).to(dev)
        x = latents.to(torch.float32).contiguous().clone()
        il = image_latents.to(dev, torch.float16).contiguous()
        emb = image_embeddings.to(dev, torch.float16).repeat_interleave(G, 0).contiguous()               # halves-major: row half G + i
        cond = controlnet_condition.to(dev, torch.float16)
        cam = None if camera_cond is None else camera_cond.to(dev, torch.float16)
        ptype, sig = PREDICTION_TYPES[self.scheduler.config.prediction_type], self.scheduler._sigmas_host
        kinds = ["plain"] * len(plan) if not scheduled else [("weighted" if weighted else "plain") if on else "off" for on, _ in plan]
        step_scales = [s for _, s in plan]
        staging = W.WindowStaging(wplan, G)
        # per group the slices a G-clip call on its windows would receive, [2G, Fw, ...] halves-major (and [G, Fw, h, w] pooled)
        cut = lambda t, gi: torch.stack([t[:, s:s + Fw] for s in (wplan.starts[k] for k in staging.windows(gi))], 1).flatten(0, 1).contiguous()
        sizes = tap_sizes(h, w, len(self.controlnet.config.block_out_channels))
        inputs = []
        for gi in range(groups):
            level_base = None
            if "weighted" in kinds:
                cw = torch.ones((1, Ft, h, w), dtype=torch.float32, device=dev) if control_weight is None else control_weight.to(dev)
                level_base = pool_control_weight(cut(cw, gi), sizes)
            inputs.append((cut(cond, gi), None if cam is None else cut(cam, gi), level_base))
        independent = G if G > 1 else 0                                     # one window per evaluation: one-clip launches
        run = lambda st, sample, t_: self._networks_step(st.kind, sample, t_, st.emb, st.cond, st.cam, st.ids, controlnet_cond_scale,
                                                         st.wbuf, overlap_streams, None, independent)
        geometry = GraphKey(Bc=G, F=Fw, hw=(h, w), cond_shape=tuple(inputs[0][0].shape), cam_shape=None if cam is None else tuple(inputs[0][1].shape),
                            kind=None, scale=None, unet=id(self.unet), controlnet=id(self.controlnet), unet_gen=self.unet._generation,
                            controlnet_gen=self.controlnet._generation, overlap=bool(overlap_streams), networks_name=None,
                            dispatch=ops.dispatch_key() + (("independent_clips", bool(independent)),)) if use_graph else None
        weights = torch.from_numpy(wplan.weights).to(dev)
        pred_all = torch.empty((2 * K, Fw, h, w, 4), dtype=torch.float32, device=dev) if groups > 1 else None
        merged = torch.empty((1, Ft, 4, h, w), dtype=torch.float32, device=dev)
        multistep = getattr(self.scheduler, "order", 1) == 2
        d_prev = torch.empty_like(x) if multistep else None
        live, loaded = {}, {}
        try:
            for i in range(self._num_timesteps):
                t = self.scheduler._timesteps_host[i]
                if self.scheduler._step_index is None:
                    self.scheduler._init_step_index(t)
                k = self.scheduler._step_index
                kind = kinds[i]
                st = live.get(kind)
                if st is None:                   # the first step of its kind in this call
                    key = geometry and geometry._replace(kind=kind, scale=float(controlnet_cond_scale) if kind == "plain" else None)
                    st = live[kind] = (key and self._step_graphs.get(key)) or StepState(kind, run, key)
                    st.windows = staging
                    st.load(emb, added_time_ids, *inputs[0], self.controlnet)
                    loaded[kind] = 0
                    if use_graph and st.graph is None:
                        staging.select(0)
                        st.capture(self._step_graphs.pool_for(key), x, il, sig[k], t)
                        self._step_graphs.insert(key, st)
                for gi in range(groups):
                    if loaded[kind] != gi:       # several groups share one state (and graph): this group's condition into it
                        st.load(emb, added_time_ids, *inputs[gi], self.controlnet)
                        loaded[kind] = gi
                    st.fold(step_scales[i])
                    staging.select(gi)
                    pred_cl = st.step(x, il, sig[k], t)                                    # [2G, Fw, h, w, 4] fp32
                    if groups > 1:               # halves-major rows of the K-window buffer
                        pred_all[gi * G:(gi + 1) * G].copy_(pred_cl[:G])
                        pred_all[K + gi * G:K + (gi + 1) * G].copy_(pred_cl[G:])
                W.cfg_window_merge(pred_all if groups > 1 else pred_cl, guidance, weights, wplan.starts, Ft, out=merged)
                if multistep:
                    x = ops.multistep_step(merged, x, self.scheduler.coefficients(k, first=i == 0), d_prev)
                else:
                    x = ops.euler_step(merged, x, sig[k], sig[k + 1], ptype)
                self.scheduler._step_index += 1
                self.scheduler.is_scale_input_called = True
                if callback_on_step_end is not None:
                    cb_latents = x.to(out_dtype)
                    outs = callback_on_step_end(self, i, t, {"latents": cb_latents})
                    new = outs.pop("latents", cb_latents)
                    if new is not x:
                        x = new.to(torch.float32).contiguous().clone()
        finally:                                 # a cached state serves the next call, windowed or not
            for st in live.values():
                st.windows = None
        return x.to(out_dtype)

    @torch.no_grad()
    def __call__(self, image=None, controlnet_condition: torch.FloatTensor = None, height: int = 576, width: int = 1024,
                 num_frames: Optional[int] = None, num_inference_steps: int = 25, min_guidance_scale: float = 1.0,
                 max_guidance_scale: float = 3.0, fps: int = 7, motion_bucket_id: int = 127,
                 noise_aug_strength: float = 0.02, decode_chunk_size: Optional[int] = None,
                 num_videos_per_prompt: Optional[int] = 1, generator=None, latents: Optional[torch.FloatTensor] = None,
                 output_type: Optional[str] = "pil", callback_on_step_end: Optional[Callable[[int, int, Dict], None]] = None,
                 callback_on_step_end_tensor_inputs: List[str] = ["latents"], return_dict: bool = True,
                 controlnet_cond_scale=1.0, batch_size=1, camera_cond=None,
                 image_embeddings: Optional[torch.Tensor] = None, image_latents: Optional[torch.Tensor] = None,
                 use_graph: bool = True, overlap_streams: bool = True, control_guidance_start: float = 0.0,
                 control_guidance_end: float = 1.0, control_weight: Optional[torch.Tensor] = None,
                 independent_clips: bool = False, window_frames: Optional[int] = None, window_stride: Optional[int] = None,
                 window_batch: Optional[int] = None):
        """Same signature as the reference (``pipeline...:316-340``; ``camera_cond`` from the ``_cam`` twin) plus
        ``image_embeddings`` ``[2,1,D]`` / ``image_latents`` ``[2,4,h,w]`` (the outputs of the CLIP / VAE-encode stages,
        ``:441,457``, for callers that have them already) and ``use_graph`` / ``overlap_streams`` (the loop as a replayed
        hipGraph with the ControlNet and the U-Net encoder on two streams - the configuration ``bench.py`` measures;
        bit-identical to eager launches, ``tests/test_model_gpu.py``).  ``fps``, ``motion_bucket_id`` and
        ``noise_aug_strength`` do not reach the U-Net in the reference either (Q4).

        Beyond the reference (see ``denoise``): ``control_guidance_start`` / ``control_guidance_end`` (diffusers' control window over
        the steps), ``controlnet_cond_scale`` as one float per step, and ``control_weight`` ``[F, h, w]`` / ``[Bc, F, h, w]`` at latent
        resolution (``h = height // 8``), intended range [0, 1] - a weight per frame and latent pixel on every ControlNet residual;
        per-frame strength ``s [F]`` is ``s[:, None, None].expand(F, h, w)``.  They are checked before any stage runs.

        ``independent_clips=True`` (see ``denoise``; NOT the reference's behaviour, default off): K requests in one call, each computed
        as a clip of its own - what raising a batch size for throughput is expected to mean.  ``image`` is a list of K images;
        ``controlnet_condition`` a list of K map sets or a ``[K, F, 3, H, W]`` tensor; ``generator`` one generator or a list of K (request
        k draws its augmentation noise and its latents from generator k, as a call of its own would); ``camera_cond`` ``[K, F, 12]``;
        ``latents`` ``[K, F, 4, h, w]``, ``image_embeddings`` ``[2K, 1, D]`` and ``image_latents`` ``[2K, 4, h, w]`` (uncond halves first)
        when given; ``control_weight`` keeps its ``[K, F, h, w]`` form.  ``batch_size`` is taken from the list, ``num_videos_per_prompt``
        must be 1.  ``.frames`` is a list of K clips, clip k what a call with request k alone returns (``output_type="latent"``: K tensors
        ``[1, F, 4, h, w]``); every clip is decoded on its own.  A mismatched length is a ``ValueError`` naming the argument, raised
        before any stage runs.  Guidance range, control scale and window are shared by the K clips.

        ``window_frames`` / ``window_stride`` / ``window_batch`` (see ``denoise``; beyond the reference, default off): a long video of
        ``num_frames`` frames from a model trained on ``window_frames``, denoised as overlapping windows whose predictions are blended at
        every step.  One request per call (``batch_size * num_videos_per_prompt == 1``, not with ``independent_clips``);
        ``controlnet_condition`` holds ``num_frames`` maps, ``camera_cond`` is ``[num_frames, 12]``, ``control_weight``
        ``[num_frames, h, w]``; ``decode_chunk_size`` defaults to ``window_frames``.  Every window is conditioned on the same first image."""
        num_frames = num_frames if num_frames is not None else self.unet.config.num_frames
        control_plan(num_inference_steps, controlnet_cond_scale, control_guidance_start, control_guidance_end)
        if window_frames is not None:
            from .windows import resolve
            if independent_clips:
                raise ValueError("`window_frames` serves one request: it does not go with `independent_clips`")
            if batch_size * (num_videos_per_prompt or 1) != 1:
                raise ValueError(f"`window_frames` serves one request: `batch_size` * `num_videos_per_prompt` must be 1; got "
                                 f"{batch_size} * {num_videos_per_prompt}")
            resolve(num_frames, window_frames, window_stride, window_batch)
            decode_chunk_size = decode_chunk_size if decode_chunk_size is not None else int(window_frames)
        elif window_stride is not None or window_batch is not None:
            raise ValueError("`window_stride` / `window_batch` need `window_frames` (the windowed loop is off without it)")
        if independent_clips:
            batch_size = self._check_independent_requests(image, controlnet_condition, generator, camera_cond, latents, image_embeddings,
                                                          image_latents, num_videos_per_prompt, num_frames)
            num_videos_per_prompt = 1                                                       # (None is taken as 1)
            if isinstance(generator, tuple):                                                # randn_tensor / prepare_latents know lists
                generator = list(generator)
        check_control_weight(control_weight, batch_size * num_videos_per_prompt, num_frames, height // self.vae_scale_factor,
                             width // self.vae_scale_factor)
        decode_chunk_size = decode_chunk_size if decode_chunk_size is not None else num_frames                # :422
        self.check_inputs(image, height, width)
        if output_type != "latent" and self.vae is None:
            raise NotImplementedError(f"output_type={output_type!r} needs a `vae` (posetraj_amd.AutoencoderKLTemporalDecoder); "
                                      "construct the pipeline with vae=, or ask for output_type='latent'")
        dev = self.unet.device
        do_cfg = max_guidance_scale > 1.0                                                   # :438
        if independent_clips and image is not None and all(torch.is_tensor(im) for im in image):
            image = torch.stack([im.reshape(im.shape[-3:]) for im in image])                # K tensors [3, H, W] -> the batch tensor
        if image_embeddings is None:                                                        # :441
            if self.image_encoder is None:
                raise NotImplementedError("no `image_encoder` was given to the pipeline: pass `image_embeddings` [2,1,D], or "
                                          "construct the pipeline with image_encoder= (posetraj_amd.CLIPVisionModelWithProjection)")
            image_embeddings = self._encode_image(image, dev, num_videos_per_prompt, do_cfg)
        # :454-463 - an fp16 VAE with force_upcast is run in fp32 around encode(): .to(dtype=torch.float32) switches this package's
        # VAE to its fp32 encoder (csrc/vae_f32.hip), .to(dtype=torch.float16) back
        needs_upcasting = self.vae is not None and getattr(self.vae, "dtype", None) == torch.float16 and \
            bool(getattr(self.vae.config, "force_upcast", False))
        if image_latents is None:                                                           # :449-462
            if self.vae is None:
                raise NotImplementedError("no `vae` was given to the pipeline: pass `image_latents` [2,4,h,w], or construct the "
                                          "pipeline with vae= (posetraj_amd.AutoencoderKLTemporalDecoder)")
            if independent_clips and torch.is_tensor(image):                                # (a tensor's range is judged per request)
                img = torch.cat([self.preprocess_condition(im.unsqueeze(0), height, width) for im in image])
            else:
                img = self.preprocess_condition(image, height, width)                        # image_processor.preprocess -> [-1, 1]
            noise = randn_tensor(img.shape, generator=generator, device=img.device, dtype=img.dtype)
            img = img + noise_aug_strength * noise
            if needs_upcasting:
                self.vae.to(dtype=torch.float32)
            else:
                img = img.to(getattr(self.vae, "dtype", None) or img.dtype)
            try:
                image_latents = self._encode_vae_image(img, dev, num_videos_per_prompt, do_cfg).to(image_embeddings.dtype)
            finally:                                                                         # (an encode that throws leaves the VAE as it was)
                if needs_upcasting:
                    self.vae.to(dtype=torch.float16)
        self.scheduler.set_timesteps(num_inference_steps, device=dev)                       # :482, before init_noise_sigma is read (:298)
        lat = self.prepare_latents(batch_size * num_videos_per_prompt, num_frames, self.unet.config.in_channels, height,
                                   width, image_embeddings.dtype, dev, generator, latents)
        if independent_clips:                                                               # K map sets, each prepared as a call of its own would
            cond = torch.stack([self.preprocess_condition(c, height, width) for c in controlnet_condition])
        else:
            cond = self.preprocess_condition(controlnet_condition, height, width).unsqueeze(0)   # :500
        cond = torch.cat([cond] * 2)                                                        # :501-503 (Q5)
        cam = None
        if camera_cond is not None:
            cam = torch.as_tensor(camera_cond, dtype=torch.float32)
            cam = torch.cat([cam if independent_clips else cam.unsqueeze(0)] * 2)
        latents = self.denoise(lat, image_latents, image_embeddings, cond, num_inference_steps, min_guidance_scale,
                               max_guidance_scale, controlnet_cond_scale, cam, callback_on_step_end,
                               callback_on_step_end_tensor_inputs, use_graph=use_graph, overlap_streams=overlap_streams,
                               control_guidance_start=control_guidance_start, control_guidance_end=control_guidance_end,
                               control_weight=control_weight, independent_clips=independent_clips,
                               **({} if window_frames is None else dict(window_frames=window_frames, window_stride=window_stride, window_batch=window_batch)))
        if not output_type == "latent":                                                     # :585-592
            if needs_upcasting:
                self.vae.to(dtype=torch.float16)
            if independent_clips:                        # clip by clip: a decode chunk never spans two requests
                frames = torch.cat([self.decode_latents(latents[k:k + 1], num_frames, decode_chunk_size) for k in range(latents.shape[0])])
            else:
                frames = self.decode_latents(latents, num_frames, decode_chunk_size)
            frames = tensor2vid(frames, self.image_processor, output_type=output_type)
        else:
            frames = [latents[k:k + 1] for k in range(latents.shape[0])] if independent_clips else latents
        self.maybe_free_model_hooks()
        if not return_dict:
            return frames
        return StableVideoDiffusionPipelineOutput(frames=frames)


# BASELINE.json names the class this way; the reference's name is the one above (pipeline...:99)
StableVideoDiffusionControlNetPipeline = StableVideoDiffusionPipelineControlNet
