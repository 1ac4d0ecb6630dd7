"""``--use_ema``: an exponential moving average of the ControlNet's parameters (the reference imports ``EMAModel`` from
``diffusers.training_utils``; ``scripts/train_svd_traj_VIPSeg_14.py:970-974`` builds it, ``:1428-1430`` steps it, ``:1477-1480`` /
``:1540-1542`` / ``:1558-1559`` swap it in for validation and for the final ``save_pretrained``, ``:992-1006`` save and load it).

The semantics are diffusers 0.24.0's ``training_utils.EMAModel``, RESTATED FROM MEMORY (the package is not available where this was
written; like the other diffusers leaves of this project it is pinned by tests against a torch restatement, not against the
package itself):

    get_decay(k):   step = max(0, k - update_after_step - 1);  0.0 if step <= 0;
                    d = 1 - (1 + step / inv_gamma) ** -power   with use_ema_warmup, else (1 + step) / (10 + step);
                    max(min(d, decay), min_decay)              - Python doubles
    step():         optimization_step += 1;  decay = cur_decay_value = get_decay(optimization_step);
                    shadow.sub_((1 - decay) * (shadow - param))  for every parameter, fp32: three rounded operations

The reference's own wiring of the option is inconsistent (the ``EMAModel`` is built over the U-Net's parameters, stepped with the
ControlNet's, saved to ``controlnet_ema/`` and loaded from ``unet_ema/``); what the option MEANS is built here: the average of the
ControlNet's parameters, saved to and loaded from ``controlnet_ema/``.

Storage: ONE flat fp32 buffer in the ``ParamStore``'s layout (tap-major convolution weights), allocated only when EMA is on.  The
update is a HIP kernel - ``pt_adamw_ema_f32`` inside the optimizer's pass (``ControlNetTrainer.optimizer_step``), or
``pt_ema_update_f32`` on its own (``step()``, and the steps the GradScaler skipped); buffer copies (``copy_to`` / ``store`` /
``restore``) are torch copies.
"""
from __future__ import annotations

import json
import os
from typing import Dict, Optional

import torch

from .modeling import EMA_CONFIG_KEYS


class EMAModel:
    """``EMAModel(trainer.params, decay=..., model_config=trainer.config)``: the shadow is a clone of the parameters at construction."""

    def __init__(self, params, decay: float = 0.9999, min_decay: float = 0.0, update_after_step: int = 0, use_ema_warmup: bool = False,
                 inv_gamma: float = 1.0, power: float = 2 / 3, model_config: Optional[dict] = None):
        self.params = params
        self.shadow = params.flat.clone()
        self.temp_stored = None
        self.decay, self.min_decay, self.update_after_step = decay, min_decay, update_after_step
        self.use_ema_warmup, self.inv_gamma, self.power = use_ema_warmup, inv_gamma, power
        self.optimization_step = 0
        self.cur_decay_value = None
        self.model_config = dict(model_config) if model_config is not None else {}

    # -- the schedule
    def get_decay(self, optimization_step: int) -> float:
        step = max(0, optimization_step - self.update_after_step - 1)
        if step <= 0:
            return 0.0
        if self.use_ema_warmup:
            cur = 1 - (1 + step / self.inv_gamma) ** -self.power
        else:
            cur = (1 + step) / (10 + step)
        return max(min(cur, self.decay), self.min_decay)

    def begin_step(self) -> float:
        """The host half of ``step()``: advance the counter, fix this step's decay; returns ``1 - decay`` (a double: the launch rounds it
        to fp32 once).  ``ControlNetTrainer.optimizer_step`` calls this and hands the value to the fused AdamW launch."""
        self.optimization_step += 1
        self.cur_decay_value = self.get_decay(self.optimization_step)
        return 1.0 - self.cur_decay_value

    def update(self, one_minus_decay: float) -> None:
        """The device half on its own: ``shadow -= one_minus_decay * (shadow - params)`` over the flat buffers, current stream."""
        from . import hip, ops
        hip.checked().pt_ema_update_f32(self.shadow.data_ptr(), self.params.flat.data_ptr(), self.params.numel, one_minus_decay,
                                        ops._stream())

    def step(self) -> None:
        """``ema.step(controlnet.parameters())`` as a launch of its own.  (A ``ControlNetTrainer(use_ema=True)`` steps its EMA inside
        ``optimizer_step``: the loop does not call this as well.)"""
        self.update(self.begin_step())

    # -- the averaged weights
    def shadow_state_dict(self) -> Dict[str, torch.Tensor]:
        """The averaged parameters by name, fp32, torch's shapes and memory order."""
        return self.params.export(self.shadow)

    def _moved(self) -> None:
        self.params.version += 1                      # the fp16 mirror and every layer's fp16 packs follow the new master values

    def copy_to(self) -> None:
        """``ema.copy_to(controlnet.parameters())``: the averaged weights become the master parameters."""
        self.params.flat.copy_(self.shadow)
        self._moved()

    def store(self) -> None:
        """``ema.store(controlnet.parameters())``: park the master parameters (before ``copy_to`` for a validation run)."""
        self.temp_stored = self.params.flat.clone()

    def restore(self) -> None:
        """``ema.restore(controlnet.parameters())``: bring the parked parameters back; the parked copy is released."""
        if self.temp_stored is None:
            raise RuntimeError("This ExponentialMovingAverage has no `store()`ed weights to `restore()`")
        self.params.flat.copy_(self.temp_stored)
        self.temp_stored = None
        self._moved()

    # -- state
    def scalars(self) -> dict:
        return {"decay": self.decay, "min_decay": self.min_decay, "optimization_step": self.optimization_step,
                "update_after_step": self.update_after_step, "use_ema_warmup": self.use_ema_warmup, "inv_gamma": self.inv_gamma,
                "power": self.power}

    def state_dict(self) -> dict:
        return dict(self.scalars(), shadow_params=self.shadow_state_dict())

    def load_state_dict(self, state_dict: dict) -> None:
        sd = dict(state_dict)
        self.decay = sd.get("decay", self.decay)
        if self.decay < 0.0 or self.decay > 1.0:
            raise ValueError("Decay must be between 0 and 1")
        self.min_decay = sd.get("min_decay", self.min_decay)
        if not isinstance(self.min_decay, float):
            raise ValueError("Invalid min_decay")
        self.optimization_step = sd.get("optimization_step", self.optimization_step)
        if not isinstance(self.optimization_step, int):
            raise ValueError("Invalid optimization_step")
        self.update_after_step = sd.get("update_after_step", self.update_after_step)
        if not isinstance(self.update_after_step, int):
            raise ValueError("Invalid update_after_step")
        self.use_ema_warmup = sd.get("use_ema_warmup", self.use_ema_warmup)
        if not isinstance(self.use_ema_warmup, bool):
            raise ValueError("Invalid use_ema_warmup")
        self.inv_gamma = sd.get("inv_gamma", self.inv_gamma)
        if not isinstance(self.inv_gamma, (float, int)):
            raise ValueError("Invalid inv_gamma")
        self.power = sd.get("power", self.power)
        if not isinstance(self.power, (float, int)):
            raise ValueError("Invalid power")
        shadow = sd.get("shadow_params")
        if shadow is not None:
            self.params.load(self.shadow, shadow)     # strict in names and shapes, like the parameters' own loader

    def save_pretrained(self, path: str) -> None:
        """diffusers' layout of an EMA folder: the model's ``config.json`` with the seven EMA scalars added, and the averaged weights as
        ``diffusion_pytorch_model.safetensors`` - ``ControlNetSDVModel.from_pretrained(ckpt, subfolder="controlnet_ema")`` reads it."""
        from . import train_state
        train_state.save_model(self.model_config, self.shadow_state_dict(), path, extra=self.scalars())

    @classmethod
    def from_pretrained(cls, path: str, trainer) -> "EMAModel":
        """An ``EMAModel`` over ``trainer.params`` with the scalars and the shadow of the folder ``save_pretrained`` wrote."""
        from safetensors.torch import load_file
        with open(os.path.join(path, "config.json")) as f:
            cfg = json.load(f)
        ema = cls(trainer.params, model_config={k: v for k, v in cfg.items() if k not in EMA_CONFIG_KEYS and not k.startswith("_")})
        ema.load_state_dict(dict({k: cfg[k] for k in EMA_CONFIG_KEYS if k in cfg},
                                 shadow_params=load_file(os.path.join(path, "diffusion_pytorch_model.safetensors"))))
        return ema
