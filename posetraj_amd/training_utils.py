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


# ------------------------------------------------------------------------------------------------- --use_8bit_adam
# Blockwise 8-bit AdamW (``optimizer_cls = bnb.optim.AdamW8bit``, ``scripts/train_svd_traj_VIPSeg_14.py:1041-1049``).  bitsandbytes is
# not available where this was written: the format below is its published blockwise dynamic quantisation RESTATED (DESIGN 4.13,
# PARITY UNPINNED) - and bit parity is out of reach anyway: the ``ParamStore`` keeps convolution weights tap-major, so a block of 256
# stored elements holds other elements than a block over torch's layout.  Host planning here is pure Python; the update is
# ``pto_adamw8_f32``.
ADAM8_BLOCK = 256                # elements per absmax
ADAM8_MIN_SIZE = 4096            # bnb's min_8bit_size: a parameter with fewer elements keeps fp32 moments
ADAM8_KINDS = ("adamw", "adamw8bit")


def create_dynamic_map(signed: bool = True, max_exponent_bits: int = 7, total_bits: int = 8) -> torch.Tensor:
    """bnb's dynamic code book: 2^total_bits sorted fp32 values in [-1, 1] (signed) or [0, 1].  Decade ``i`` of
    ``max_exponent_bits`` holds the midpoints of ``linspace(0.1, 1, k_i + 1)`` (fp64) times ``10^(i - max_exponent_bits + 1)`` with
    ``k_i = 2^i`` (signed: each value also negated) or ``2^(i + 1)``; 0 and 1.0 complete the book."""
    non_sign_bits = total_bits - (1 if signed else 0)
    data = []
    for i in range(max_exponent_bits):
        k = 2 ** (i + non_sign_bits - max_exponent_bits)
        b = torch.linspace(0.1, 1, k + 1, dtype=torch.float64)
        means = ((b[:-1] + b[1:]) / 2.0 * 10.0 ** (i - max_exponent_bits + 1)).tolist()
        data += means
        if signed:
            data += [-v for v in means]
    data += [0.0, 1.0]
    if len(data) != 2 ** total_bits:
        raise ValueError(f"create_dynamic_map: {len(data)} values for {total_bits} bits")
    return torch.tensor(sorted(data), dtype=torch.float64).to(torch.float32)


def plan_8bit_state(names, shapes, offsets) -> dict:
    """Where every parameter's optimizer state lives (no device).  ``names``: the store's order; ``shapes`` / ``offsets``: name ->
    shape / first element in the flat buffers.  Returns

        segments      one ``(name, start, count, state, kind, work)`` per parameter, the fields of ``pt_adam8_segment``: kind 1
                      (8-bit, ``count >= ADAM8_MIN_SIZE``) - ``state`` is its first block of 256 stored elements (blocks start at the
                      parameter and never cross into the next; the last may be short; block b's codes lie at ``256 b``); kind 0
                      (fp32) - ``state`` is its offset in the compact fp32 moment buffers (rounded up to 8 per parameter)
        n_blocks, n_work          blocks of the 8-bit parameters; units of 256 elements over all parameters (what the launch walks)
        n_8bit, n_f32             elements with 8-bit / fp32 moments;  ``n_f32_alloc``: floats in each compact buffer
        state_bytes               device bytes of the whole state: codes, absmax, fp32 moments, the two books and the table"""
    segments, n_blocks, n_work, n_8bit, n_f32, n_f32_alloc = [], 0, 0, 0, 0, 0
    end = 0
    for k in names:
        count = 1
        for s in shapes[k]:
            count *= int(s)
        start = int(offsets[k])
        if start % 8 or start < end or count < 1:
            raise ValueError(f"plan_8bit_state: {k} starts at {start} (a multiple of 8 behind the parameter in front of it) with {count} elements")
        end = start + count
        units = -(-count // ADAM8_BLOCK)
        if count >= ADAM8_MIN_SIZE:
            segments.append((k, start, count, n_blocks, 1, n_work))
            n_blocks, n_8bit = n_blocks + units, n_8bit + count
        else:
            segments.append((k, start, count, n_f32_alloc, 0, n_work))
            n_f32, n_f32_alloc = n_f32 + count, n_f32_alloc + (count + 7) // 8 * 8
        n_work += units
    state_bytes = 2 * ADAM8_BLOCK * n_blocks + 2 * 4 * n_blocks + 2 * 4 * n_f32_alloc + 2 * 4 * 256 + 32 * len(segments)
    return dict(segments=segments, n_blocks=n_blocks, n_work=n_work, n_8bit=n_8bit, n_f32=n_f32, n_f32_alloc=n_f32_alloc,
                block=ADAM8_BLOCK, state_bytes=state_bytes)


class Adam8bitState:
    """The optimizer state of ``ControlNetTrainer(use_8bit_adam=True)`` over a ``ParamStore``: uint8 codes and per-block absmax for the
    large parameters, compact fp32 moments for the small ones, the two books and the segment table, all on the store's device.  A
    fresh state is zero: every code the code of 0.0, every absmax 0."""

    def __init__(self, params):
        from . import hip
        import ctypes as C
        dev = params.flat.device
        self.params = params
        self.plan = plan = plan_8bit_state(params.names, params.shapes, params.offsets)
        self.qmap1, self.qmap2 = create_dynamic_map(True).to(dev), create_dynamic_map(False).to(dev)
        self.zero_codes = (int((self.qmap1 == 0).nonzero()[0, 0]), int((self.qmap2 == 0).nonzero()[0, 0]))
        nb, nf = plan["n_blocks"], plan["n_f32_alloc"]
        self.state1 = torch.full((nb * ADAM8_BLOCK,), self.zero_codes[0], dtype=torch.uint8, device=dev)
        self.state2 = torch.full((nb * ADAM8_BLOCK,), self.zero_codes[1], dtype=torch.uint8, device=dev)
        self.absmax1 = torch.zeros(nb, dtype=torch.float32, device=dev)
        self.absmax2 = torch.zeros(nb, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros(nf, dtype=torch.float32, device=dev)           # the small parameters' moments only
        self.exp_avg_sq = torch.zeros(nf, dtype=torch.float32, device=dev)
        table = (hip.Adam8Segment * len(plan["segments"]))(*[hip.Adam8Segment(*seg[1:]) for seg in plan["segments"]])
        self.table = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
        self._segments = C.cast(self.table.data_ptr(), C.POINTER(hip.Adam8Segment))
        self._by_name = {seg[0]: seg for seg in plan["segments"]}

    @staticmethod
    def _ptr(t):
        return t.data_ptr() if t.numel() else None

    def step(self, lr, beta1, beta2, eps, weight_decay, step, inv_scale, ema_shadow=None, one_minus_decay=0.0) -> None:
        """``pto_adamw8_f32`` over the store: parameters, fp16 mirror, zeroed gradient and (with ``ema_shadow``) the EMA in one launch."""
        from . import hip, ops
        P, plan = self.params, self.plan
        hip.checked().pto_adamw8_f32(P.flat.data_ptr(), P.grad.data_ptr(), self._ptr(self.state1), self._ptr(self.state2), self._ptr(self.absmax1),
                                    self._ptr(self.absmax2), self.qmap1.data_ptr(), self.qmap2.data_ptr(), self._ptr(self.exp_avg),
                                    self._ptr(self.exp_avg_sq), self._segments, len(plan["segments"]), plan["n_work"], P.numel, plan["n_blocks"],
                                    plan["n_f32_alloc"], lr, beta1, beta2, eps, weight_decay, step, inv_scale, P.flat16.data_ptr(), 1,
                                    None if ema_shadow is None else ema_shadow.data_ptr(), one_minus_decay, ops._stream())

    def dequantize(self):
        """``(exp_avg, exp_avg_sq)`` as flat fp32 buffers in the store's layout (``pto_adam8_dequant_f32``): what the next step reads."""
        from . import hip, ops
        P, plan = self.params, self.plan
        m, v = torch.zeros_like(P.flat), torch.zeros_like(P.flat)
        hip.checked().pto_adam8_dequant_f32(self._ptr(self.state1), self._ptr(self.state2), self._ptr(self.absmax1), self._ptr(self.absmax2),
                                           self.qmap1.data_ptr(), self.qmap2.data_ptr(), self._ptr(self.exp_avg), self._ptr(self.exp_avg_sq),
                                           self._segments, len(plan["segments"]), plan["n_work"], P.numel, plan["n_blocks"], plan["n_f32_alloc"],
                                           m.data_ptr(), v.data_ptr(), ops._stream())
        return m, v

    def _slices(self, name):
        """The views of one parameter's state: ``(state1, state2, absmax1, absmax2)`` (kind 1) or ``(exp_avg, exp_avg_sq)`` (kind 0)."""
        _, _, count, state, kind, _ = self._by_name[name]
        if kind:
            nb = -(-count // ADAM8_BLOCK)
            c = slice(state * ADAM8_BLOCK, state * ADAM8_BLOCK + count)
            return self.state1[c], self.state2[c], self.absmax1[state:state + nb], self.absmax2[state:state + nb]
        return self.exp_avg[state:state + count], self.exp_avg_sq[state:state + count]

    def state_dict(self) -> dict:
        """``optimizer.safetensors`` of an 8-bit checkpoint: ``state1.<name>`` / ``state2.<name>`` (uint8, STORED order: tap-major for
        convolution weights, 1-D) and ``absmax1.<name>`` / ``absmax2.<name>`` for the 8-bit parameters, ``exp_avg.<name>`` /
        ``exp_avg_sq.<name>`` (torch's shape and order) for the fp32 ones, ``qmap1`` / ``qmap2``."""
        P, out = self.params, {"qmap1": self.qmap1.cpu(), "qmap2": self.qmap2.cpu()}
        for name, start, count, state, kind, _ in self.plan["segments"]:
            views = self._slices(name)
            if kind:
                for key, t in zip(("state1", "state2", "absmax1", "absmax2"), views):
                    out[f"{key}.{name}"] = t.cpu().clone()
            else:
                for key, t in zip(("exp_avg", "exp_avg_sq"), views):
                    out[f"{key}.{name}"] = P.shaped(t, name).contiguous().cpu().clone()
        return out

    def load_state_dict(self, sd: dict) -> None:
        """Strict in names, shapes and books (a checkpoint quantised with other books would decode to other moments)."""
        want = set(self.state_dict_keys())
        missing, extra = sorted(want - set(sd)), sorted(set(sd) - want)
        if missing or extra:
            raise KeyError(f"Adam8bitState.load_state_dict: missing {missing[:4]}{'...' if len(missing) > 4 else ''}, unexpected {extra[:4]}{'...' if len(extra) > 4 else ''}")
        for key, book in (("qmap1", self.qmap1), ("qmap2", self.qmap2)):
            if not torch.equal(sd[key].to(torch.float32).cpu(), book.cpu()):
                raise ValueError(f"Adam8bitState.load_state_dict: {key} differs from this build's code book")
        P = self.params
        for name, start, count, state, kind, _ in self.plan["segments"]:
            views = self._slices(name)
            keys = ("state1", "state2", "absmax1", "absmax2") if kind else ("exp_avg", "exp_avg_sq")
            for key, dst in zip(keys, views):
                src = sd[f"{key}.{name}"]
                if kind:
                    if src.dtype != dst.dtype or src.numel() != dst.numel():
                        raise ValueError(f"Adam8bitState.load_state_dict: {key}.{name} is {src.dtype} x {src.numel()}, expected {dst.dtype} x {dst.numel()}")
                    dst.copy_(src.reshape(-1).to(dst.device))
                else:
                    if tuple(src.shape) != P.shapes[name]:
                        raise ValueError(f"Adam8bitState.load_state_dict: {key}.{name} has shape {tuple(src.shape)}, expected {P.shapes[name]}")
                    P.shaped(dst, name).copy_(src.to(device=dst.device, dtype=torch.float32))

    def state_dict_keys(self):
        keys = ["qmap1", "qmap2"]
        for name, _, _, _, kind, _ in self.plan["segments"]:
            keys += [f"{k}.{name}" for k in (("state1", "state2", "absmax1", "absmax2") if kind else ("exp_avg", "exp_avg_sq"))]
        return keys
