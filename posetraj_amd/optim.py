"""The optimizer of ``ControlNetTrainer``: AdamW over a ``ParamStore``, with fp32 moments (``AdamW``; ``optimizer_cls =
torch.optim.AdamW``, ``scripts/train_svd_traj_VIPSeg_14.py:1051``) or block-quantised ones (``AdamW8bit``; ``--use_8bit_adam``,
``bnb.optim.AdamW8bit``, ``:1041-1049``).  Either object owns its state buffers, the ONE launch of a step and the optimizer's part of a
checkpoint:

    kind                         "adamw" / "adamw8bit": the strings of ``trainer_state.json``
    step(lr, step, inv_scale, ema_shadow=None, one_minus_decay=0.0)
                                 parameters, fp16 mirror, zeroed gradient and (with ``ema_shadow``) the EMA in one launch on the current
                                 stream; betas, eps and weight decay are the object's
    state_dict() / load_state_dict(sd)      the tensors of ``optimizer.safetensors`` (host); the loader is strict in names and shapes
    checkpoint_meta() / check_checkpoint_meta(state, where)      the keys the kind adds to ``trainer_state.json``, and the refusal of a
                                 checkpoint of the other kind
    state_bytes                  device bytes of the state

``params`` is a ``ParamStore``, or anything with its ``names``, ``shapes``, ``offsets``, ``numel``, ``flat``, ``grad``, ``flat16`` and
``export`` / ``load`` / ``shaped``.  Construction launches nothing: both build over a CPU-resident store.  The GradScaler's rules, the
schedule and the EMA's counters stay with the trainer (``ControlNetTrainer.optimizer_step``).

bitsandbytes is not available where this was written: the 8-bit format below is its published blockwise dynamic quantisation
RESTATED (PARITY UNPINNED) - and bit parity is out of reach anyway: the ``ParamStore`` keeps convolution weights
tap-major, so a block of 256 stored elements holds other elements than a block over torch's layout.  Host planning here is pure
Python; the update is ``pto_adamw8_f32``.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import hip, ops

ADAM8_BLOCK = 256                # elements per absmax
ADAM8_MIN_SIZE = 4096            # bnb's min_8bit_size: a parameter with fewer elements keeps fp32 moments
ADAM8_KINDS = ("adamw", "adamw8bit")


class AdamW:
    """AdamW with two flat fp32 moment buffers in the store's layout (tap-major convolution weights: AdamW is element-wise and does
    not care).  ``step`` is ``pt_adamw_fused_f32``, or ``pt_adamw_ema_f32`` with a shadow; ``lr`` is the base rate, ``step`` takes the
    scheduled rate of its step."""
    kind = "adamw"

    def __init__(self, params, *, lr, betas, eps, weight_decay):
        self.params = params
        self.lr, self.betas, self.eps, self.weight_decay = lr, tuple(betas), eps, weight_decay
        self._allocate(params.flat.device)

    def _allocate(self, dev) -> None:
        n = self.params.numel
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=dev)

    @property
    def state_bytes(self) -> int:
        return 8 * self.params.numel

    def step(self, lr, step, inv_scale, ema_shadow=None, one_minus_decay=0.0) -> None:
        """AdamW + the fp16 mirror of the new parameters + the gradient's zeroing (+ the EMA of the new parameters) in ONE pass."""
        P = self.params
        adamw = (P.flat.data_ptr(), P.grad.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), P.numel, lr, self.betas[0],
                 self.betas[1], self.eps, self.weight_decay, step, inv_scale, P.flat16.data_ptr(), 1)
        if ema_shadow is None:
            hip.checked().pt_adamw_fused_f32(*adamw, ops._stream())
        else:
            hip.checked().pt_adamw_ema_f32(*adamw, ema_shadow.data_ptr(), one_minus_decay, ops._stream())

    def state_dict(self) -> dict:
        """``optimizer.safetensors`` of an fp32 checkpoint: ``exp_avg.<name>`` / ``exp_avg_sq.<name>``, torch's shape and order."""
        out = {}
        for key, buf in (("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq)):
            for k, v in self.params.export(buf).items():
                out[f"{key}.{k}"] = v.cpu()
        return out

    def load_state_dict(self, sd: dict) -> None:
        """Strict in names and shapes (``ParamStore.load``)."""
        for key, buf in (("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq)):
            self.params.load(buf, {k[len(key) + 1:]: v for k, v in sd.items() if k.startswith(key + ".")})

    def checkpoint_meta(self) -> dict:
        return {}                                     # (a checkpoint of the fp32 optimizer has neither key)

    def check_checkpoint_meta(self, state: dict, where: str) -> None:
        have = state.get("optimizer", "adamw")
        if have != self.kind:
            raise ValueError(f"{where}: the checkpoint holds the state of optimizer {have!r} but the trainer runs {self.kind!r} "
                             f"(use_8bit_adam={self.kind == 'adamw8bit'}); states of 'adamw' and 'adamw8bit' are not converted into each other")


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


class AdamW8bit(AdamW):
    """AdamW with block-quantised moments: uint8 codes and per-block absmax for the large parameters, compact fp32 moments
    (``exp_avg`` / ``exp_avg_sq`` hold the small parameters' only), the two books and the segment table, all on the store's device.  A
    fresh state is zero: every code the code of 0.0, every absmax 0.  ``step`` is ``pto_adamw8_f32``."""
    kind = "adamw8bit"

    def _allocate(self, dev) -> None:
        params = self.params
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

    @property
    def state_bytes(self) -> int:
        return self.plan["state_bytes"]

    @staticmethod
    def _ptr(t):
        return t.data_ptr() if t.numel() else None

    def step(self, lr, step, inv_scale, ema_shadow=None, one_minus_decay=0.0) -> None:
        """``pto_adamw8_f32`` over the store: parameters, fp16 mirror, zeroed gradient and (with ``ema_shadow``) the EMA in one launch."""
        P, plan = self.params, self.plan
        hip.checked().pto_adamw8_f32(P.flat.data_ptr(), P.grad.data_ptr(), self._ptr(self.state1), self._ptr(self.state2), self._ptr(self.absmax1),
                                    self._ptr(self.absmax2), self.qmap1.data_ptr(), self.qmap2.data_ptr(), self._ptr(self.exp_avg),
                                    self._ptr(self.exp_avg_sq), self._segments, len(plan["segments"]), plan["n_work"], P.numel, plan["n_blocks"],
                                    plan["n_f32_alloc"], lr, self.betas[0], self.betas[1], self.eps, self.weight_decay, step, inv_scale,
                                    P.flat16.data_ptr(), 1, None if ema_shadow is None else ema_shadow.data_ptr(), one_minus_decay, ops._stream())

    def dequantize(self):
        """``(exp_avg, exp_avg_sq)`` as flat fp32 buffers in the store's layout (``pto_adam8_dequant_f32``): what the next step reads."""
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
            raise KeyError(f"AdamW8bit.load_state_dict: missing {missing[:4]}{'...' if len(missing) > 4 else ''}, unexpected {extra[:4]}{'...' if len(extra) > 4 else ''}")
        for key, book in (("qmap1", self.qmap1), ("qmap2", self.qmap2)):
            if not torch.equal(sd[key].to(torch.float32).cpu(), book.cpu()):
                raise ValueError(f"AdamW8bit.load_state_dict: {key} differs from this build's code book")
        P = self.params
        for name, start, count, state, kind, _ in self.plan["segments"]:
            views = self._slices(name)
            keys = ("state1", "state2", "absmax1", "absmax2") if kind else ("exp_avg", "exp_avg_sq")
            for key, dst in zip(keys, views):
                src = sd[f"{key}.{name}"]
                if kind:
                    if src.dtype != dst.dtype or src.numel() != dst.numel():
                        raise ValueError(f"AdamW8bit.load_state_dict: {key}.{name} is {src.dtype} x {src.numel()}, expected {dst.dtype} x {dst.numel()}")
                    dst.copy_(src.reshape(-1).to(dst.device))
                else:
                    if tuple(src.shape) != P.shapes[name]:
                        raise ValueError(f"AdamW8bit.load_state_dict: {key}.{name} has shape {tuple(src.shape)}, expected {P.shapes[name]}")
                    P.shaped(dst, name).copy_(src.to(device=dst.device, dtype=torch.float32))

    def state_dict_keys(self):
        keys = ["qmap1", "qmap2"]
        for name, _, _, _, kind, _ in self.plan["segments"]:
            keys += [f"{k}.{name}" for k in (("state1", "state2", "absmax1", "absmax2") if kind else ("exp_avg", "exp_avg_sq"))]
        return keys

    def checkpoint_meta(self) -> dict:
        return {"optimizer": self.kind, "optimizer_block_size": self.plan["block"]}

    def check_checkpoint_meta(self, state: dict, where: str) -> None:
        super().check_checkpoint_meta(state, where)
        if state.get("optimizer_block_size") != self.plan["block"]:
            raise ValueError(f"{where}: 8-bit optimizer state in blocks of {state.get('optimizer_block_size')!r}, this build uses {self.plan['block']}")
