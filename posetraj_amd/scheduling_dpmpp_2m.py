"""``DPMPP2MDiscreteScheduler`` - DPM-Solver++(2M), the second-order multistep solver of k-diffusion's ``sample_dpmpp_2m``, on the
sigma tables of this package's ``EulerDiscreteScheduler``.  Beyond the reference project, which ships the Euler sampler only.

One network evaluation per step like Euler; the solver keeps one more sample-sized fp32 tensor, the previous denoised estimate.  With
``sigma`` the current and ``sigma'`` the next noise level, ``D`` the denoised estimate and ``h = ln(sigma / sigma')``::

    x' = (sigma'/sigma) x - expm1(-h) ((1 + 1/(2r)) D - (1/(2r)) D_prev),      r = ln(sigma_prev / sigma) / h

which is ``x' = a x + b D + c D_prev``.  ``coefficients`` computes ``(c_skip, c_out, a, b, c)`` on the host in fp64; the device
pass (``pts_multistep_step`` / ``pts_cfg_multistep_step``, include/posetraj_sampler.h) only multiplies and adds.  The first step
of a run has no previous estimate and is exactly the Euler step; a step to ``sigma' = 0`` returns ``D``.  There is no
``lower_order_final``, no SDE variant and no thresholding - this is not diffusers' ``DPMSolverMultistepScheduler`` and takes none
of its options.

    pipe.scheduler = DPMPP2MDiscreteScheduler.from_config(pipe.scheduler.config)
"""
from __future__ import annotations

import inspect
import math
from typing import Optional, Tuple, Union

import torch

from . import ops
from .scheduling_euler_discrete_karras_fix import PREDICTION_TYPES, EulerDiscreteScheduler, EulerDiscreteSchedulerOutput


class DPMPP2MDiscreteScheduler(EulerDiscreteScheduler):
    order = 2

    @classmethod
    def from_config(cls, config) -> "DPMPP2MDiscreteScheduler":
        """From the ``config`` of an ``EulerDiscreteScheduler`` (or of this class): the constructor arguments are the same.  Keys
        the constructor does not know are ignored, like diffusers' ``from_config``."""
        known = [p for p in inspect.signature(EulerDiscreteScheduler.__init__).parameters if p != "self"]
        return cls(**{k: config[k] for k in known if k in config})

    # ------------------------------------------------------------------ tables (host)
    def _install(self, sigmas, timesteps, device):
        super()._install(sigmas, timesteps, device)
        self._denoised_prev = None           # fp32, the sample's shape: D of this run's previous step() (None: no step yet); set_timesteps starts a new run

    def _init_step_index(self, timestep):
        super()._init_step_index(timestep)
        self._denoised_prev = None           # `_step_index is None`: a new run over the same table

    def coefficients(self, i: int, first: Optional[bool] = None) -> Tuple[float, float, float, float, float]:
        """``(c_skip, c_out, a, b, c)`` of step ``i`` (from ``_sigmas_host[i]`` to ``_sigmas_host[i + 1]``), pure host fp64:
        ``D = mo c_out + x c_skip`` and ``x' = a x + b D + c D_prev``.  ``first``: the step has no previous estimate (``c = 0``,
        the Euler step); by default step 0 of the table."""
        sig = self._sigmas_host
        if not 0 <= i < len(sig) - 1:
            raise IndexError(f"step {i} is outside the {len(sig) - 1}-step sigma table")
        s, s_next = float(sig[i]), float(sig[i + 1])
        ptype = self.config.prediction_type
        if ptype not in PREDICTION_TYPES:
            raise ValueError(f"prediction_type given as {ptype} must be one of `epsilon`, or `v_prediction`")
        if PREDICTION_TYPES[ptype] == 0:
            c_skip, c_out = 1.0 / (s * s + 1.0), -s / math.sqrt(s * s + 1.0)
        elif PREDICTION_TYPES[ptype] == 1:
            c_skip, c_out = 1.0, -s
        else:
            c_skip, c_out = 0.0, 1.0
        if s_next == 0.0:
            return c_skip, c_out, 0.0, 1.0, 0.0
        h = math.log(s / s_next)
        a, e = s_next / s, -math.expm1(-h)
        if (i == 0) if first is None else first:
            return c_skip, c_out, a, e, 0.0
        r = math.log(float(sig[i - 1]) / s) / h
        return c_skip, c_out, a, e * (1.0 + 1.0 / (2.0 * r)), -e / (2.0 * r)

    # ------------------------------------------------------------------ per-step tensor maths (device)
    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor,
             return_dict: bool = True) -> Union[EulerDiscreteSchedulerOutput, Tuple]:
        """One DPM-Solver++(2M) step.  The scheduler owns the fp32 history tensor of the run; it starts empty after
        ``set_timesteps`` and whenever ``_step_index`` is None.  The solver is deterministic: no churn arguments."""
        if isinstance(timestep, int) or isinstance(timestep, (torch.IntTensor, torch.LongTensor)) or \
                (isinstance(timestep, torch.Tensor) and timestep.dtype in (torch.int32, torch.int64)):
            raise ValueError("Passing integer indices (e.g. from `enumerate(timesteps)`) as timesteps to"
                             " `DPMPP2MDiscreteScheduler.step()` is not supported. Make sure to pass"
                             " one of the `scheduler.timesteps` as a timestep.")
        if self.config.prediction_type not in PREDICTION_TYPES:
            raise ValueError(f"prediction_type given as {self.config.prediction_type} must be one of `epsilon`, or `v_prediction`")
        if self._step_index is None:
            self._init_step_index(timestep)
        first = self._denoised_prev is None
        if not first and (self._denoised_prev.shape != sample.shape or self._denoised_prev.device != sample.device):
            raise ValueError(f"DPMPP2MDiscreteScheduler.step: sample of shape {tuple(sample.shape)} on {sample.device} in a run whose history has "
                             f"shape {tuple(self._denoised_prev.shape)} on {self._denoised_prev.device}; call set_timesteps to start a new run")
        history = torch.empty(sample.shape, dtype=torch.float32, device=sample.device) if first else self._denoised_prev
        prev = ops.multistep_step(model_output, sample.to(torch.float32), self.coefficients(self._step_index, first=first),
                                  history).to(model_output.dtype)
        self._denoised_prev = history
        self._step_index += 1
        if not return_dict:
            return (prev,)
        return EulerDiscreteSchedulerOutput(prev_sample=prev, pred_original_sample=None)
