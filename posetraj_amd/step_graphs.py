"""The denoise loop's step states (``StableVideoDiffusionPipelineControlNet.denoise``): what one KIND of step - "plain",
"weighted", "off" - keeps between iterations and, as a captured hipGraph, between clips.  The ~2 500 launches of ControlNet + U-Net are
captured ONCE over static input buffers and replayed per iteration and for later clips of the same geometry; the fused loop kernels
around them carry the per-step scalars and stay eager.  Later captures of a geometry share the first one's memory pool (the kinds
replay one after the other on one stream, each prediction is consumed before the next replay)."""
from typing import NamedTuple, Optional

import torch

from . import ops


class GraphKey(NamedTuple):
    """Everything a captured step depends on.  Two keys are of the same geometry when they differ in ``kind`` / ``scale`` only."""
    Bc: int; F: int; hw: tuple; cond_shape: tuple; cam_shape: Optional[tuple]                  # geometry
    kind: Optional[str]; scale: Optional[float]          # "plain" | "weighted" | "off"; the scale a plain step bakes into its epilogues, or None
    unet: int; controlnet: int; unet_gen: int; controlnet_gen: int                             # identity
    overlap: bool; networks_name: Optional[str]
    dispatch: tuple      # every switch that decides which launches a step issues: ops.dispatch_key() + (("independent_clips", bool),) - denoise

    def geometry(self):
        return self._replace(kind=None, scale=None)


class StepGraphs(dict):
    """The captured states of one pipeline, ``GraphKey`` -> state: at most one per kind, all of one geometry.  Filled through ``insert``
    only; no device call in here (of a state it reads ``graph``, None until captured, and ``graph.pool()``)."""

    def of_kind(self, kind):
        return next((s for k, s in self.items() if k.kind == kind), None)

    def pool_for(self, key):
        """The memory pool of a captured state of ``key``'s geometry and another kind (the earliest one), or None."""
        geo = key.geometry()
        return next((s.graph.pool() for k, s in self.items() if k.kind != key.kind and k.geometry() == geo and s.graph is not None), None)

    def insert(self, key, state):
        """Drops every state of another geometry and the one of ``key``'s kind (a plain graph with another scale), then stores."""
        geo = key.geometry()
        for k in [k for k in self if k.kind == key.kind or k.geometry() != geo]:
            del self[k]
        self[key] = state


def _into(buf, src):
    """``src`` into the buffer ``buf`` that a captured graph reads (a clone at first use); None stays None."""
    return None if src is None else src.clone() if buf is None else buf.copy_(src)


class StepState:
    """One kind of step.  ``run(state, sample, t)`` launches its networks.  With a ``key`` the state is static: it owns copies of the
    clip's inputs and its condition embedding at addresses a captured graph reads, ``capture`` makes the graph and ``step`` replays
    it.  Without one it refers to the caller's tensors and ``step`` launches eagerly (the ControlNet's own cache holds the embedding).

    ``windows`` (optional, ``posetraj_amd.windows.WindowStaging``; set per call by the windowed loop and cleared by it): the latents are a
    long video ``[1, Ft, 4, h, w]`` and a step evaluates one group of its windows - the plan gives the size of ``xin`` and the staging
    call, everything else is the state of a batch of that many clips (same key, same graph)."""

    emb = ids = cond = cam = cond_embed = xin = t = graph = pred = None
    wbase = wbuf = folded = None             # weighted: the pooled weights and the same times ``folded``, per tap size
    windows = None

    def __init__(self, kind, run, key=None, windows=None):
        self.kind, self.run, self.key, self.windows = kind, run, key, windows

    def load(self, emb, ids, cond, cam, level_base, controlnet):
        """The clip's inputs, in place when the state is static; "off" reads neither the control maps nor the camera."""
        on = self.kind != "off"
        if self.key is None:
            self.emb, self.ids, self.cond, self.cam = emb, ids, cond, cam
        else:
            self.emb, self.ids = _into(self.emb, emb), _into(self.ids, ids)
            self.cond, self.cam = _into(self.cond, cond if on else None), _into(self.cam, cam if on else None)
            if on:                           # once per clip, eagerly: the graph reads this address whatever the ControlNet's cache holds
                self.cond_embed = controlnet._cond_embedding(self.cond, self.cam if controlnet.config.camera else None, out=self.cond_embed)
        if self.kind == "weighted":          # this call's pooled weights into buffers the state owns
            self.wbase = {sz: _into((self.wbase or {}).get(sz), b) for sz, b in level_base.items()}
            self.wbuf = self.wbuf or {sz: torch.empty_like(b) for sz, b in level_base.items()}
            self.folded = None

    def fold(self, scale):
        if self.kind == "weighted" and self.folded != scale:         # this step's scale into the factors the weighted kernels read
            for sz, b in self.wbase.items():
                torch.mul(b, scale, out=self.wbuf[sz])
            self.folded = scale

    def _stage(self, x, il, sigma, t):
        if self.windows is None:
            ops.scale_concat_input(x, il, sigma, out=self.xin)
        else:
            self.windows.stage(x, il, sigma, out=self.xin)
        self.t.fill_(float(t))

    def capture(self, pool, x, il, sigma, t):
        """Warm-up on a fresh stream (weight-only caches, allocator sizing), then the capture into ``pool``; both read defined values."""
        dev = x.device
        shape = (2 * x.shape[0], x.shape[1], x.shape[3], x.shape[4], 8) if self.windows is None else self.windows.input_shape(x.shape[3], x.shape[4])
        self.xin = torch.empty(shape, dtype=torch.float16, device=dev)
        self.t = torch.zeros(1, dtype=torch.float32, device=dev)
        for sz, b in (self.wbase or {}).items():
            self.wbuf[sz].copy_(b)
        self._stage(x, il, sigma, t)
        run = lambda: self.run(self, self.xin.permute(0, 1, 4, 2, 3), self.t)
        warm = torch.cuda.Stream(device=dev)
        warm.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(warm):
            run()
        torch.cuda.current_stream(dev).wait_stream(warm)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, pool=pool):
            self.pred = run()

    def step(self, x, il, sigma, t):
        """Latents ``x`` [Bc, F, 4, h, w] at ``sigma`` -> the fp32 channels-last prediction [2Bc, F, h, w, 4]."""
        if self.graph is None:
            xin = ops.scale_concat_input(x, il, sigma) if self.windows is None else self.windows.stage(x, il, sigma)
            return self.run(self, xin.permute(0, 1, 4, 2, 3), t)                                      # [2Bc, F, 8, h, w] view
        self._stage(x, il, sigma, t)
        self.graph.replay()
        return self.pred
