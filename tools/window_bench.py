#!/usr/bin/env python3
"""What the windowed denoise loop costs (profiles/r19/windows.txt).

    python tools/window_bench.py [--workload M] [--frames 28] [--window-frames 14] [--window-stride 7] [--infer-steps 8] [--runs 3]

bench.py's networks (full-width random-init SVD U-Net + ControlNet, hipGraph + two streams) and its synthetic clips.  Three
schedules on the same tree, ms per loop iteration each: WINDOWS - one request of ``--frames`` frames as K overlapping windows of
``--window-frames``, all K in one group; BATCH - an ``independent_clips`` batch of K clips of ``--window-frames`` frames (what the windowed
iteration evaluates, without the two window passes and with the fused sampler epilogue); NATIVE - one clip of ``--frames`` frames through
the long-clip temporal attention.  One capture run per schedule, then ``--runs`` timed runs (wall time around ``denoise`` with a device
synchronisation, as bench.py times its steps); medians.  Then the two new kernels on their own at this geometry (hipEvents around
``--kernel-reps`` launches each, median of ``--runs``) and the flat sampler step the windowed loop adds.  Prints one JSON line."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="M", choices=("L", "M"), help="bench.py's geometries: L = 576 x 1024, M = 320 x 576")
ap.add_argument("--frames", type=int, default=28)
ap.add_argument("--window-frames", type=int, default=14)
ap.add_argument("--window-stride", type=int, default=7)
ap.add_argument("--infer-steps", type=int, default=8)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--kernel-reps", type=int, default=50)
a = ap.parse_args()
dev = torch.device("cuda:0")

import bench
from posetraj_amd import (ControlNetSDVModel, EulerDiscreteScheduler, SVD_SCHEDULER_CONFIG, StableVideoDiffusionPipelineControlNet,
                          UNetSpatioTemporalConditionControlNetModel, ops, windows as W)

height, width = bench.WORKLOADS[a.workload]
h, w = height // 8, width // 8
Ft, Fw = a.frames, a.window_frames
plan = W.window_plan(Ft, Fw, a.window_stride)
K = plan.K
unet = UNetSpatioTemporalConditionControlNetModel(**bench.SVD).init_random_(seed=100, device=dev)
cn = ControlNetSDVModel(**bench.SVD).init_random_(seed=200, device=dev)
sched = EulerDiscreteScheduler(**SVD_SCHEDULER_CONFIG)
sched.set_timesteps(a.infer_steps)
lat, il, emb, cond = bench.synth_clip(height, width, Ft, bench.SVD["cross_attention_dim"], 1234, dev, sched.init_noise_sigma)
cut = lambda t: torch.stack([t[:, s:s + Fw] for s in plan.starts], 1).flatten(0, 1).contiguous()
batch = (cut(lat), il.repeat_interleave(K, 0), emb.repeat_interleave(K, 0), cut(cond))              # the K windows as K clips, halves-major
new_pipe = lambda: StableVideoDiffusionPipelineControlNet(unet=unet, controlnet=cn, scheduler=EulerDiscreteScheduler(**SVD_SCHEDULER_CONFIG))
kw = dict(num_inference_steps=a.infer_steps, use_graph=True, overlap_streams=True)
pipes = {"windows": new_pipe(), "batch": new_pipe(), "native": new_pipe()}                            # one graph cache per schedule
runs = {"windows": lambda: pipes["windows"].denoise(lat, il, emb, cond, window_frames=Fw, window_stride=a.window_stride, **kw),
        "batch": lambda: pipes["batch"].denoise(*batch, independent_clips=True, **kw),
        "native": lambda: pipes["native"].denoise(lat, il, emb, cond, **kw)}
res = {}
for name, run in runs.items():
    run()                                                                # captures the graph
    torch.cuda.synchronize()
    tt = []
    for _ in range(a.runs):
        t0 = time.perf_counter()
        out = run()
        torch.cuda.synchronize()
        tt.append((time.perf_counter() - t0) / a.infer_steps * 1e3)
    res[name] = tt
    assert bool(torch.isfinite(out).all()), name
med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}


def kernel_ms(fn):
    """Median over ``--runs`` of the mean time of ``--kernel-reps`` back-to-back launches (hipEvents; 4 untimed launches first)."""
    for _ in range(4):
        fn()
    out = []
    for _ in range(a.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.kernel_reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / a.kernel_reps)
    return sorted(out)[len(out) // 2]


x = lat.float().contiguous()
xin = torch.empty((2 * K, Fw, h, w, 8), dtype=torch.float16, device=dev)
pred = torch.randn(2 * K, Fw, h, w, 4, device=dev)
guid = torch.linspace(1.0, 3.0, Fw, device=dev)
wts = torch.from_numpy(plan.weights).to(dev)
merged = torch.empty((1, Ft, 4, h, w), dtype=torch.float32, device=dev)
guid_b = guid.repeat(K, 1).contiguous()
xb = batch[0].float().contiguous()
xin_b = torch.empty_like(xin)
kernels = {
    "ptw_scale_concat_windows": kernel_ms(lambda: W.scale_concat_windows(x, il, 1.5, plan.starts, Fw, out=xin)),
    "ptw_cfg_window_merge": kernel_ms(lambda: W.cfg_window_merge(pred, guid, wts, plan.starts, Ft, out=merged)),
    "euler_step (flat, on the merged prediction)": kernel_ms(lambda: ops.euler_step(merged, x, 1.5, 1.2, 0)),
    "batch: pt_scale_concat_input": kernel_ms(lambda: ops.scale_concat_input(xb, batch[1], 1.5, out=xin_b)),
    "batch: pt_cfg_euler_step": kernel_ms(lambda: ops.cfg_euler_step(pred, guid_b, 1.5, 1.2, 0, xb)),
}
# bytes the two passes move per step: prologue reads K Fw latent frames (fp32) and writes 2 K Fw pixels of 16 bytes; the epilogue reads
# 2 K Fw prediction pixels of 16 bytes and writes Ft frames (fp32)
traffic = {"ptw_scale_concat_windows_MB": round((K * Fw * 4 * 4 + 2 * K * Fw * 16) * h * w / 1e6, 2),
           "ptw_cfg_window_merge_MB": round((2 * K * Fw * 16 + Ft * 4 * 4) * h * w / 1e6, 2)}
print(json.dumps({"geometry": f"Ft={Ft} Fw={Fw} s={a.window_stride} K={K}, {height}x{width}", "infer_steps": a.infer_steps,
                  "ms_per_iteration": {k: [round(v, 2) for v in vs] for k, vs in res.items()},
                  "median_ms": {k: round(v, 2) for k, v in med.items()},
                  "windows_over_batch": round(med["windows"] / med["batch"], 4), "windows_over_native": round(med["windows"] / med["native"], 4),
                  "windows_minus_batch_ms": round(med["windows"] - med["batch"], 3),
                  "kernel_ms": {k: round(v, 4) for k, v in kernels.items()}, "traffic_per_step": traffic,
                  "max_memory_allocated_GB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}))
