#!/usr/bin/env python3
"""What the control window and the weighted path cost in the denoise loop (profiles/r12/control_schedule.txt).

    python tools/control_schedule_bench.py --workload L|M [--clips 2] [--infer-steps 25]

bench.py's workload (full-width random-init SVD U-Net + ControlNet, one synthetic 14-frame clip, hipGraph + two streams), timed per
clip in four modes: the default call (every step plain), ``control_guidance_end = 0.5`` (plain + off steps), a ``control_weight`` map
(every step weighted), and both.  One capture clip per mode, then ``--clips`` timed clips (wall time around ``denoise`` with a device
synchronisation, as bench.py times its steps).  Derived: ms per plain / weighted iteration = clip time / steps; ms per OFF iteration
= (clip time with the window - on-steps x ms per plain iteration) / off-steps.  One workload per run, so that a caller can put each
run under its own time limit.  Prints one JSON line."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from posetraj_amd import (ControlNetSDVModel, EulerDiscreteScheduler, SVD_SCHEDULER_CONFIG, StableVideoDiffusionPipelineControlNet,
                          UNetSpatioTemporalConditionControlNetModel)
from posetraj_amd.control_schedule import control_plan

ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="L", choices=list(bench.WORKLOADS))
ap.add_argument("--clips", type=int, default=2)
ap.add_argument("--infer-steps", type=int, default=25)
ap.add_argument("--frames", type=int, default=14)
a = ap.parse_args()
dev = torch.device("cuda:0")
height, width = bench.WORKLOADS[a.workload]
unet = UNetSpatioTemporalConditionControlNetModel(**bench.SVD).init_random_(seed=100, device=dev)
cn = ControlNetSDVModel(**bench.SVD).init_random_(seed=200, device=dev)
sched = EulerDiscreteScheduler(**SVD_SCHEDULER_CONFIG)
pipe = StableVideoDiffusionPipelineControlNet(unet=unet, controlnet=cn, scheduler=sched)
sched.set_timesteps(a.infer_steps)
lat, il, emb, cond = bench.synth_clip(height, width, a.frames, bench.SVD["cross_attention_dim"], 1234, dev, sched.init_noise_sigma)
h, w = height // 8, width // 8
box = torch.zeros(a.frames, h, w, device=dev)
box[:, h // 4:3 * h // 4, w // 4:3 * w // 4] = 1.0                    # a dragged object's region: the middle quarter of the frame
modes = {"plain": {}, "window_end_0.5": dict(control_guidance_end=0.5), "weighted": dict(control_weight=box),
         "weighted_window_end_0.5": dict(control_weight=box, control_guidance_end=0.5)}
res = {}
for name, kw in modes.items():
    run = lambda: pipe.denoise(lat, il, emb, cond, num_inference_steps=a.infer_steps, use_graph=True, overlap_streams=True, **kw)
    run()                                                            # captures (or finds) the graphs of this mode's step kinds
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.clips):
        out = run()
    torch.cuda.synchronize()
    res[name] = (time.perf_counter() - t0) / a.clips * 1e3
    assert bool(torch.isfinite(out).all())
n_on = sum(on for on, _ in control_plan(a.infer_steps, 1.0, 0.0, 0.5))
n_off = a.infer_steps - n_on
plain_it, weighted_it = res["plain"] / a.infer_steps, res["weighted"] / a.infer_steps
print(json.dumps({"workload": a.workload, "geometry": f"{a.frames}x{height}x{width}", "infer_steps": a.infer_steps, "clips_timed": a.clips,
                  "ms_per_clip": {k: round(v, 2) for k, v in res.items()}, "window_end_0.5_steps_on_off": [n_on, n_off],
                  "ms_per_iteration": {"plain": round(plain_it, 2), "weighted": round(weighted_it, 2),
                                       "off": round((res["window_end_0.5"] - n_on * plain_it) / n_off, 2),
                                       "off_from_weighted_runs": round((res["weighted_window_end_0.5"] - n_on * weighted_it) / n_off, 2)},
                  "weighted_over_plain": round(weighted_it / plain_it, 4), "off_over_plain": round((res["window_end_0.5"] - n_on * plain_it) / n_off / plain_it, 4),
                  "graph_states": len(pipe._step_graphs), "max_memory_allocated_GB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}))
