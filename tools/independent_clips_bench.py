#!/usr/bin/env python3
"""What ``independent_clips=True`` costs and what a batch of two buys (profiles/r18/independent_clips.txt).

    python tools/independent_clips_bench.py --workload L|M [--infer-steps 8] [--runs 3]     # the denoise loop, K = 2
    python tools/independent_clips_bench.py --train [--steps 3] [--warmup 2]                 # the two-clip training step at 14 x 320 x 576

Loop: bench.py's networks (full-width random-init SVD U-Net + ControlNet, hipGraph + two streams) and its synthetic clips.  Three
schedules of the same two requests, ms per loop iteration each: the COUPLED batch (the reference's meaning of a batch, the default), the
INDEPENDENT batch (``independent_clips=True``: another context index in the temporal blocks, otherwise the same launches - the two
should agree within run-to-run spread), and the two requests as single clips one after the other (two iterations counted as one
step of two clips).  One capture run per schedule, then ``--runs`` timed runs (wall time around ``denoise`` with a device
synchronisation, as bench.py times its steps); the ratios are taken between the MEDIANS, in both legs.  Training:
``ControlNetTrainer`` at ``per_gpu_batch_size`` 2 with and without the flag, median wall time of ``--steps`` steps (forward + backward
+ AdamW) behind ``--warmup``.  One leg per run, so that a caller can put
each under its own time limit.  Prints one JSON line."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="M", choices=("L", "M"), help="bench.py's geometries: L = 14 x 576 x 1024, M = 14 x 320 x 576")
ap.add_argument("--train", action="store_true")
ap.add_argument("--runs", type=int, default=3, help="timed runs of every schedule of the loop leg (each run: the K = 2 requests once)")
ap.add_argument("--infer-steps", type=int, default=8)
ap.add_argument("--frames", type=int, default=14)
ap.add_argument("--steps", type=int, default=3, help="timed training steps per trainer")
ap.add_argument("--warmup", type=int, default=2)
a = ap.parse_args()
dev = torch.device("cuda:0")
K = 2


def loop_leg():
    import bench
    from posetraj_amd import (ControlNetSDVModel, EulerDiscreteScheduler, SVD_SCHEDULER_CONFIG, StableVideoDiffusionPipelineControlNet,
                              UNetSpatioTemporalConditionControlNetModel)
    height, width = bench.WORKLOADS[a.workload]
    unet = UNetSpatioTemporalConditionControlNetModel(**bench.SVD).init_random_(seed=100, device=dev)
    cn = ControlNetSDVModel(**bench.SVD).init_random_(seed=200, device=dev)
    sched = EulerDiscreteScheduler(**SVD_SCHEDULER_CONFIG)
    sched.set_timesteps(a.infer_steps)
    reqs = [bench.synth_clip(height, width, a.frames, bench.SVD["cross_attention_dim"], 1234 + k, dev, sched.init_noise_sigma) for k in range(K)]
    halves = lambda j: torch.cat([torch.cat([r[j][:1] for r in reqs]), torch.cat([r[j][1:] for r in reqs])])     # halves-major: uncond rows first
    batch = (torch.cat([r[0] for r in reqs]), halves(1), halves(2), halves(3))
    new_pipe = lambda: StableVideoDiffusionPipelineControlNet(unet=unet, controlnet=cn, scheduler=EulerDiscreteScheduler(**SVD_SCHEDULER_CONFIG))
    kw = dict(num_inference_steps=a.infer_steps, use_graph=True, overlap_streams=True)
    pipes = {"coupled": new_pipe(), "independent": new_pipe(), "singles": new_pipe()}          # one graph cache per schedule
    runs = {"coupled": lambda: [pipes["coupled"].denoise(*batch, **kw)],
            "independent": lambda: [pipes["independent"].denoise(*batch, independent_clips=True, **kw)],
            "singles": lambda: [pipes["singles"].denoise(*r, **kw) for r in reqs]}
    res, outs = {}, {}
    for name, run in runs.items():
        run()                                                            # captures (or finds) the graph
        torch.cuda.synchronize()
        tt = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            outs[name] = run()
            torch.cuda.synchronize()
            tt.append((time.perf_counter() - t0) / a.infer_steps * 1e3)
        res[name] = tt
        assert all(bool(torch.isfinite(o).all()) for o in outs[name])
    best = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    ind, single = outs["independent"][0], torch.cat(outs["singles"])
    rel = float((ind.double() - single.double()).norm() / single.double().norm())
    rel_c = float((outs["coupled"][0].double() - single.double()).norm() / single.double().norm())
    print(json.dumps({"leg": "loop", "workload": a.workload, "geometry": f"{a.frames}x{height}x{width}", "clips_in_batch": K, "infer_steps": a.infer_steps,
                      "ms_per_step_of_two_clips": {k: [round(x, 2) for x in v] for k, v in res.items()},
                      "independent_over_coupled": round(best["independent"] / best["coupled"], 4),
                      "batch_gain_over_sequential_singles": round(best["singles"] / best["independent"], 4),
                      "rel_l2_vs_the_single_clip_runs": {"independent": rel, "coupled": rel_c},
                      "max_memory_allocated_GB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}))


def train_leg():
    from posetraj_amd import ControlNetSDVModel, UNetSpatioTemporalConditionControlNetModel
    from posetraj_amd.training import ControlNetTrainer
    height, width = 320, 576
    cfg = dict(num_attention_heads=(5, 10, 20, 20), num_frames=a.frames)
    unet = UNetSpatioTemporalConditionControlNetModel(**cfg).init_random_(seed=1, device=dev, keep_source=True)
    cn = ControlNetSDVModel.from_unet(unet, conditioning_embedding_out_channels=(16, 32, 96, 256))
    sd, ccfg = cn.state_dict(), dict(cn.config)
    g = torch.Generator().manual_seed(3)
    for k in sd:                                                     # a ControlNet some way into training: the zero-convs have moved
        if k.startswith(("controlnet_down_blocks", "controlnet_mid_block", "controlnet_cond_embedding.conv_out")):
            sd[k] = (torch.randn(sd[k].shape, generator=g) * 0.02).half()
    del cn
    h, w, D = height // 8, width // 8, unet.config.cross_attention_dim
    lat = torch.randn(K, a.frames, 4, h, w, generator=g) * 0.18215 * 5
    emb = torch.randn(K, 1, D, generator=g)
    traj = torch.rand(K, a.frames, 3, height, width, generator=g) * 2 - 1
    mv = torch.tensor([127.0, 60.0])
    res, losses = {}, {}
    for name, flag in (("coupled", False), ("independent", True), ("coupled_again", False)):
        tr = ControlNetTrainer(ccfg, sd, unet, learning_rate=1e-5, conditioning_dropout_prob=0.1, freeze_gc=False, independent_clips=flag)
        gen = torch.Generator().manual_seed(5)
        for _ in range(a.warmup):
            tr.step(lat, emb, mv, traj, generator=gen)
        torch.cuda.synchronize()
        tt = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            out = tr.step(lat, emb, mv, traj, generator=gen)
            torch.cuda.synchronize()
            tt.append((time.perf_counter() - t0) * 1e3)
        res[name], losses[name] = tt, out["loss"]
        assert out["loss"] == out["loss"]
        del tr
        torch.cuda.empty_cache()
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    print(json.dumps({"leg": "train", "geometry": f"{a.frames}x{height}x{width}", "per_gpu_batch_size": K,
                      "ms_per_step": {k: [round(x, 1) for x in v] for k, v in res.items()},
                      "clips_per_s": {k: round(K / v * 1e3, 3) for k, v in med.items()},
                      "independent_over_coupled": round(med["independent"] / min(med["coupled"], med["coupled_again"]), 4),
                      "last_loss": losses, "peak_device_GiB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 1)}))


train_leg() if a.train else loop_leg()
