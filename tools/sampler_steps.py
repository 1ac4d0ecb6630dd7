#!/usr/bin/env python3
"""Steps against sampler: what DPM-Solver++(2M) (posetraj_amd.DPMPP2MDiscreteScheduler) buys over Euler (DESIGN 4.18;
profiles/r14/sampler_steps.txt).

    python tools/sampler_steps.py [--part a|b|ab] [--clips 5] [--workload L] [--out profiles/r14/sampler_steps.txt]

(a) Discretisation error on the tiny nets of tests/parity.py (14 x 8 x 8 latent, seeded inputs, scale 1.0, hipGraph + two streams):
    rel-L2 of the final latents of Euler and 2M at N = 8, 10, 12, 15, 20, 25, 50 to a 200-step run of each sampler.  Random-init tiny
    nets: this measures the solver on a smooth ODE, not the quality of a trained checkpoint.
(b) Time at full width, built the way bench.py builds its networks (random-init SVD U-Net + ControlNet, one synthetic 14-frame clip
    of the workload's geometry, hipGraph + two streams): ``denoise`` time per clip of Euler@25, 2M@25 and 2M@15, alternated in one
    process - one warm-up clip each, then ``--clips`` rounds of one clip each in turn, a device synchronisation around every clip.
    Reported: median, min and max per configuration, and the run-to-run spread of Euler@25 against which 2M@25 is read.
"""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from posetraj_amd import (ControlNetSDVModel, DPMPP2MDiscreteScheduler, EulerDiscreteScheduler, SVD_SCHEDULER_CONFIG,
                          StableVideoDiffusionPipelineControlNet, UNetSpatioTemporalConditionControlNetModel, hip)

ap = argparse.ArgumentParser()
ap.add_argument("--part", default="ab", choices=["a", "b", "ab"])
ap.add_argument("--clips", type=int, default=5)
ap.add_argument("--workload", default="L", choices=list(bench.WORKLOADS))
ap.add_argument("--frames", type=int, default=14)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r14", "sampler_steps.txt"))
a = ap.parse_args()
dev = torch.device("cuda:0")
SAMPLERS = {"euler": EulerDiscreteScheduler, "2m": DPMPP2MDiscreteScheduler}
lines = [f"tools/sampler_steps.py --part {a.part} --clips {a.clips} --workload {a.workload}   library {hip.source_digest()[:12]}   {torch.cuda.get_device_name(0)}"]


def say(s=""):
    print(s, flush=True)
    lines.append(s)


if "a" in a.part:
    from tests import parity as P
    cn_o, unet_o = P.build_oracle_nets(0)
    cn_h, unet_h = P.build_hip_nets(cn_o, unet_o, dev)
    lat, il, emb, cond = P.loop_inputs(0, 14, 8, 8, unet_o.config.cross_attention_dim)
    pipe = StableVideoDiffusionPipelineControlNet(unet=unet_h, controlnet=cn_h, scheduler=EulerDiscreteScheduler(**SVD_SCHEDULER_CONFIG))
    lat0 = (lat * float(pipe.scheduler.init_noise_sigma)).to(dev)

    def run(sampler, n):
        pipe.scheduler = SAMPLERS[sampler](**SVD_SCHEDULER_CONFIG)
        out = pipe.denoise(lat0, il.to(dev), emb.to(dev), cond.to(dev), num_inference_steps=n, controlnet_cond_scale=1.0, use_graph=True, overlap_streams=True)
        torch.cuda.synchronize()
        return out

    ref = {s: run(s, 200) for s in SAMPLERS}
    say()
    say("(a) tiny nets, 14 x 8 x 8, SVD Karras ladder 700 -> 0.002, scale 1.0: rel-L2 of the final latents (HIP path, hipGraph + two streams)")
    say(f"    the two 200-step references differ by {P.rel_l2(ref['2m'], ref['euler']):.3e}")
    say("      N   Euler | Euler@200   2M | Euler@200   Euler | 2M@200    2M | 2M@200    2M/Euler (to Euler@200)  (to 2M@200)")
    for n in (8, 10, 12, 15, 20, 25, 50):
        e, m = run("euler", n), run("2m", n)
        d = [P.rel_l2(e, ref["euler"]), P.rel_l2(m, ref["euler"]), P.rel_l2(e, ref["2m"]), P.rel_l2(m, ref["2m"])]
        say(f"    {n:3d}   {d[0]:.3e}           {d[1]:.3e}        {d[2]:.3e}         {d[3]:.3e}      {d[1] / d[0]:.3f}                    {d[3] / d[2]:.3f}")
    del pipe, cn_h, unet_h
    torch.cuda.empty_cache()

if "b" in a.part:
    height, width = bench.WORKLOADS[a.workload]
    unet = UNetSpatioTemporalConditionControlNetModel(**bench.SVD).init_random_(seed=100, device=dev)
    cn = ControlNetSDVModel(**bench.SVD).init_random_(seed=200, device=dev)
    euler = EulerDiscreteScheduler(**SVD_SCHEDULER_CONFIG)
    pipe = StableVideoDiffusionPipelineControlNet(unet=unet, controlnet=cn, scheduler=euler)
    two_m = DPMPP2MDiscreteScheduler.from_config(euler.config)
    euler.set_timesteps(25)
    lat, il, emb, cond = bench.synth_clip(height, width, a.frames, bench.SVD["cross_attention_dim"], 1234, dev, euler.init_noise_sigma)
    configs = [("Euler@25", euler, 25), ("2M@25", two_m, 25), ("2M@15", two_m, 15)]

    def clip(sched, n):
        pipe.scheduler = sched
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pipe.denoise(lat, il, emb, cond, num_inference_steps=n, use_graph=True, overlap_streams=True)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for name, sched, n in configs:                                  # warm-up: the first one captures the graph all three replay
        _, out = clip(sched, n)
        assert bool(torch.isfinite(out).all()), name
    graph = pipe._step_graphs.of_kind("plain").graph
    times = {name: [] for name, _, _ in configs}
    for _ in range(a.clips):
        for name, sched, n in configs:
            times[name].append(clip(sched, n)[0])
    assert pipe._step_graphs.of_kind("plain").graph is graph     # one captured graph served every clip
    say()
    say(f"(b) full width, {a.frames} x {height} x {width}, random-init SVD U-Net + ControlNet, hipGraph + two streams: ms per clip of `denoise`,")
    say(f"    {a.clips} clips each, alternated in one process after one warm-up clip each, synchronised around every clip")
    say("    config      median      min      max   ms/step (median)   clips")
    for name, _, n in configs:
        t = times[name]
        say(f"    {name:9s} {statistics.median(t):8.1f} {min(t):8.1f} {max(t):8.1f}   {statistics.median(t) / n:8.2f}           {' '.join('%.1f' % v for v in t)}")
    e, m, m15 = (statistics.median(times[k]) for k in ("Euler@25", "2M@25", "2M@15"))
    spread = max(times["Euler@25"]) - min(times["Euler@25"])
    say(f"    2M@25 - Euler@25 = {m - e:+.1f} ms ({(m / e - 1) * 100:+.2f} %); run-to-run spread of Euler@25 (max - min) = {spread:.1f} ms ({spread / e * 100:.2f} %)")
    say(f"    2M@15 / Euler@25 = {m15 / e:.3f} (15 / 25 = 0.600)")
    say(f"    max memory allocated {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GB")

os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print("wrote", a.out)
