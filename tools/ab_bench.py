#!/usr/bin/env python3
"""A/B of library tuning switches on ONE box (devices differ by up to ~10 % in wall time, so numbers from different gpurun
calls do not compare): runs bench.py once per variant per round, interleaved, each in a fresh process, and prints the clip time
of each.

    python tools/ab_bench.py [--rounds 2] [--workload L] NAME=KEY1=V1,KEY2=V2 ...
A KEY with a dot is a module switch of posetraj_amd, set before bench.py starts (ops.FUSED_LNLIN=0, blocks.FF_CHUNK_BYTES=134217728);
any other KEY is an environment variable of the child (PT_LIB=<other .so>; BENCH_FLAGS=--no-overlap passes bench.py flags).
e.g. python tools/ab_bench.py base= two=ops.FUSED_LNLIN=0
"""
import ast
import json
import os
import subprocess
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bench = os.path.join(root, "bench.py")
CHILD = """
import importlib, runpy, sys
sys.path.insert(0, {root!r})
for mod, attr, val in {attrs!r}:
    m = importlib.import_module("posetraj_amd." + mod)
    setattr(m, attr, type(getattr(m, attr))(val))
sys.argv = [{bench!r}] + {argv!r}
runpy.run_path({bench!r}, run_name="__main__")
"""
args = sys.argv[1:]
rounds, workload = 2, "L"
while args and args[0].startswith("--"):
    if args[0] == "--rounds":
        rounds = int(args[1])
    elif args[0] == "--workload":
        workload = args[1]
    args = args[2:]
variants = []
for a in args:
    name, _, sets = a.partition("=")
    kv = dict(s.split("=", 1) for s in sets.split(",") if s)
    env = {k: v for k, v in kv.items() if "." not in k}
    attrs = [tuple(k.rsplit(".", 1)) + (ast.literal_eval(v),) for k, v in kv.items() if "." in k]
    variants.append((name, kv, env, attrs))
res = {v[0]: [] for v in variants}
for r in range(rounds):
    for name, kv, env, attrs in variants:
        argv = ["--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-profile", "--no-decode", "--workload", workload] + \
            env.get("BENCH_FLAGS", "").split()
        p = subprocess.run([sys.executable, "-c", CHILD.format(root=root, attrs=attrs, bench=bench, argv=argv)],
                           env=dict(os.environ, **{k: v for k, v in env.items() if k != "BENCH_FLAGS"}), capture_output=True, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        ms = json.loads(line[-1])["ms_per_step"] if line else float("nan")
        if not line:
            print(p.stderr[-2000:], flush=True)
        res[name].append(ms)
        print(f"round {r} {name:14s} {ms:9.1f} ms/clip   {kv}", flush=True)
base = min(res[variants[0][0]])
for name, *_ in variants:
    v = res[name]
    print(f"{name:14s} min {min(v):9.1f}  mean {sum(v) / len(v):9.1f}  vs {variants[0][0]} {min(v) / base:6.3f}")
