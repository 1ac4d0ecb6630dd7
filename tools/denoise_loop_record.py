#!/usr/bin/env python3
"""The denoise loop of one checkout against another's, launch for launch (profiles/r16/denoise_loop_refactor.txt).

    python tools/denoise_loop_record.py ROOT record FILE          (ROOT: a checkout with its library built, e.g. the parent commit's)
    python tools/denoise_loop_record.py . compare FILE OUT.txt

Tiny nets and inputs of tests/test_control_schedule_gpu.py, seven scenarios (default, A weight map, B per-step scales, C window, D all
three, A on the camera twin, default under DPMPP2MDiscreteScheduler).  Per scenario: the igemm-family shape sequence of the eager loop
(``ops.Profiler.shapes``) and the final latents - eager, as graph + two streams, the graphs replayed for a second clip, eager again.
``compare`` wants equal sequences and ``torch.equal`` latents, writes the table to OUT.txt and exits 1 otherwise.  One process per call."""
import os, sys
root, mode, path = os.path.abspath(sys.argv[1]), sys.argv[2], sys.argv[3]
sys.path.insert(0, root)
import torch
import posetraj_amd
assert os.path.dirname(os.path.dirname(os.path.abspath(posetraj_amd.__file__))) == root, posetraj_amd.__file__
from posetraj_amd import DPMPP2MDiscreteScheduler, hip, ops
from tests import test_control_schedule_gpu as T

dev = torch.device("cuda:0")
benches = {False: T.Bench(dev, camera=False), True: T.Bench(dev, camera=True)}
CASES = [("default", "default", False, False), ("A", "A", False, False), ("B", "B", False, False), ("C", "C", False, False),
         ("D", "D", False, False), ("camera A", "A", True, False), ("default 2M", "default", False, True)]
res = {"digest": hip.source_digest()}
for label, scen, camera, two_m in CASES:
    b = benches[camera]
    pipe = b.new_pipe()
    if two_m:
        pipe.scheduler = DPMPP2MDiscreteScheduler.from_config(pipe.scheduler.config)
    b.cn_h._cond_cache = None
    ops.Profiler.shapes = []
    eager = b.run(scen, False, pipe)[-1]
    shapes, ops.Profiler.shapes = ops.Profiler.shapes, None
    graph = b.run(scen, True, pipe)[-1]
    graph_again = b.run(scen, True, pipe)[-1]                  # the replay of the captured states for a second clip
    eager_after = b.run(scen, False, pipe)[-1]
    assert torch.isfinite(eager).all()
    res[label] = dict(shapes=[tuple(int(v) for v in s) for s in shapes], eager=eager, graph=graph, graph_again=graph_again,
                      eager_after=eager_after)
    print(f"{label:11s} {len(shapes):5d} igemm-family launches recorded, graph == eager: {torch.equal(eager, graph)}", flush=True)

if mode == "record":
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    torch.save(res, path)
    print("recorded", path)
else:
    ref, lines, ok = torch.load(path), [], True
    same = ref["digest"] == res["digest"]
    ok &= same
    lines.append(f"hip.source_digest() parent {ref['digest']} this tree {res['digest']}: {'equal' if same else 'DIFFERENT'}")
    lines.append("scenario     launches (parent / this)   shape sequences   eager latents   graph + two streams   graph, second clip   eager after the graphs")
    for label, *_ in CASES:
        p, t = ref[label], res[label]
        seq = p["shapes"] == t["shapes"]
        eq = [torch.equal(p[k], t[k]) for k in ("eager", "graph", "graph_again", "eager_after")]
        ok &= seq and all(eq)
        lines.append(f"{label:11s}  {len(p['shapes']):5d} / {len(t['shapes']):5d}              {'equal' if seq else 'DIFFER':15s}   " +
                     "   ".join(f"{'bit-identical' if e else 'DIFFER':19s}" for e in eq))
    lines.append("ALL EQUAL" if ok else "MISMATCH")
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[4])), exist_ok=True)
    open(sys.argv[4], "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    sys.exit(0 if ok else 1)
