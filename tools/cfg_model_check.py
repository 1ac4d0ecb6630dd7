#!/usr/bin/env python3
"""The tile-configuration plan of the built library (pt_igemm_plan: choose_cfg + plan_splits of csrc/igemm.hip) against the
measured sweeps (tools/igemm_cfg_sweep.py tables): for every shape the configuration the library picks, what it costs against the
best measured one, and the total regret weighted by how often the shape occurs in one loop iteration.  CPU only: the planner is
host code and touches no device.

    python tools/cfg_model_check.py profiles/r06/igemm_cfg_sweep_L_r06c.txt profiles/r06/igemm_cfg_sweep_M_r06c.txt
A what-if calibration (other constants in choose_cfg / plan_splits) is an edit of csrc/igemm.hip and a rebuild; this tool builds the
library when a source is newer than it.
"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from posetraj_amd import hip

FAKE = 1 << 20          # 16-byte-aligned stand-in for every device pointer: the planner never dereferences them


def plan(M, N, K, geglu, side):
    """(configuration, split-K count) of pt_igemm_f16 for the linear layer [M, K] x [K, N] (N packed: GEGLU halves it)."""
    p = hip.IgemmParams()
    p.x0 = p.w = p.out = p.splitk_ws = FAKE
    p.C0, p.ld0 = K, K
    p.Nimg, p.Hin, p.Win, p.Hout, p.Wout, p.KH, p.KW, p.stride = M, 1, 1, 1, 1, 1, 1, 1
    p.M, p.N, p.K, p.Kpad, p.ldo = M, N, K, K, N // 2 if geglu else N
    p.act, p.out_scale = (1 if geglu else 0), 1.0
    p.splitk_ws_bytes = 1 << 62                              # any workspace the plan asks for is on offer
    if side:
        p.res, p.ldr = FAKE, N
    cfg, splits = C.c_int32(), C.c_int32()
    hip.check(hip.lib().pt_igemm_plan(C.byref(p), C.byref(cfg), C.byref(splits), None), "pt_igemm_plan")
    return cfg.value, splits.value


def main(paths):
    hip.build()
    # launches per loop iteration of the swept shapes (profiles/r05/igemm_shapes_L_r05z4.txt; the same layers at the M row counts)
    COUNT = {(2560, 320): 0, (960, 320): 14, (320, 320): 17, (320, 1280): 0, (5120, 640): 21, (1920, 640): 14, (640, 640): 28, (640, 2560): 21,
             (10240, 1280): 21, (3840, 1280): 14, (1280, 1280): 28, (1280, 5120): 21, (1280, 11520): 12, (320, 2880): 11, (640, 5760): 9,
             (320, 960): 14, (640, 1920): 14, (1280, 3840): 14, (1280, 23040): 2, (640, 11520): 1, (320, 5760): 2, (1280, 2560): 2}
    tot_auto = tot_best = tot_model = 0.0
    for path in paths:
        print(f"== {path}")
        for line in open(path):
            parts = [c.strip() for c in line.split("|")]
            head = parts[0].split()
            if len(head) != 5 or not head[0].isdigit():
                continue
            M, N, K, g, r = (int(v) for v in head)
            us = {}
            for c, cell in zip((0, 1, 2, 3, 4), parts[1:6]):
                if cell != "-":
                    us[c] = float(cell.split("us")[0])
            auto = float(parts[6].split("us")[0])
            pick, s = plan(M, N, K, g, r)
            # a forced configuration 3 in the sweep was measured WITH the split plan of the shipped build; an un-split pick of 3 where
            # the shipped build splits (or the reverse) is not in the table: flagged
            best = min(us, key=us.get)
            n = COUNT.get((N, K), 1)
            rows = M
            if rows in (4032, 1260):
                n = {(1280, 11520): 19, (10240, 1280): 6, (1280, 5120): 6, (1280, 3840): 22, (1280, 1280): 12, (3840, 1280): 4, (1280, 23040): 3,
                     (1280, 2560): 3}.get((N, K), 1)
            flag = "" if pick == best else f"   <- best {best} {us[best]:.1f}us ({100 * (us[pick] / us[best] - 1):+.0f} %)"
            print(f"{M:7d} {N:6d} {K:6d} g{g} r{r}  model {pick}{' split ' + str(s) if s > 1 else '':9s} {us[pick]:8.1f}us  auto(shipped) {auto:8.1f}us  x{n:2d}{flag}")
            tot_auto += n * auto; tot_best += n * us[best]; tot_model += n * us[pick]
    print(f"weighted per iteration: shipped auto {tot_auto / 1e3:.2f} ms, this model {tot_model / 1e3:.2f} ms, best measured {tot_best / 1e3:.2f} ms")


if __name__ == "__main__":
    main(sys.argv[1:])
