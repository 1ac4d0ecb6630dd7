#!/usr/bin/env python3
"""Did a source-level refactor change what the kernels execute?

    python tools/isa_compare.py PARENT_TREE [source.hip ...]     (default: every source of posetraj_amd/csrc)
    python tools/isa_compare.py PARENT_TREE --pool [--rename OLD=NEW ...] source.hip ...

Compiles each source of this tree and the file of the same name in PARENT_TREE/posetraj_amd/csrc to gfx950 assembly (the
compile-and-walk of tools/isa_wait_scan.py; no GPU needed) and compares per kernel, label names stripped:
  same   the instruction streams are identical (operands included);
  alloc  the opcode sequence is identical, registers or immediates differ;
  counts the sequence differs, but the instructions that do the work - MFMA, LDS reads / writes, LDS-DMA, other global / buffer
         loads and stores, scratch, barriers - occur equally often (address bookkeeping was re-scheduled or re-allocated);
  DIFF   one of those counts differs: printed, parent -> new.
--pool, for kernels that changed file: the listed sources (each may exist in one tree only) are pooled per tree.  A kernel is
compared with the one of its mangled name in the file of the same name if there is one, else with the one kernel of that name
in the rest of the other tree's pool (printed with the file it came from).  --rename OLD=NEW (repeatable) matches a parent
kernel whose short name (`dot_diff_kernel<1>`, as printed) is OLD with the new tree's NEW.  A kernel with no partner, or several, is DIFF.
Where both trees have been built it then compares posetraj_amd/build_resources.json: per kernel, spills, scratch and LDS must not
grow and the occupancy must not change (WORSE); the register count may move.
Exit status 1 if any kernel is DIFF or WORSE or exists in one tree only."""
import collections
import json
import os
import re
import sys

from isa_wait_scan import CSRC, kernel_streams, short

CLASSES = ("v_mfma", "ds_read", "ds_write", "global_load_lds", "global_load", "global_store", "global_atomic", "buffer_",
           "scratch_", "s_barrier")


def klass(op: str) -> str:
    for c in CLASSES:                                        # global_load_lds before global_load
        if op.startswith(c):
            return c
    return ""


def resources(parent_tree: str, renames=()) -> int:
    paths = [os.path.join(t, "posetraj_amd", "build_resources.json") for t in (parent_tree, os.path.dirname(os.path.dirname(CSRC)))]
    if not all(os.path.exists(p) for p in paths):
        print("resources: build both trees first (posetraj_amd/build_resources.json)")
        return 0
    a, b = (json.load(open(p)) for p in paths)
    for old, new in dict(renames).items():                        # a renamed kernel's row under its new name
        hit = [k for k in b if short(k) == new]
        for k in [k for k in a if short(k) == old and k not in b and len(hit) == 1]:
            a[hit[0]] = a.pop(k)
    bad = moved = 0
    for k in sorted(set(a) | set(b)):
        x, y = a.get(k, {}), b.get(k, {})
        worse = [f for f in ("VGPRs Spill", "SGPRs Spill", "ScratchSize", "LDS Size") if y.get(f, 0) > x.get(f, 0)]
        if worse or x.get("Occupancy") != y.get("Occupancy") or not x or not y:
            bad += 1
            print(f"resources          WORSE  {short(k)}: " + ", ".join(f"{f} {x.get(f)} -> {y.get(f)}" for f in sorted(set(x) | set(y)) if x.get(f) != y.get(f)))
        elif x != y:
            moved += 1
            print(f"resources          moved  {short(k)}: " + ", ".join(f"{f} {x[f]} -> {y[f]}" for f in sorted(x) if x[f] != y.get(f)))
    print(f"resources          {len(b)} kernels: {len(b) - bad - moved} equal, {moved} moved, {bad} WORSE")
    return bad


def compare(src: str, k: str, a: list, b: list, tally, origin: str = "") -> int:
    """One kernel of source `src`, parent stream a against new stream b: its verdict into `tally`, a line unless it is an unmoved `same`."""
    sa, sb = ([re.sub(r"\.L\w+", ".L", t) for t in x] for x in (a, b))
    oa, ob = ([t.split()[0] for t in s] for s in (sa, sb))
    ca, cb = (collections.Counter(filter(None, map(klass, o))) for o in (oa, ob))
    verdict = "same" if sa == sb else "alloc" if oa == ob else "counts" if ca == cb else "DIFF"
    tally[verdict] += 1
    if verdict == "DIFF":
        print(f"{src:18s} DIFF   {short(k)}{origin}: " + ", ".join(f"{c} {ca[c]} -> {cb[c]}" for c in CLASSES if ca[c] != cb[c]))
    elif verdict != "same":
        waits = sum(o == "s_waitcnt" for o in oa), sum(o == "s_waitcnt" for o in ob)
        print(f"{src:18s} {verdict:6s} {short(k)}{origin}: {len(oa)} -> {len(ob)} instructions, s_waitcnt {waits[0]} -> {waits[1]}")
    elif origin:
        print(f"{src:18s} same   {short(k)}{origin}")
    return verdict == "DIFF"


def pooled(parent: str, names: list, renames: dict) -> int:
    old, new = ({n: kernel_streams(os.path.join(d, n)) for n in names if os.path.exists(os.path.join(d, n))} for d in (parent, CSRC))
    bad, tallies = 0, {n: collections.Counter() for n in new}
    for n in new:                                            # the kernels that stayed in their file
        for k in sorted(set(old.get(n, ())) & set(new[n])):
            bad += compare(n, k, old[n].pop(k), new[n].pop(k), tallies[n])
    for n, k in sorted((n, k) for n in old for k in old[n]):      # the rest: moved, renamed or gone
        want = renames.get(short(k))
        hits = [(m, j) for m in new for j in new[m] if (short(j) == want if want else j == k)]
        if len(hits) != 1:
            print(f"{n:18s} DIFF   {short(k)}: {'only in the parent tree' if not hits else f'{len(hits)} candidates in the new tree'}")
            bad += 1
            continue
        m, j = hits[0]
        bad += compare(m, j, old[n][k], new[m].pop(j), tallies[m], f"  (from {n}" + (f": {short(k)}" if want else "") + ")")
    for m in new:
        for j in sorted(new[m]):
            print(f"{m:18s} DIFF   {short(j)}: only in the new tree")
            bad += 1
        print(f"{m:18s} {sum(tallies[m].values()) + len(new[m])} kernels: " + ", ".join(f"{c} {v}" for v, c in tallies[m].items()))
    return bad


def main():
    args, pool, renames = sys.argv[2:], False, {}
    while args and args[0].startswith("--"):
        opt = args.pop(0)
        if opt == "--pool":
            pool = True
        elif opt == "--rename":
            old, new = args.pop(0).split("=", 1)
            renames[old] = new
        else:
            sys.exit(f"unknown option {opt}")
    parent = os.path.join(sys.argv[1], "posetraj_amd", "csrc")
    if pool:
        bad = pooled(parent, [os.path.basename(a) for a in args], renames)
        sys.exit(1 if bad + resources(sys.argv[1], renames) else 0)
    srcs = args or sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip"))
    bad = 0
    for src in srcs:
        a, b = kernel_streams(src, parent), kernel_streams(src)
        tally = collections.Counter()
        for k in sorted(set(a) | set(b)):
            if k not in a or k not in b:
                print(f"{os.path.basename(src):18s} DIFF   {short(k)}: only in the {'parent' if k in a else 'new'} tree")
                bad += 1
                continue
            bad += compare(os.path.basename(src), k, a[k], b[k], tally)
        print(f"{os.path.basename(src):18s} {len(b)} kernels: " + ", ".join(f"{n} {v}" for v, n in tally.items()))
    bad += resources(sys.argv[1])
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
