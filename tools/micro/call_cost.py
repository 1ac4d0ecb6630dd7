"""Host cost of one call into the library: hip.check(hip.lib().pt_x(...), "pt_x") against hip.checked().pt_x(...).

    python tools/micro/call_cost.py          # CPU only: pt_prof_enable(0) touches no device and returns 0

200 000 calls per repeat, five repeats of each form in one process, alternating order; nanoseconds per call."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from posetraj_amd import hip  # noqa: E402

N, REPEATS = 200_000, 5


def old():
    for _ in range(N):
        hip.check(hip.lib().pt_prof_enable(0), "pt_prof_enable")


def new():
    for _ in range(N):
        hip.checked().pt_prof_enable(0)


def main():
    ns = {"old": [], "new": []}
    old(); new()                                                # load both handles, warm the interpreter's caches
    for r in range(REPEATS):
        for name, fn in ((("old", old), ("new", new)) if r % 2 == 0 else (("new", new), ("old", old))):
            t = time.perf_counter()
            fn()
            ns[name].append((time.perf_counter() - t) / N * 1e9)
    print("ns per call                                    repeats                    median   min   max  spread")
    for name, form in (("old", 'hip.check(hip.lib().pt_x(..), "pt_x")'), ("new", "hip.checked().pt_x(..)")):
        v = ns[name]
        print(f"{form:40s} {' '.join(f'{x:5.0f}' for x in v)}   {statistics.median(v):6.0f} {min(v):5.0f} {max(v):5.0f} {max(v) - min(v):6.0f}")
    d, allowed = statistics.median(ns["new"]) - statistics.median(ns["old"]), max(ns["old"]) - min(ns["old"])
    print(f"median(new) - median(old) = {d:+.0f} ns per call; bound: at most +{allowed:.0f} (the old form's own spread): {'within' if d <= allowed else 'EXCEEDED'}")
    return 0 if d <= allowed else 1


if __name__ == "__main__":
    sys.exit(main())
