#!/usr/bin/env python3
"""Temporal attention at 33 - 128 frames on the MI355X (profiles/r10/temporal_long_fwd.txt, temporal_long_bwd_ab.txt are its output).

  --fwd   ops.attn_temporal timed as tools/norm_bench.py does (read qkv + write out, TB/s) at the level-0 geometry of both
          workloads (B = 2, heads 5, head_dim 64, S = 40 x 72 and 72 x 128) and the level-2 one (heads 20, S = 10 x 18 and 18 x 32),
          F = 32 (the two-block kernel) and F = 48, 64, 96, 128 (the long-clip kernel).
  --bwd   ptt_attn_temporal_bwd_long_f16 against the recomputing path autodiff._attention_backward on the same inputs, alternating,
          B = 1, head_dim 64: S = 40 x 72, heads 5 and S = 10 x 18, heads 20, at F = 48 and 64; the rel-L2 between the two results is
          printed beside the times.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from posetraj_amd import autodiff as AD, hip, ops

dev = torch.device("cuda:0")


def timed(fn, n=10, rounds=3):
    """[us per call] of ``rounds`` windows of ``n`` calls, after a warm-up."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / n * 1e3)
    return out


def forward():
    for (B, S, heads) in [(2, 40 * 72, 5), (2, 72 * 128, 5), (2, 10 * 18, 20), (2, 18 * 32, 20)]:
        C = heads * 64
        for F in (32, 48, 64, 96, 128):
            qkv = torch.randn(B * F * S, 3 * C, device=dev, dtype=torch.float16)
            us = min(timed(lambda: ops.attn_temporal(qkv, B, F, S, heads, 64)))
            nbytes = qkv.numel() * 2 + B * F * S * C * 2
            print(f"attn_temporal   B={B} F={F:3d} S={S:5d} heads={heads:3d}: {us:9.1f} us  {nbytes / us / 1e6:6.2f} TB/s (read qkv + write out)", flush=True)
            del qkv


def backward():
    for (S, heads) in [(40 * 72, 5), (10 * 18, 20)]:
        for F in (48, 64):
            B, hd = 1, 64
            C = heads * hd
            qkv = torch.randn(B * F * S, 3 * C, device=dev, dtype=torch.float16)
            dy = torch.randn(B * F * S, C, device=dev, dtype=torch.float16)
            dq = torch.empty_like(qkv)

            def fused():
                hip.checked().ptt_attn_temporal_bwd_long_f16(qkv.data_ptr(), 3 * C, C, 2 * C, dy.data_ptr(), C, dq.data_ptr(), 3 * C, B, F, S, heads, hd,
                                                             hd ** -0.5, ops._stream())

            def recompute():
                return AD._attention_backward(qkv, dy, C, heads, hd, F, S, (B, F * S, S, 1), 1)

            fused()
            ref = recompute()
            d = float((dq.double() - ref.double()).norm() / ref.double().norm())
            tf, tr = [], []
            for _ in range(3):                                # alternate the two
                tf += timed(fused, rounds=1)
                tr += timed(recompute, rounds=1)
            print(f"attn_temporal_bwd B={B} F={F:3d} S={S:5d} heads={heads:3d}: fused {min(tf):9.1f} us (windows {' '.join(f'{t:.1f}' for t in tf)})  "
                  f"recompute {min(tr):9.1f} us (windows {' '.join(f'{t:.1f}' for t in tr)})  fused / recompute {min(tf) / min(tr):.3f}  "
                  f"rel-L2 between them {d:.2e}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--fwd", action="store_true")
    ap.add_argument("--bwd", action="store_true")
    a = ap.parse_args()
    ops.ensure_ready(dev)
    if a.fwd or not a.bwd:
        forward()
    if a.bwd or not a.fwd:
        backward()
