"""U-Net / ControlNet parity on the tiny nets for one subset of the residual-stream kinds that the oracle's fp16-fused storage
model keeps as fp16 pairs (oracle.quant.WIDE_STREAM; profiles/r02/parity_wide_kinds.txt).

    python tools/wide_kinds_ladder.py [KINDS]        KINDS = comma-separated subset of sc,xs,rb,tr,ds (default sc,xs,rb)
"""
import sys, os
sys.path.insert(0, os.getcwd())
import torch
from oracle import quant
from tests import parity as P
kinds = sys.argv[1] if len(sys.argv) > 1 else "sc,xs,rb"
quant.WIDE_STREAM = frozenset(k for k in kinds.split(",") if k)
for hw in ((16, 16), (40, 72)):
    d = P.net_ladder("cuda:0", latent_hw=hw, modes=("fp32", "fp16-fused"))
    print(kinds, hw, "unet hip|fp32 %.3e fused|fp32 %.3e   cn hip|fp32 %.3e fused|fp32 %.3e" % (
        d["unet"]["hip|fp32"], d["unet"]["fp16-fused|fp32"], d["controlnet_mid"]["hip|fp32"], d["controlnet_mid"]["fp16-fused|fp32"]), flush=True)
