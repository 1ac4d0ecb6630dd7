"""Shared by tests/test_independent_clips_cpu.py and tests/test_independent_clips_gpu.py: the numpy model of ``vec_mode`` 3
(include/posetraj_hip.h), batches of DIFFERENT clips for the tiny networks of tests/parity.py, and the fp32 oracle's prediction for a
batch (the reference's coupled batch) and for one clip of it alone (what ``independent_clips=True`` must compute)."""
import numpy as np
import torch

FORWARD_BOUND = 1e-3              # the project's stated bound for one network forward, rel-L2 (tests/test_parity_ladder_gpu.py: TOL_UNET_FP32)
CHAINED_BOUND = 2.2e-3            # ... and for the two networks chained, one loop iteration (TOL_LOOP_FP32 there)
COND_SCALE = 0.9
# (Bc, frames, latent h, latent w): 8 x 24 has S = 192, 48, 12, 3 over the levels (the deepest attention has ODD S: the interleave's
# parity then depends on the CFG half); 16 x 8 has S = 128, 32, 8, 2 (even everywhere).  Latent sides are multiples of 8 (four levels).
FORWARD_CASES = [(2, 3, 8, 24), (3, 2, 8, 24), (2, 2, 16, 8), (3, 2, 16, 8)]
SEED = 7                          # tests/test_independent_clips_cpu.py holds these inputs to the discrimination condition


def mode2_index(m, vFS, vS, vB):
    """vec_mode 2: the reference's batch-wide interleave."""
    return ((m // vFS) * vS + m % vS) % vB


def mode3_index(m, vG, vFS, vS, vB):
    """vec_mode 3, the formula of include/posetraj_hip.h, for rows ``m`` (numpy integers)."""
    b = m // vFS
    return (((b // vG) * vS + m % vS) % (vB // vG)) * vG + b % vG


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def clip_batch(Bc, F, h, w, xdim=64, seed=SEED, change_clip=None):
    """A CFG batch of ``Bc`` clips that differ in everything, halves-major (row ``half * Bc + clip``): network input ``sample``
    ``[2 Bc, F, 8, h, w]`` (both halves of a clip share the noisy latent; the uncond half's image latent is zero), ``ehs`` ``[2 Bc, 1, D]``
    (uncond rows zero), ``ids``, ``cond`` (a clip's maps in both halves).  ``change_clip=c``: clip c's embedding, latent, image latent
    and maps redrawn from another generator, every other clip bit for bit what it was."""
    r16 = lambda t: t.half().float()
    lat, il, e, maps = [], [], [], []
    for c in range(Bc):
        g = torch.Generator().manual_seed(1000 * seed + 17 * c + (500 if c == change_clip else 0))
        lat.append(r16(torch.randn(F, 4, h, w, generator=g)))
        il.append(r16(torch.randn(1, 4, h, w, generator=g)).expand(F, 4, h, w))
        e.append(r16(torch.randn(1, xdim, generator=g)))
        maps.append(r16(torch.rand(F, 3, 8 * h, 8 * w, generator=g) * 2 - 1))
    lat, il, e, maps = (torch.stack(t) for t in (lat, il, e, maps))
    sample = torch.cat([torch.cat([lat, torch.zeros_like(il)], 2), torch.cat([lat, il], 2)])
    return dict(sample=sample, t=torch.tensor(1.137), ehs=torch.cat([torch.zeros_like(e), e]), ids=torch.tensor([[6, 128, 0.02]] * (2 * Bc)),
                cond=torch.cat([maps, maps]))


def one_clip(batch, c):
    """Request ``c`` of ``clip_batch`` as a CFG batch of its own: rows ``c`` and ``Bc + c``."""
    Bc = batch["sample"].shape[0] // 2
    rows = [c, Bc + c]
    return {k: (v if k == "t" else v[rows]) for k, v in batch.items()}


@torch.no_grad()
def oracle_prediction(cn_o, unet_o, i):
    """ControlNet residuals x COND_SCALE into the U-Net, fp32 on the CPU -> ``[B, F, 4, h, w]``.  On more than one clip this is the
    REFERENCE's batch: coupled through the temporal blocks' context."""
    down, mid = cn_o(i["sample"], i["t"], i["ehs"], i["ids"], controlnet_cond=i["cond"], return_dict=False, conditioning_scale=COND_SCALE)
    return unet_o(i["sample"], i["t"], i["ehs"], list(down), mid, return_dict=False, added_time_ids=i["ids"])[0]


@torch.no_grad()
def oracle_networks(cn_o, unet_o, i):
    """The fp32 oracle on ONE request: the ControlNet's unscaled residuals ``down`` / ``mid`` (``[2 F, C, h', w']``), the U-Net's
    prediction on them (``pred``: one network forward, the way tests/parity.py: net_ladder takes it) and the prediction of the two
    networks chained at COND_SCALE, as the loop runs them (``pred_chained``)."""
    down, mid = cn_o(i["sample"], i["t"], i["ehs"], i["ids"], controlnet_cond=i["cond"], return_dict=False)
    pred = unet_o(i["sample"], i["t"], i["ehs"], list(down), mid, return_dict=False, added_time_ids=i["ids"])[0]
    return dict(down=list(down), mid=mid, pred=pred, pred_chained=oracle_prediction(cn_o, unet_o, i))


def clip_rows(pred, c):
    """Rows ``c`` and ``Bc + c`` of a ``[2 Bc, ...]`` prediction."""
    Bc = pred.shape[0] // 2
    return pred[[c, Bc + c]]


def loop_requests(K, frames, h, w, xdim=64, seed=SEED):
    """K requests for the denoise loop, each drawn like tests/parity.py: loop_inputs draws one - ``(lat [1, F, 4, h, w], il [2, 4, h, w],
    emb [2, 1, D], cond [2, F, 3, H, W])`` - and the same as ONE batch, halves-major."""
    from tests import parity
    reqs = [parity.loop_inputs(100 * seed + 7 * k, frames, h, w, xdim) for k in range(K)]
    halves = lambda j: torch.cat([torch.cat([r[j][:1] for r in reqs]), torch.cat([r[j][1:] for r in reqs])])
    return reqs, (torch.cat([r[0] for r in reqs]), halves(1), halves(2), halves(3))


def integer_case(Bc, F, S, N=64, K=64, seed=0):
    """Small-integer operands of ``out = x . w^T + bias + res + vec[vidx(m)]`` (every sum exact in fp16 / fp32) and the rows of the
    CPU integer model for the mode-3 index; the table's rows are all different."""
    g = torch.Generator().manual_seed(seed + 100 * Bc + 10 * F + S)
    M = 2 * Bc * F * S
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()
    x, w, bias, res = ri(-3, 3, M, K), ri(-2, 2, N, K), ri(-4, 4, N), ri(-8, 8, M, N)
    vec = ri(-8, 8, 2 * Bc, N) + 32.0 * torch.arange(2 * Bc).float()[:, None]            # row r sits near 32 r: no two rows alike
    idx = torch.from_numpy(mode3_index(np.arange(M), Bc, F * S, S, 2 * Bc))
    want = x.double() @ w.double().t() + bias.double() + res.double() + vec.double()[idx]
    assert float(want.abs().max()) < 2048 and torch.equal(want.half().double(), want)    # exact in fp16
    return dict(M=M, x=x, w=w, bias=bias, res=res, vec=vec, idx=idx, want=want.half(), vec_kw=dict(vec_mode=3, vG=Bc, vFS=F * S, vS=S, vB=2 * Bc))
