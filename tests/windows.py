"""Shared by tests/test_windows_cpu.py and tests/test_windows_gpu.py: the plan cases, the blend weights by their direct formula, a
numpy model of the two kernels of include/posetraj_window.h that walks the flat indices as the kernels do (with switches that plant
the faults the tests must notice), the same two passes by tensor slicing, and the merge in fp32 torch arithmetic for the device."""
import numpy as np
import torch

# (Ft, Fw, s) -> starts
PLAN_CASES = [((14, 14, 7), [0]), ((7, 4, 3), [0, 3]), ((9, 4, 2), [0, 2, 4, 5]), ((6, 4, 3), [0, 2]), ((5, 3, 1), [0, 1, 2])]
LAST_ACCEPTED, TOO_MANY = (65, 2, 1), (66, 2, 1)     # K = ceil((Ft - Fw) / s) + 1 = 64 (the limit) and 65
LOOP_BOUND = 1e-3                    # the project's stated bound for a loop's output, rel-L2 (tests/test_parity_ladder_gpu.py)


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def covering(Ft, Fw, starts):
    """Per frame the windows that cover it, ascending."""
    return [[k for k, s in enumerate(starts) if s <= f < s + Fw] for f in range(Ft)]


def direct_weights(Ft, Fw, starts):
    """``[K, Fw]`` fp32 by the definition: triangle ``t(j) = min(j + 1, Fw - j)`` over the sum of the covering windows' triangles, in
    fp64, rounded once."""
    tri = lambda j: min(j + 1, Fw - j)
    out = np.zeros((len(starts), Fw), dtype=np.float32)
    for f, ks in enumerate(covering(Ft, Fw, starts)):
        total = sum(float(tri(f - starts[k])) for k in ks)
        for k in ks:
            out[k, f - starts[k]] = np.float32(float(tri(f - starts[k])) / total)
    return out


# ---------------------------------------------------------------------------------------------------------- the prologue
def gather_model(lat, il, sigma, starts, Fw):
    """``ptw_scale_concat_windows`` pixel by pixel over the flat output index: ``lat`` fp32 ``[Ft, 4, h, w]``, ``il`` fp16
    ``[2, 4, h, w]`` -> fp16 ``[2K, Fw, h, w, 8]``."""
    Ft, _, h, w = lat.shape
    K, HW = len(starts), h * w
    s32 = np.float32(sigma)
    inv = np.float32(1.0) / np.sqrt(s32 * s32 + np.float32(1.0))
    latf, ilf = lat.reshape(-1), il.reshape(-1)
    out = np.zeros(2 * K * Fw * HW * 8, dtype=np.float16)
    for i in range(2 * K * Fw * HW):
        p, nf = i % HW, i // HW
        j, row = nf % Fw, nf // Fw
        half, k = row // K, row % K
        for c in range(4):
            out[i * 8 + c] = np.float16(latf[((starts[k] + j) * 4 + c) * HW + p] * inv)
            out[i * 8 + 4 + c] = ilf[(half * 4 + c) * HW + p]
    return out.reshape(2 * K, Fw, h, w, 8)


def gather_direct(lat, il, sigma, starts, Fw):
    """The same by slicing: window k is frames ``starts[k] .. + Fw`` scaled, both halves; channels 4..7 the half's image latent."""
    s32 = np.float32(sigma)
    inv = np.float32(1.0) / np.sqrt(s32 * s32 + np.float32(1.0))
    rows = []
    for half in range(2):
        for s in starts:
            x = (lat[s:s + Fw] * inv).astype(np.float16)                                   # [Fw, 4, h, w]
            rows.append(np.concatenate([x, np.broadcast_to(il[half], x.shape)], axis=1).transpose(0, 2, 3, 1))
    return np.stack(rows)


# ---------------------------------------------------------------------------------------------------------- the epilogue
def merge_model(pred, guidance, weights, starts, Ft, descending=False, global_guidance=False, swap_halves=False):
    """``ptw_cfg_window_merge`` pixel by pixel over the flat index of the long video, every operation one fp32 rounding (numpy float32
    scalars): ``pred`` fp32 or fp16 ``[2K, Fw, h, w, ldn]`` -> fp32 ``[Ft, 4, h, w]``.  The three switches plant faults: the covering
    windows in descending order, the guidance indexed by the frame of the long video (modulo Fw) instead of the window's, the two
    halves exchanged."""
    rows, Fw, h, w, ldn = pred.shape
    K, HW, f16 = rows // 2, h * w, pred.dtype == np.float16
    pf, wf = pred.reshape(-1), np.asarray(weights, dtype=np.float32).reshape(-1)
    g = np.asarray(guidance, dtype=np.float32).reshape(-1)
    out = np.zeros(Ft * 4 * HW, dtype=np.float32)
    for i in range(Ft * HW):
        p, f = i % HW, i // HW
        ks = [k for k in range(K) if starts[k] <= f < starts[k] + Fw]
        acc, first = [np.float32(0)] * 4, True
        for k in (reversed(ks) if descending else ks):
            j = f - starts[k]
            u = (((0 * K + k) * Fw + j) * HW + p) * ldn
            c = (((1 * K + k) * Fw + j) * HW + p) * ldn
            if swap_halves:
                u, c = c, u
            gj = g[f % Fw] if global_guidance else g[j]
            for ch in range(4):
                pu, pc = np.float32(pf[u + ch]), np.float32(pf[c + ch])
                d = np.float32(pc - pu)
                gd = np.float32(gj * d)
                mo = np.float32(pu + gd)
                if f16:
                    mo = np.float32(np.float16(mo))
                term = np.float32(wf[k * Fw + j] * mo)
                acc[ch] = term if first else np.float32(acc[ch] + term)
            first = False
        for ch in range(4):
            out[(f * 4 + ch) * HW + p] = acc[ch]
    return out.reshape(Ft, 4, h, w)


def merge_reference(pred, guidance, weights, starts, Ft):
    """The header's arithmetic in its stated order by tensor slicing, with torch ``sub`` / ``mul`` / ``add`` only (one fp32 rounding
    each, no fused multiply-add), on whatever device ``pred`` lives: fp16 or fp32 ``[2K, Fw, h, w, ldn]`` -> fp32 ``[Ft, 4, h, w]``."""
    rows, Fw, h, w, _ = pred.shape
    K = rows // 2
    out = torch.zeros((Ft, 4, h, w), dtype=torch.float32, device=pred.device)
    seen = [False] * Ft
    for k in range(K):
        pu, pc = pred[k, ..., :4].float(), pred[K + k, ..., :4].float()                  # [Fw, h, w, 4]
        d = torch.sub(pc, pu)
        mo = torch.add(pu, torch.mul(guidance.reshape(Fw, 1, 1, 1), d))
        if pred.dtype == torch.float16:
            mo = mo.half().float()
        term = torch.mul(weights[k].reshape(Fw, 1, 1, 1), mo).permute(0, 3, 1, 2)        # [Fw, 4, h, w]
        for j in range(Fw):
            f = starts[k] + j
            out[f] = term[j] if not seen[f] else torch.add(out[f], term[j])
            seen[f] = True
    assert all(seen)
    return out
