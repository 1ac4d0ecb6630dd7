"""Weight pre-packing: reference (diffusers-format) state-dict tensors -> the fp16 ``[Npad, Kpad]`` images the HIP
kernels stream (``include/posetraj_hip.h`` conventions).  Pure layout work (permute / pad / concatenate), done once
at load time on whatever device the source tensors live on."""
from __future__ import annotations

from typing import Optional

import torch

from .ops import Packed

BN, BK = 128, 64


def _round_up(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def _finish(w2d: torch.Tensor, bias: Optional[torch.Tensor], device, **kw) -> Packed:
    N, K = w2d.shape
    Np, Kp = _round_up(N, BN), _round_up(K, BK)
    w = torch.zeros((Np, Kp), dtype=torch.float16, device=device)
    w[:N, :K] = w2d.to(device=device, dtype=torch.float16)
    b = None
    if bias is not None:
        b = torch.zeros((Np,), dtype=torch.float16, device=device)
        b[:N] = bias.to(device=device, dtype=torch.float16)
    return Packed(w=w, bias=b, N=N, K=K, **kw)


def _geglu_interleave(t: torch.Tensor) -> torch.Tensor:
    """rows [value(0..I) | gate(0..I)] -> blocks of 16: value[0:16], gate[0:16], value[16:32], gate[16:32], ...
    so that a 32-column slab of the GEMM tile holds both operands of 16 outputs."""
    two_i = t.shape[0]
    inner = two_i // 2
    if inner % 16:
        raise ValueError(f"GEGLU inner width {inner} must be a multiple of 16")
    val = t[:inner].reshape(inner // 16, 16, *t.shape[1:])
    gate = t[inner:].reshape(inner // 16, 16, *t.shape[1:])
    return torch.stack([val, gate], dim=1).reshape(two_i, *t.shape[1:])


def pack_linear(w: torch.Tensor, bias: Optional[torch.Tensor], device, geglu: bool = False) -> Packed:
    w = w.detach().float()
    bias = None if bias is None else bias.detach().float()
    if geglu:
        w = _geglu_interleave(w)
        bias = None if bias is None else _geglu_interleave(bias)
    return _finish(w, bias, device, cin=w.shape[1], geglu=geglu)


def pack_conv2d(w: torch.Tensor, bias: Optional[torch.Tensor], device, stride: int = 1, padding: int = 1) -> Packed:
    """``[Co, Ci, kh, kw]`` -> ``[Co, kh*kw*Cip]`` with Ci zero-padded to a multiple of 8."""
    co, ci, kh, kw = w.shape
    cip = _round_up(ci, 8)
    wp = torch.zeros((co, kh, kw, cip), dtype=torch.float32, device=w.device)
    wp[..., :ci] = w.detach().float().permute(0, 2, 3, 1)
    return _finish(wp.reshape(co, kh * kw * cip), None if bias is None else bias.detach().float(), device,
                   KH=kh, KW=kw, stride=stride, pad_h=padding, pad_w=padding, cin=cip)


# Nearest-2x upsampling followed by a 3 x 3, padding-1 convolution reads only a 2 x 2 neighbourhood of the low-resolution image;
# which one depends on the parity (py, px) of the output pixel.  Output row parity p folds the three kernel rows into two taps:
_UPFOLD_TAPS = (((0,), (1, 2)), ((0, 1), (2,)))      # [p][a] -> the original ky (kx) summed into tap a


def pack_conv2d_upfold(w: torch.Tensor, bias: Optional[torch.Tensor], device) -> Packed:
    """``Upsample2D``'s 3 x 3 convolution ``[Co, Ci, 3, 3]`` as four 2 x 2 convolutions on the low-resolution input, one per output
    parity class ``par = 2 py + px`` (``pt_igemm_params.upsample2x == 2``): output pixel ``(2 i + py, 2 j + px)`` takes tap ``(a, b)``
    from input ``(i - (1 - py) + a, j - (1 - px) + b)``.  The four ``[Npad, Kpad]`` images (K ordered a, b, ci) are stacked by ``par``;
    the taps are summed in fp32 from whatever dtype the state dict holds and rounded to fp16 once.  The bias is shared."""
    co, ci, kh, kw = w.shape
    if (kh, kw) != (3, 3) or ci % 64:
        raise ValueError(f"unsupported upsampler weight {tuple(w.shape)}: 3 x 3 with a multiple of 64 input channels")
    w32 = w.detach().float().permute(0, 2, 3, 1)                               # [co, ky, kx, ci]
    blocks = []
    for par in range(4):
        rows, cols = _UPFOLD_TAPS[par >> 1], _UPFOLD_TAPS[par & 1]
        f = torch.stack([torch.stack([sum(w32[:, ky, kx] for ky in rows[a] for kx in cols[b]) for b in range(2)], dim=1)
                         for a in range(2)], dim=1)                              # [co, a, b, ci]
        blocks.append(_finish(f.reshape(co, 4 * ci), None, device).w)
    b = None
    if bias is not None:
        b = torch.zeros((blocks[0].shape[0],), dtype=torch.float16, device=device)
        b[:co] = bias.detach().to(device=device, dtype=torch.float16)
    return Packed(w=torch.cat(blocks, dim=0), bias=b, N=co, K=4 * ci, KH=2, KW=2, stride=1, pad_h=0, pad_w=0, cin=ci, upfold=True)


def pack_conv_t3(w: torch.Tensor, bias: Optional[torch.Tensor], device) -> Packed:
    """Conv3d ``[Co, Ci, 3, 1, 1]`` (padding (1,0,0)) -> a (3 x 1) convolution over the image (H', W') = (F, H*W)."""
    co, ci, kt, kh, kw = w.shape
    if (kt, kh, kw) != (3, 1, 1) or ci % 8:
        raise ValueError(f"unsupported temporal conv weight {tuple(w.shape)}")
    wp = w.detach().float().reshape(co, ci, 3).permute(0, 2, 1).reshape(co, 3 * ci)
    return _finish(wp, None if bias is None else bias.detach().float(), device, KH=3, KW=1, stride=1, pad_h=1, pad_w=0,
                   cin=ci)


def vec16(t: torch.Tensor, device) -> torch.Tensor:
    return t.detach().to(device=device, dtype=torch.float16).contiguous()
