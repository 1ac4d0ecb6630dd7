"""The folded upsampler pack (packing.pack_conv2d_upfold) on the CPU: nearest-2x upsampling + 3 x 3 convolution equals four 2 x 2
convolutions on the low-resolution input, one per output parity class, on weights summed at pack time; the rows of the four
classes scatter into the output through the row formula of ``pt_igemm_params.upsample2x == 2`` (include/posetraj_hip.h)."""
import pytest
import torch
import torch.nn.functional as F

from posetraj_amd.packing import pack_conv2d_upfold

GEOMS = [(2, 1, 1), (1, 1, 4), (2, 3, 1), (2, 5, 7)]     # (Nimg, Hin, Win): degenerate images, odd extents, Win no power of two


def _orow(mc: torch.Tensor, Win: int, py: int, px: int) -> torch.Tensor:
    return (mc // Win) * 4 * Win + py * 2 * Win + 2 * (mc % Win) + px


def _folded_forward(pk, x: torch.Tensor) -> torch.Tensor:
    """x [N, C, H, W] fp32 -> [N * 2H * 2W, Co] fp32 in output row order, from the pack's four blocks alone."""
    N, C, H, W = x.shape
    Np = pk.w.shape[0] // 4
    out = torch.zeros(N * 4 * H * W, pk.N)
    mc = torch.arange(N * H * W)
    for par in range(4):
        py, px = par >> 1, par & 1
        wb = pk.w[par * Np:par * Np + pk.N, :pk.K].float().reshape(pk.N, 2, 2, C).permute(0, 3, 1, 2)   # K ordered (a, b, ci)
        # origin shift (1 - py, 1 - px), output extent = input extent: pad that side by one, the other side by what is left
        xp = F.pad(x, (1 - px, px, 1 - py, py))
        y = F.conv2d(xp, wb) + pk.bias[:pk.N].float().view(1, -1, 1, 1)
        assert y.shape[-2:] == (H, W)
        out[_orow(mc, W, py, px)] = y.permute(0, 2, 3, 1).reshape(N * H * W, pk.N)
    return out


@pytest.mark.parametrize("geom", GEOMS)
def test_four_folded_convs_equal_the_nine_tap_form(geom):
    N, H, W = geom
    C, Co = 64, 24
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, C, H, W, generator=g)
    w = (torch.randn(Co, C, 3, 3, generator=g) / (9 * C) ** 0.5)
    b = (0.1 * torch.randn(Co, generator=g)).half().float()
    pk = pack_conv2d_upfold(w, b, "cpu")
    assert (pk.KH, pk.KW, pk.K, pk.N, pk.cin, pk.upfold) == (2, 2, 4 * C, Co, C, True)
    assert pk.w.shape == (4 * 128, 4 * C) and pk.w.dtype == torch.float16 and pk.bias.shape == (128,)
    # weights whose folded sums are fp16-representable (multiples of 1/64 up to 4 x 8/64): the pack loses nothing, so the four
    # 2 x 2 convolutions equal the 9-tap form to fp32 rounding
    w8 = (torch.randint(-8, 9, (Co, C, 3, 3), generator=g).float() / 64)
    got = _folded_forward(pack_conv2d_upfold(w8, b, "cpu"), x)
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w8, b, padding=1).permute(0, 2, 3, 1).reshape(-1, Co)
    rel = float((got - ref).norm() / ref.norm())
    assert rel < 1e-6, (geom, rel)


def test_row_formula_is_a_bijection_onto_the_output():
    for N, H, W in GEOMS:
        mc = torch.arange(N * H * W)
        rows = torch.cat([_orow(mc, W, par >> 1, par & 1) for par in range(4)])
        assert sorted(rows.tolist()) == list(range(4 * N * H * W))
        # row (img, 2 i + py, 2 j + px) of the [N, 2H, 2W] image
        img, i, j = mc // (H * W), (mc // W) % H, mc % W
        for par in range(4):
            py, px = par >> 1, par & 1
            assert torch.equal(_orow(mc, W, py, px), (img * 2 * H + 2 * i + py) * 2 * W + 2 * j + px)


def test_fp32_source_weights_are_rounded_once():
    g = torch.Generator().manual_seed(5)
    C, Co = 64, 8
    w = torch.randn(Co, C, 3, 3, generator=g)                # fp32, not fp16-representable
    pk = pack_conv2d_upfold(w, None, "cpu")
    assert pk.bias is None
    taps = (((0,), (1, 2)), ((0, 1), (2,)))
    wl = w.permute(0, 2, 3, 1)
    for par in range(4):
        for a in range(2):
            for b in range(2):
                s32 = sum(wl[:, ky, kx] for ky in taps[par >> 1][a] for kx in taps[par & 1][b])
                blk = pk.w[par * 128:par * 128 + Co, (a * 2 + b) * C:(a * 2 + b + 1) * C]
                assert torch.equal(blk, s32.half()), (par, a, b)
        assert not pk.w[par * 128 + Co:(par + 1) * 128].any()
    # the same from an fp16 state dict: summed in fp32, not in fp16
    pk16 = pack_conv2d_upfold(w.half(), None, "cpu")
    s = (w.half().float().permute(0, 2, 3, 1)[:, 1:, 1:].sum(dim=(1, 2))).half()     # par 0, tap (1, 1) <- ky, kx in {1, 2}
    assert torch.equal(pk16.w[:Co, 3 * C:4 * C], s)


def test_packer_refuses_what_the_kernels_do_not_serve():
    with pytest.raises(ValueError):
        pack_conv2d_upfold(torch.zeros(8, 32, 3, 3), None, "cpu")       # C % 64
    with pytest.raises(ValueError):
        pack_conv2d_upfold(torch.zeros(8, 64, 1, 1), None, "cpu")


def test_a_library_without_the_mode_is_an_error_not_wrong_output(monkeypatch):
    """PT_ABI_VERSION is the same before and after the mode exists, so ops.igemm probes the library (host only): one that knows
    the mode refuses ``upsample2x = 3``; one that takes it would read 2 as the gathered upsample."""
    from posetraj_amd import hip, ops
    monkeypatch.setattr(ops, "_fold_ok", None)
    ops._need_fold_mode()                                    # the tree's own library knows it
    assert ops._fold_ok is True

    class Older:
        @staticmethod
        def pt_igemm_plan(*a):
            return 0
    monkeypatch.setattr(ops, "_fold_ok", None)
    monkeypatch.setattr(hip, "lib", lambda: Older)
    with pytest.raises(RuntimeError, match="predates the folded upsampler"):
        ops._need_fold_mode()
