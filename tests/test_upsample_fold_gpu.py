"""The folded upsampler (``pt_igemm_params.upsample2x == 2``, packing.pack_conv2d_upfold) on the MI355X: nearest-2x upsampling +
3 x 3 convolution as four 2 x 2 convolutions, one per output parity class.  Every result is compared with fp32 PyTorch on the
upsampled image at the kernel suite's tolerance (tests/test_kernels_gpu.py: rel-L2 <= 4e-4 for kernels whose error is their
fp16 output rounding); folding weights that were already fp16 adds one rounding per folded weight and sits at 2.5 - 2.6e-4."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
TOL = 4e-4                     # tests/test_kernels_gpu.py: TOL
TOL_BLOCKS_FIXTURE = 1.0e-3    # tests/test_parity_ladder_gpu.py: HIP blocks <-> reference-run blocks.npz
DEV = "cuda:0"

CASES = {                      # (Nimg, Hin, Win, C, Co)
    "a": (2, 5, 7, 64, 64),        # class_rows = 70: every class one ragged tile, one K tile per tap
    "b": (3, 10, 14, 128, 320),    # class_rows = 420: a full 256-row tile plus a ragged one per class
    "c": (2, 1, 1, 64, 64),        # degenerate images
    "d": (1, 3, 1, 64, 64),
    "e": (1, 16, 16, 320, 320),    # 256-row classes, exactly one tile each
}


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def h16(*shape, g, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).half().to(DEV)


_made = {}


def case(name):
    """Inputs, the folded pack and the fp32 reference of a case; computed once and shared (nothing writes to them)."""
    if name not in _made:
        from posetraj_amd.packing import pack_conv2d_upfold
        N, H, W, Ci, Co = CASES[name]
        g = torch.Generator().manual_seed(900 + ord(name))
        x = h16(N, H, W, Ci, g=g)
        w, b = h16(Co, Ci, 3, 3, g=g, scale=(9 * Ci) ** -0.5), h16(Co, g=g)
        ref = F.conv2d(F.interpolate(x.float().permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest"), w.float(), b.float(),
                       padding=1).permute(0, 2, 3, 1).reshape(N * 4 * H * W, Co)
        _made[name] = (x, w, b, pack_conv2d_upfold(w, b, DEV), ref)
    return _made[name]


def run_folded(name, cfg=-1):
    from posetraj_amd import hip, ops
    N, H, W, Ci, Co = CASES[name]
    x, _, _, pk, _ = case(name)
    hip.check(hip.lib().pt_igemm_force_config(cfg))
    try:
        y = ops.igemm(x, pk, geom=(N, H, W), upsample2x=True)
    finally:
        hip.check(hip.lib().pt_igemm_force_config(-1))
    assert y.shape == (N * 4 * H * W, Co)
    return y


@pytest.mark.parametrize("name", ["a", "c", "d", "e"])
def test_folded_upsample_conv(name):
    r = rel(run_folded(name), case(name)[4])
    print(f"folded upsample conv, case {name} {CASES[name]}: rel-L2 {r:.3e}")
    assert r < TOL, r


@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4])
def test_folded_upsample_conv_every_tile_config(cfg):
    """Case (b) under every tile configuration that serves it: class-local tile decoding in igemm8_kernel (0), igemm10_kernel (3)
    and the plain loop (1, 2, 4), with a full and a ragged M tile per class."""
    r = rel(run_folded("b", cfg), case("b")[4])
    print(f"folded upsample conv, case b {CASES['b']}, configuration {cfg}: rel-L2 {r:.3e}")
    assert r < TOL, r


def test_folded_upsample_conv_is_reproducible():
    assert torch.equal(run_folded("b"), run_folded("b"))


def test_profiler_records_the_mode():
    from posetraj_amd import ops
    old, ops.Profiler.shapes = ops.Profiler.shapes, []
    try:
        run_folded("a")
        shapes = ops.Profiler.shapes
    finally:
        ops.Profiler.shapes = old
    N, H, W, Ci, Co = CASES["a"]
    assert len(shapes) == 1 and shapes[0][:7] == (N * 4 * H * W, Co, 4 * Ci, 2, 2, 1, 2), shapes


def test_plain_pack_still_takes_the_gathered_upsample():
    """``upsample2x=True`` on an ordinary 3 x 3 pack still takes mode 1: the gather reads the low-resolution source through the
    coordinate shift, so its result is bit-identical to THIS build's kernel on the materialised upsampled image (same K order, same
    tiles) and within the kernel tolerance of fp32 torch.  Not a comparison with an earlier build: a change that moved both forms
    alike is held by the torch comparison here and by tests/test_kernels_gpu.py, test_backward_gpu.py and the VAE tests."""
    from posetraj_amd import hip, ops
    from posetraj_amd.packing import pack_conv2d
    N, H, W, Ci, Co = CASES["b"]
    x, w, b, _, ref = case("b")
    pk = pack_conv2d(w, b, DEV)
    assert not pk.upfold
    xu = x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2).contiguous()
    for cfg in (-1, 0, 3):
        hip.check(hip.lib().pt_igemm_force_config(cfg))
        try:
            y1 = ops.igemm(x, pk, geom=(N, H, W), upsample2x=True)
            y0 = ops.igemm(xu, pk, geom=(N, 2 * H, 2 * W))
        finally:
            hip.check(hip.lib().pt_igemm_force_config(-1))
        assert torch.equal(y1, y0), cfg
        assert rel(y1, ref) < TOL


def _params(x, pk, out, geom):
    from posetraj_amd import hip
    N, H, W = geom
    p = hip.IgemmParams()
    p.x0, p.C0, p.ld0 = x.data_ptr(), x.shape[-1], x.shape[-1]
    p.Nimg, p.Hin, p.Win, p.Hout, p.Wout = N, H, W, 2 * H, 2 * W
    p.KH, p.KW, p.stride, p.upsample2x = 2, 2, 1, 2
    p.M, p.N, p.K, p.Kpad = N * 4 * H * W, pk.N, pk.K, pk.Kpad
    p.w, p.bias = pk.w.data_ptr(), pk.bias.data_ptr()
    p.out, p.ldo = out.data_ptr(), out.stride(0)
    p.out_scale, p.cs_scale = 1.0, 1.0
    return p


def test_everything_the_upsampler_does_not_use_is_refused():
    """Each combination returns an error from the parameter checks (no launch: the output keeps its fill), and the raw
    parameter block itself - the one ops.igemm builds - is accepted."""
    from posetraj_amd import hip, ops
    ops.ensure_ready(DEV)
    L = hip.lib()
    N, H, W, Ci, Co = CASES["a"]
    x, _, _, pk, ref = case("a")
    out = torch.full((N * 4 * H * W, Co), 7.0, dtype=torch.float16, device=DEV)
    side = torch.zeros((N * 4 * H * W, Co), dtype=torch.float16, device=DEV)
    f32 = torch.zeros((N * 4 * H * W, Co), dtype=torch.float32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def bad(**kw):
        p = _params(x, pk, out, (N, H, W))
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    refused = {
        "x1": bad(x1=x.data_ptr(), C1=Ci, ld1=Ci, K=8 * Ci, Kpad=8 * Ci),
        "res": bad(res=side.data_ptr(), ldr=Co),
        "res_lo": bad(res=side.data_ptr(), res_lo=side.data_ptr(), ldr=Co),
        "vec": bad(vec=side.data_ptr(), ldv=Co, vec_mode=1, vG=H * W),
        "blend": bad(blend=side.data_ptr(), ldb=Co, alpha=0.5),
        "out_lo": bad(out_lo=side.data_ptr()),
        "out_f32": bad(out=f32.data_ptr(), out_f32=1),
        "silu": bad(act=2),
        "geglu": bad(act=1),
        "cs_cols": bad(cs_cols=8, cs_scale=2.0),
        "C0 % 64": bad(C0=32, K=128, Kpad=128),
        "3 x 3 taps": bad(KH=3, KW=3, K=9 * Ci, Kpad=9 * Ci),
        "extent": bad(Hout=H, Wout=W, M=N * H * W),
        "stride": bad(stride=2),
        "mode 3": bad(upsample2x=3),
    }
    for what, p in refused.items():
        assert L.pt_igemm_plan(C.byref(p), None, None, None) != 0, what
        assert L.pt_igemm_f16(C.byref(p), stream) != 0, what
        assert L.pt_last_error(), what
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    hip.check(L.pt_igemm_f16(C.byref(_params(x, pk, out, (N, H, W))), stream))
    assert rel(out, ref) < TOL


def test_folded_upsample_conv_never_runs_split_k():
    """A shape the planner would split in mode 1 terms (64 rows, K = 5120: 4 tiles of 256 x 320, 80 K tiles)."""
    from posetraj_amd import hip
    L = hip.lib()
    N, H, W, Ci = 1, 4, 4, 1280
    x = torch.zeros(1, dtype=torch.float16, device=DEV)       # the plan dereferences no pointer
    p = hip.IgemmParams()
    p.x0, p.w, p.out = x.data_ptr(), x.data_ptr(), x.data_ptr()
    p.C0, p.ld0, p.ldo = Ci, Ci, Ci
    p.Nimg, p.Hin, p.Win, p.Hout, p.Wout = N, H, W, 2 * H, 2 * W
    p.KH, p.KW, p.stride, p.upsample2x = 2, 2, 1, 2
    p.M, p.N, p.K, p.Kpad = N * 4 * H * W, Ci, 4 * Ci, 4 * Ci
    p.out_scale, p.cs_scale = 1.0, 1.0
    assert L.pt_igemm_splitk_ws_bytes(C.byref(p)) == 0
    cfg, splits, gm = C.c_int32(), C.c_int32(), C.c_int32()
    hip.check(L.pt_igemm_plan(C.byref(p), C.byref(cfg), C.byref(splits), C.byref(gm)))
    assert splits.value == 1
    p.KH, p.KW, p.upsample2x, p.K, p.Kpad, p.pad_h, p.pad_w = 3, 3, 1, 9 * Ci, 9 * Ci, 1, 1       # the gathered form of the same layer does
    assert L.pt_igemm_splitk_ws_bytes(C.byref(p)) > 0


def test_up_block_packs_its_upsampler_folded(golden):
    """CrossAttnUpBlockSpatioTemporal against the reference-run fixture (tests/golden/blocks.npz), as the parity ladder runs it:
    the block's ``upsamplers.0.conv`` (128 channels, 28 images of 4 x 6) goes through the folded form."""
    from posetraj_amd import blocks as HB, ops
    from tests import parity as P
    g = golden("blocks")
    B, Fr = P.BLK["B"], P.BLK["F"]
    i = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("in_")}
    cl = lambda t: ops.to_channels_last(t.to(DEV).half())
    ts, xs = HB.RowStack(), HB.RowStack()
    sd = {"u." + k: v for k, v in P.blocks_modules()["up"].state_dict().items()}
    up = HB.UpBlock(sd, "u.", True, 2, DEV, ts, xs)
    assert up.up.upfold and (up.up.KH, up.up.KW, up.up.K) == (2, 2, 4 * P.BLK["C2"])
    temb_all, xattn_all = ts.pack(DEV), xs.pack(DEV)
    emb = i["temb"][::Fr].contiguous()
    ehs = i["ehs"][::Fr].reshape(B, -1).contiguous()
    ctx = HB.Ctx(B=B, F=Fr, temb=ops.igemm(ops.silu(emb.to(DEV).half()), temb_all), xattn=ops.igemm(ehs.to(DEV).half(), xattn_all))
    old, ops.Profiler.shapes = ops.Profiler.shapes, []
    try:
        y = up.run(ctx, cl(i["up_x"]), [cl(i["up_skip_in"]), cl(i["up_skips"][0]), cl(i["up_skips"][1])])
        modes = [s[6] for s in ops.Profiler.shapes]
    finally:
        ops.Profiler.shapes = old
    assert modes.count(2) == 1 and modes.count(1) == 0, modes
    r = P.rel_l2(y.permute(0, 3, 1, 2), torch.from_numpy(g["up"]))
    print(f"up block with the folded upsampler vs the reference-run fixture: {r:.3e}")
    assert r < TOL_BLOCKS_FIXTURE, r
