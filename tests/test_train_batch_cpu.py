"""Batches of clips per training step (``ControlNetTrainer`` at ``per_gpu_batch_size`` > 1), the host side: the clip-batch extension
of the C ABI (include/posetraj_batch.h), the context index of the temporal blocks' cross-attention against the gather the
oracle's own temporal transformer performs, what the reference's spatial-loss expression does at two clips (a
B x B cross product over clip 0's residuals, which the product does NOT reproduce), and the shape checks of ``_step_inputs``."""
import contextlib
import io

import pytest
import torch


def ctx_index(B, F, S):
    """j(r) for every token row r = (b F + f) S + s: the context row of clip (b S + s) mod B."""
    r = torch.arange(B * F * S)
    return ((r // (F * S)) * S + r % S) % B


def test_batch_entry_points_refuse_on_the_host_and_size_their_workspace():
    """The host refuses what the kernels do not cover before any launch, and the workspace query follows its formula.  (The header's
    contract with the library: tests/test_abi_cpu.py.)"""
    from posetraj_amd import hip
    assert "batch.hip" in hip.SOURCES
    L, C = hip.lib(), hip.checked()
    assert L.ptb_add_rowvec_interleaved_f16(None, None, 3, 4, 64, 320, None, None) != 0 and b"null pointer" in L.pt_last_error()
    assert L.ptb_colsum_interleaved_f16(None, 3, 4, 64, 320, None, None) != 0 and b"ptb_colsum_interleaved_f16" in L.pt_last_error()
    # 2 strips x 3 classes -> 682 slabs wanted, 64 rows per slab at least: 4 slabs over the 256 rows of a class
    assert L.ptb_colsum_interleaved_ws_floats(3, 4, 64, 320) == 4 * 3 * 320
    assert L.ptb_colsum_interleaved_ws_floats(3, 4, 64, 12) == 0 and L.ptb_colsum_interleaved_ws_floats(0, 4, 64, 320) == 0
    with pytest.raises(RuntimeError, match="ptb_colsum_interleaved_det_f16"):
        C.ptb_colsum_interleaved_det_f16(None, 3, 4, 64, 320, None, None, 0, None)


def test_context_index_is_the_gather_of_the_oracles_temporal_block():
    """B = 3 clips, S = 4 positions (S mod B = 1: the class of a position shifts from clip to clip).  The context row of clip b is the
    constant b; a spy in place of the temporal block's cross-attention records which constant each of its ``[B S, F]``-major tokens
    was handed by ``TransformerSpatioTemporalModel.forward`` itself."""
    from oracle import blocks as OB
    B, F, hh, ww, C = 3, 2, 2, 2, 32
    S = hh * ww
    with contextlib.redirect_stdout(io.StringIO()):
        m = OB.TransformerSpatioTemporalModel(1, C, C, num_layers=1, cross_attention_dim=8)
    seen = {}

    class Spy(torch.nn.Module):
        def forward(self, x, encoder_hidden_states=None):
            seen["ctx"] = encoder_hidden_states[:, 0, 0].clone()              # one context per row p = b S + s of the block's [B S, F, C] view
            return torch.zeros_like(x)

    m.temporal_transformer_blocks[0].attn2 = Spy()
    ehs = torch.arange(B, dtype=torch.float32).repeat_interleave(F).view(B * F, 1, 1).expand(B * F, 1, 8).contiguous()
    with torch.no_grad():
        m(torch.randn(B * F, C, hh, ww, generator=torch.Generator().manual_seed(0)), ehs, torch.zeros(B, F))
    got = seen["ctx"].long()                                                  # [B S]
    assert got.shape == (B * S,)
    j = ctx_index(B, F, S).view(B, F, S)
    for f in range(F):                                                        # every frame of (b, s) sits in row b S + s of the block
        assert torch.equal(j[:, f].reshape(-1), got)
    assert not torch.equal(got, torch.arange(B * S) // S) and not torch.equal(got, torch.arange(B * S) % S % B)      # neither `b` nor `s mod B`


@pytest.fixture(scope="module")
def tiny():
    from oracle import init as OI, nets as ON
    from tests.golden.make_golden import TRAIN_CE, TRAIN_CFG
    with contextlib.redirect_stdout(io.StringIO()):
        cn = OI.seeded_init_(ON.ControlNetSDVModel(**TRAIN_CFG, conditioning_embedding_out_channels=TRAIN_CE), seed=81)
        un = OI.seeded_init_(ON.UNetSpatioTemporalConditionControlNetModel(**TRAIN_CFG), seed=82)
    return cn, un


def test_reference_spatial_loss_at_two_clips_is_a_cross_product_over_clip_zero(tiny):
    """``oracle.train.training_loss(use_spatial=True)`` restates the reference's expression (``:1392-1411``).  At B = 2 its
    ``loss_spatial`` is: every clip's one-frame pass receives the residuals of frame ``ran_idx`` of CLIP 0, and every clip's prediction
    meets every clip's sigma - written out below - not the mean of the per-clip losses the product computes."""
    from oracle import train as OT
    cn, un = tiny
    B, F, h, w, ri = 2, 4, 8, 8, 2
    g = torch.Generator().manual_seed(5)
    lat = torch.randn(B, F, 4, h, w, generator=g) * 0.9
    emb = torch.randn(B, 1, 16, generator=g)
    traj = torch.rand(B, F, 3, h * 8, w * 8, generator=g) * 2 - 1
    noise, sig, mv = torch.randn(lat.shape, generator=g), torch.tensor([0.7, 1.9]), torch.tensor([127.0, 60.0])
    with torch.no_grad():
        out = OT.training_loss(cn, un, lat, noise, sig, emb, mv, traj, 0.18215, ran_idx=ri, use_spatial=True)
        inp, noisy, ts, ehs, ids = out["inp_noisy_latents"], lat + noise * sig.view(B, 1, 1, 1, 1), out["timesteps"], out["encoder_hidden_states"], out["added_time_ids"]
        down, mid = cn(inp, ts, ehs, added_time_ids=ids, controlnet_cond=traj, return_dict=False)
        one = lambda res, m_: un(inp[:, ri].unsqueeze(1), ts, ehs, added_time_ids=ids, down_block_additional_residuals=res,
                                 mid_block_additional_residual=m_, return_dict=False)[0][:, 0]
        pred0 = one([d[ri].unsqueeze(0) for d in down], mid[ri].unsqueeze(0))                  # clip 0's frame, broadcast to both clips
        pred_own = one([d[ri::F] for d in down], mid[ri::F])                                    # clip b's own frame
    term = lambda p, s, b: (1 + s ** 2) / s ** 2 * (p * (-s / (s ** 2 + 1) ** 0.5) + noisy[b, ri] / (s ** 2 + 1) - lat[b, ri]) ** 2
    cross = torch.stack([torch.stack([term(pred0[j], sig[i], j) for j in range(B)]).mean() for i in range(B)]).mean()
    per_clip = torch.stack([term(pred_own[b], sig[b], b).mean() for b in range(B)]).mean()
    ref = float(out["loss_spatial"])
    print(f"reference expression at B = 2: {ref:.6f}; cross product written out {float(cross):.6f}; per-clip mean {float(per_clip):.6f}")
    assert abs(float(cross) / ref - 1) < 1e-5
    assert abs(float(per_clip) / ref - 1) > 1e-2


def test_step_inputs_checks_the_batch_dimension_of_every_argument():
    from posetraj_amd import training as T
    B, F, h, w = 2, 4, 8, 8
    lat, emb = torch.zeros(B, F, 4, h, w), torch.zeros(B, 1, 16)
    traj, mv = torch.zeros(B, F, 3, 8 * h, 8 * w), torch.tensor([127.0, 60.0])
    kw = dict(scaling_factor=0.18215, conditioning_dropout_prob=0.1, use_spatial=True, noise=None, sigmas=torch.tensor([0.7, 1.9]),
              random_p=torch.tensor([0.05, 0.7]), ran_idx=1, generator=torch.Generator().manual_seed(0), kernel=False, lazy_traj=True)
    run = lambda *a, **over: T._step_inputs(torch.device("cpu"), *a, None, **dict(kw, **over))
    I = run(lat, emb, mv, traj, camera_cond=torch.zeros(B, F, 12))
    assert I["dims"] == (B, F, h, w) and tuple(I["ids"].shape) == (B, 3) and tuple(I["cam_host"].shape) == (B, F, 12) and I["ran_idx"] == 1
    assert tuple(I["timesteps"].shape) == (B,) and I["cond_scale"].tolist()[0] > 0
    for name, args, over in (("motion_values", (lat, emb, torch.tensor([127.0]), traj), {}),
                             ("motion_values", (lat, emb, [127.0, 60.0, 1.0], traj), {}),
                             ("camera_cond", (lat, emb, mv, traj), dict(camera_cond=torch.zeros(1, F, 12))),
                             ("camera_cond", (lat, emb, mv, traj), dict(camera_cond=torch.zeros(B, F, 9))),
                             ("encoder_hidden_states", (lat, emb[:1], mv, traj), {}),
                             ("trajectories", (lat, emb, mv, traj[:, :3]), {}),
                             ("sigmas", (lat, emb, mv, traj), dict(sigmas=torch.tensor([0.7]))),
                             ("random_p", (lat, emb, mv, traj), dict(random_p=torch.tensor([0.1, 0.2, 0.3]))),
                             ("noise", (lat, emb, mv, traj), dict(noise=torch.zeros(1, F, 4, h, w))),
                             ("latents", (lat[:, :, :3], emb, mv, traj), {})):
        with pytest.raises(ValueError, match=name):
            run(*args, **over)
