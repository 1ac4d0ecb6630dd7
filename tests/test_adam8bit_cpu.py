"""``--use_8bit_adam`` on the host: the two code books, the planner that places every parameter's optimizer state, the table the
kernel reads, and the checkpoint format over a CPU-resident store.  No kernel runs here (tests/test_adam8bit_gpu.py)."""
import ctypes
import json
import os
import types

import pytest
import torch

HAND = [1, 320, 4095, 4096, 4232, 5000, 3 * 3 * 32 * 48]     # element counts: fp32 state below 4096, short last blocks, a convolution


def _store(counts):
    names = [f"p{i}" for i in range(len(counts))]
    shapes, offsets, n = {}, {}, 0
    for k, c in zip(names, counts):
        shapes[k], offsets[k] = (c,), n
        n += (c + 7) // 8 * 8                                 # ParamStore's rule
    return names, shapes, offsets, n


@pytest.mark.parametrize("signed", [True, False])
def test_books(signed):
    from posetraj_amd.optim import create_dynamic_map
    b = create_dynamic_map(signed)
    assert b.dtype == torch.float32 and b.shape == (256,)
    v = b.tolist()
    assert all(x < y for x, y in zip(v, v[1:]))               # sorted, distinct
    assert 0.0 in v and v[-1] == 1.0
    pos = min(x for x in v if x > 0)
    if signed:
        assert v.index(0.0) == 127 and abs(v[0] + 0.99297) < 1e-5 and abs(pos - 5.5e-7) < 1e-9
        assert sorted(-x for x in v[:-1]) == v[:-1]           # symmetric apart from 1.0
    else:
        assert v.index(0.0) == 0 and v[0] == 0.0 and abs(pos - 3.25e-7) < 1e-9


def test_planner_on_a_hand_made_list():
    from posetraj_amd.optim import ADAM8_BLOCK, ADAM8_MIN_SIZE, plan_8bit_state
    names, shapes, offsets, n = _store(HAND)
    plan = plan_8bit_state(names, shapes, offsets)
    assert (ADAM8_BLOCK, ADAM8_MIN_SIZE, plan["block"]) == (256, 4096, 256)
    assert [s[0] for s in plan["segments"]] == names
    blocks, f32, work = 0, 0, 0
    covered = torch.zeros(n, dtype=torch.int32)
    owner = {}                                                # block -> parameter
    for (k, start, count, state, kind, w), c in zip(plan["segments"], HAND):
        assert (start, count, kind, w) == (offsets[k], c, int(c >= 4096), work)
        units = -(-c // 256)
        tails = [min(256, c - 256 * u) for u in range(units)]
        assert sum(tails) == c and all(t == 256 for t in tails[:-1]) and tails[-1] == c - 256 * (units - 1)
        if kind:
            assert state == blocks
            for u in range(units):                            # no block belongs to two parameters, none crosses the parameter's end
                assert owner.setdefault(state + u, k) == k
                covered[start + 256 * u: start + 256 * u + tails[u]] += 1
            blocks += units
        else:
            assert state == f32 and state % 8 == 0
            covered[start:start + c] += 1
            f32 += (c + 7) // 8 * 8
        work += units
    assert plan["n_blocks"] == blocks == len(owner) == sum(-(-c // 256) for c in HAND if c >= 4096) == 16 + 17 + 20 + 54
    assert plan["n_work"] == work == sum(-(-c // 256) for c in HAND)
    assert plan["n_8bit"] == sum(c for c in HAND if c >= 4096) and plan["n_f32"] == 1 + 320 + 4095 and plan["n_f32_alloc"] == f32 == 8 + 320 + 4096
    live = torch.zeros(n, dtype=torch.int32)
    for k, c in zip(names, HAND):
        live[offsets[k]:offsets[k] + c] = 1
    assert torch.equal(covered, live)                         # every element once, the padding never
    assert plan["state_bytes"] == 2 * 256 * blocks + 8 * blocks + 8 * f32 + 2048 + 32 * len(HAND)
    with pytest.raises(ValueError):
        plan_8bit_state(names, shapes, dict(offsets, p1=4))


def test_full_width_controlnet_state_is_a_quarter_of_the_fp32_moments():
    from posetraj_amd.controlnet_sdv import ControlNetSDVModel
    from posetraj_amd.optim import plan_8bit_state
    spec = ControlNetSDVModel().param_spec()
    names = list(spec)
    shapes = {k: tuple(spec[k]) for k in names}
    offsets, n = {}, 0
    for k in names:
        offsets[k] = n
        n += (int(torch.Size(shapes[k]).numel()) + 7) // 8 * 8
    plan = plan_8bit_state(names, shapes, offsets)
    assert n > 600e6 and len(plan["segments"]) == len(names)
    assert plan["n_8bit"] + plan["n_f32"] == sum(torch.Size(s).numel() for s in shapes.values())
    assert plan["state_bytes"] <= 0.26 * 8 * n, plan["state_bytes"] / (8 * n)
    assert plan["n_work"] < 2 ** 31 and max(s[5] for s in plan["segments"]) < 2 ** 31


def test_segment_struct_and_the_host_refusal_of_the_step():
    """The table entry the kernel reads, as ``hip`` binds it from include/posetraj_optim.h (the header's contract with the library:
    tests/test_abi_cpu.py), and the step's refusal of null pointers before any launch."""
    from posetraj_amd import hip
    hip.build()
    assert [f[0] for f in hip.Adam8Segment._fields_] == ["start", "count", "state", "kind", "work"] and ctypes.sizeof(hip.Adam8Segment) == 32
    assert hip.ABIS["optim"].structs == {"pt_adam8_segment": hip.Adam8Segment}
    seg = hip.Adam8Segment(8, 320, 16, 1, 3)
    assert (seg.start, seg.count, seg.state, seg.kind, seg.work) == (8, 320, 16, 1, 3)
    L = hip.lib()
    assert L.pto_adamw8_f32(*([None] * 11), 0, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 1, 1.0, None, 0, None, 0.0, None) != 0      # refused on the host: no launch
    assert b"pto_adamw8_f32" in L.pt_last_error()


def test_checkpoint_of_the_8bit_state_round_trips_and_the_kinds_do_not_mix(tmp_path):
    """``save_state`` / ``load_state`` over a CPU-resident store: the file set, the keys of ``optimizer.safetensors``, the stored
    order of the codes, torch's order of a small convolution's fp32 moments, and the refusal to load the other kind."""
    from safetensors.torch import load_file
    from posetraj_amd import optim, train_state as TS
    from posetraj_amd.autodiff import ParamStore
    g = torch.Generator().manual_seed(0)
    sd = {"conv_in.weight": torch.randn(6, 5, 3, 3, generator=g), "conv_in.bias": torch.randn(6, generator=g),
          "big.conv.weight": torch.randn(32, 48, 3, 3, generator=g), "big.proj.weight": torch.randn(70, 60, generator=g),
          "mid.mix_factor": torch.tensor([0.25])}

    def trainer(eight):
        P = ParamStore(sd, "cpu")
        opt = (optim.AdamW8bit if eight else optim.AdamW)(P, lr=1e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
        return types.SimpleNamespace(params=P, optimizer=opt, config={"in_channels": 5}, optimizer_steps=0, skipped_steps=0, loss_scale=65536.0, _clean=0,
                                     growth_interval=2000, _micro=0, _accum_scale=None, lr=1e-5, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8,
                                     accumulation=1)
    a = trainer(True)
    A = a.optimizer
    assert A.kind == "adamw8bit" and A.exp_avg.numel() == A.exp_avg_sq.numel() == A.plan["n_f32_alloc"] < a.params.numel      # no full-size moment buffer
    assert not any(hasattr(a.params, name) for name in ("exp_avg", "exp_avg_sq", "adam8"))
    assert A.zero_codes == (127, 0) and bool((A.state1 == 127).all()) and bool((A.state2 == 0).all()) and float(A.absmax1.abs().sum()) == 0.0
    assert A.table.numel() == 32 * len(sd) and A.state1.numel() == 256 * A.plan["n_blocks"]
    A.state1.copy_(torch.randint(0, 256, A.state1.shape, generator=g, dtype=torch.uint8))
    A.state2.copy_(torch.randint(0, 256, A.state2.shape, generator=g, dtype=torch.uint8))
    A.absmax1.copy_(torch.rand(A.absmax1.shape, generator=g)); A.absmax2.copy_(torch.rand(A.absmax2.shape, generator=g))
    A.exp_avg.copy_(torch.randn(A.exp_avg.shape, generator=g)); A.exp_avg_sq.copy_(torch.rand(A.exp_avg_sq.shape, generator=g))
    a.optimizer_steps = 7
    ck = str(tmp_path / "checkpoint-7")
    TS.save_state(a, ck)
    assert sorted(os.listdir(ck)) == ["controlnet", "optimizer.safetensors", "trainer_state.json"]
    state = json.load(open(os.path.join(ck, "trainer_state.json")))
    assert state["optimizer"] == "adamw8bit" and state["optimizer_block_size"] == 256
    m = load_file(os.path.join(ck, "optimizer.safetensors"))
    big, small = ["big.conv.weight", "big.proj.weight"], ["conv_in.weight", "conv_in.bias", "mid.mix_factor"]
    assert set(m) == {"qmap1", "qmap2"} | {f"{p}.{k}" for p in ("state1", "state2", "absmax1", "absmax2") for k in big} | \
        {f"{p}.{k}" for p in ("exp_avg", "exp_avg_sq") for k in small}
    seg = {s[0]: s for s in A.plan["segments"]}
    for k in big:
        _, start, count, blk, kind, _ = seg[k]
        assert kind == 1 and m[f"state1.{k}"].dtype == torch.uint8 and m[f"state1.{k}"].shape == (count,)
        assert torch.equal(m[f"state1.{k}"], A.state1[256 * blk:256 * blk + count]) and m[f"absmax2.{k}"].shape == (-(-count // 256),)
    _, _, count, off, kind, _ = seg["conv_in.weight"]
    assert kind == 0 and m["exp_avg.conv_in.weight"].shape == (6, 5, 3, 3)
    assert torch.equal(m["exp_avg.conv_in.weight"].permute(2, 3, 0, 1).reshape(-1), A.exp_avg[off:off + count])      # stored tap-major
    assert torch.equal(m["qmap1"], A.qmap1) and torch.equal(m["qmap2"], A.qmap2)
    b = trainer(True)
    TS.load_state(b, ck)
    B = b.optimizer
    assert b.optimizer_steps == 7
    for k in sd:
        for x, y in zip(A._slices(k), B._slices(k)):
            assert torch.equal(x, y), k
    with pytest.raises(ValueError, match="'adamw8bit'.*'adamw'|'adamw'.*'adamw8bit'"):
        TS.load_state(trainer(False), ck)
    f = trainer(False)
    ck32 = str(tmp_path / "checkpoint-8")
    TS.save_state(f, ck32)
    s32 = json.load(open(os.path.join(ck32, "trainer_state.json")))
    assert "optimizer" not in s32 and "optimizer_block_size" not in s32
    assert set(load_file(os.path.join(ck32, "optimizer.safetensors"))) == {f"{p}.{k}" for p in ("exp_avg", "exp_avg_sq") for k in sd}
    with pytest.raises(ValueError, match="'adamw'.*'adamw8bit'"):
        TS.load_state(trainer(True), ck32)
    bad = dict(m, qmap1=m["qmap1"] * 2)
    with pytest.raises(ValueError, match="qmap1"):
        B.load_state_dict(bad)
    with pytest.raises(KeyError):
        B.load_state_dict({k: v for k, v in m.items() if k != "absmax1.big.conv.weight"})
