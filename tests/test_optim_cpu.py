"""``posetraj_amd/optim.py`` on the host: the two optimizer classes behind one interface over a CPU-resident store (no kernel runs:
construction launches nothing), and the checkpoint files of both kinds against fixtures written before the optimizer had an object
of its own.  The launches are tests/test_optim_gpu.py's."""
import inspect
import json
import os
import types

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HYPER = dict(lr=1e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
BIG, SMALL = ["big.conv.weight", "big.proj.weight"], ["conv_in.weight", "conv_in.bias", "mid.mix_factor"]
BUFFERS = {"adamw": ("exp_avg", "exp_avg_sq"), "adamw8bit": ("state1", "state2", "absmax1", "absmax2", "exp_avg", "exp_avg_sq")}


def _sd():
    """The state dict of tests/test_adam8bit_cpu.py's checkpoint test: a convolution under 4096 elements, one over, a linear layer
    over, a bias and a scalar."""
    g = torch.Generator().manual_seed(0)
    return {"conv_in.weight": torch.randn(6, 5, 3, 3, generator=g), "conv_in.bias": torch.randn(6, generator=g),
            "big.conv.weight": torch.randn(32, 48, 3, 3, generator=g), "big.proj.weight": torch.randn(70, 60, generator=g),
            "mid.mix_factor": torch.tensor([0.25])}


def _optimizer(kind, P):
    from posetraj_amd import optim
    return {"adamw": optim.AdamW, "adamw8bit": optim.AdamW8bit}[kind](P, **HYPER)


def _fill(opt, seed):
    g = torch.Generator().manual_seed(seed)
    for name in BUFFERS[opt.kind]:
        buf = getattr(opt, name)
        if buf.dtype == torch.uint8:
            buf.copy_(torch.randint(0, 256, buf.shape, generator=g, dtype=torch.uint8))
        else:
            buf.copy_(torch.rand(buf.shape, generator=g) if name.endswith(("sq", "2")) else torch.randn(buf.shape, generator=g))


def test_the_store_holds_no_optimizer_state():
    from posetraj_amd.autodiff import ParamStore
    P = ParamStore(_sd(), "cpu")
    assert not any(hasattr(P, name) for name in ("exp_avg", "exp_avg_sq", "adam8"))
    assert list(inspect.signature(ParamStore.__init__).parameters) == ["self", "sd", "device"]
    # "the master moved and the same pass wrote the fp16 mirror": the version advances and half_view() does not cast again
    v = P.version
    P.flat16.fill_(3.0)
    P.moved_with_mirror()
    assert P.version == v + 1 and bool((P.half_view("conv_in.bias") == 3.0).all())
    P.version += 1                                                 # a move without the mirror: the next half_view() casts
    assert torch.equal(P.half_view("conv_in.bias"), P.value("conv_in.bias").half())


@pytest.mark.parametrize("kind", ["adamw", "adamw8bit"])
def test_interface_on_a_cpu_store(kind):
    from posetraj_amd.autodiff import ParamStore
    sd = _sd()
    P = ParamStore(sd, "cpu")
    opt = _optimizer(kind, P)
    assert opt.kind == kind and (opt.betas, opt.eps, opt.weight_decay, opt.lr) == ((0.9, 0.999), 1e-8, 1e-2, 1e-5)
    if kind == "adamw":
        assert opt.exp_avg.shape == opt.exp_avg_sq.shape == (P.numel,) and opt.exp_avg.dtype == torch.float32
        assert float(opt.exp_avg.abs().sum()) == 0.0 == float(opt.exp_avg_sq.abs().sum())
        assert opt.state_bytes == 8 * P.numel and opt.checkpoint_meta() == {}
        want = {f"{p}.{k}" for p in ("exp_avg", "exp_avg_sq") for k in sd}
    else:
        assert opt.state_bytes == opt.plan["state_bytes"] < 8 * P.numel
        assert opt.checkpoint_meta() == {"optimizer": "adamw8bit", "optimizer_block_size": 256}
        assert opt.exp_avg.numel() == opt.plan["n_f32_alloc"] < P.numel and opt.zero_codes == (127, 0)
        want = {"qmap1", "qmap2"} | {f"{p}.{k}" for p in ("state1", "state2", "absmax1", "absmax2") for k in BIG} | \
            {f"{p}.{k}" for p in ("exp_avg", "exp_avg_sq") for k in SMALL}
    _fill(opt, 1)
    m = opt.state_dict()
    assert set(m) == want and all(t.device.type == "cpu" for t in m.values())
    for k in (sd if kind == "adamw" else SMALL):                   # fp32 moments travel in torch's shape and order
        assert m[f"exp_avg.{k}"].shape == sd[k].shape and m[f"exp_avg.{k}"].is_contiguous() and m[f"exp_avg.{k}"].dtype == torch.float32
    other = _optimizer(kind, ParamStore(sd, "cpu"))
    _fill(other, 2)
    other.load_state_dict(m)
    back = other.state_dict()
    assert set(back) == set(m) and all(back[k].dtype == m[k].dtype and torch.equal(back[k], m[k]) for k in m)
    for k in sd:                                                   # ... and so does every stored element (the padding between parameters is no state)
        if kind == "adamw":
            views = [(P.raw(getattr(opt, b), k), P.raw(getattr(other, b), k)) for b in BUFFERS[kind]]
        else:
            views = list(zip(opt._slices(k), other._slices(k)))
        assert all(torch.equal(x, y) for x, y in views), k
    # strict in names and shapes
    first = sorted(m)[0] if kind == "adamw" else "absmax1.big.conv.weight"
    with pytest.raises(KeyError):
        other.load_state_dict({k: v for k, v in m.items() if k != first})
    with pytest.raises(ValueError):
        other.load_state_dict(dict(m, **{"exp_avg.conv_in.bias": torch.zeros(7)}))
    # the other kind, and (8-bit) another block size, are refused with load_state's messages
    mine = dict(opt.checkpoint_meta())
    opt.check_checkpoint_meta(mine, "ck")
    swapped = {"optimizer": "adamw8bit", "optimizer_block_size": 256} if kind == "adamw" else {}
    with pytest.raises(ValueError, match="ck: the checkpoint holds the state of optimizer .* but the trainer runs .*"
                                         rf"\(use_8bit_adam={kind == 'adamw8bit'}\); states of 'adamw' and 'adamw8bit' are not converted into each other"):
        opt.check_checkpoint_meta(swapped, "ck")
    with pytest.raises(ValueError, match="'adamw8bit'.*'adamw'" if kind == "adamw" else "'adamw'.*'adamw8bit'"):
        opt.check_checkpoint_meta(swapped, "ck")
    if kind == "adamw8bit":
        with pytest.raises(ValueError, match="ck: 8-bit optimizer state in blocks of 128, this build uses 256"):
            opt.check_checkpoint_meta(dict(mine, optimizer_block_size=128), "ck")


def _tensors(path):
    from safetensors.torch import load_file
    return load_file(path)


@pytest.mark.parametrize("kind", ["adamw", "adamw8bit"])
def test_checkpoints_written_before_the_optimizer_object_load_and_come_back_the_same(kind, tmp_path):
    """``tests/golden/checkpoint_adamw`` and ``tests/golden/checkpoint_adamw8bit`` were written by ``train_state.save_state`` of commit
    be7f237 ("Training: batches of clips per step"), the last one whose ``ParamStore`` held the moments: the state dict above, moments
    / codes / absmax filled from ``torch.Generator().manual_seed(1)``, 7 optimizer steps, 2 skipped, loss scale 32768, growth
    counter 5.  Today's ``load_state`` reads them and today's ``save_state`` writes the same files: every tensor equal in key, dtype,
    shape and bytes, ``trainer_state.json`` equal as a dict."""
    from posetraj_amd import train_state as TS
    from posetraj_amd.autodiff import ParamStore
    src, out = os.path.join(GOLDEN, f"checkpoint_{kind}"), str(tmp_path / "again")
    P = ParamStore({k: torch.zeros_like(v) for k, v in _sd().items()}, "cpu")
    t = types.SimpleNamespace(params=P, optimizer=_optimizer(kind, P), config={"in_channels": 5}, optimizer_steps=0, skipped_steps=0,
                              loss_scale=65536.0, _clean=0, growth_interval=2000, _micro=0, _accum_scale=None, accumulation=1,
                              lr=HYPER["lr"], betas=HYPER["betas"], weight_decay=HYPER["weight_decay"], eps=HYPER["eps"])
    TS.load_state(t, src)
    assert (t.optimizer_steps, t.skipped_steps, t.loss_scale, t._clean) == (7, 2, 32768.0, 5)
    assert all(torch.equal(P.value(k), v) for k, v in _sd().items())
    TS.save_state(t, out)
    found = sorted(os.path.relpath(os.path.join(d, f), out) for d, _, files in os.walk(out) for f in files)
    assert found == sorted(os.path.relpath(os.path.join(d, f), src) for d, _, files in os.walk(src) for f in files)
    for rel in ("optimizer.safetensors", os.path.join("controlnet", "diffusion_pytorch_model.safetensors")):
        a, b = _tensors(os.path.join(src, rel)), _tensors(os.path.join(out, rel))
        assert list(a) and set(a) == set(b), rel
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (rel, k)
            assert torch.equal(a[k].contiguous().reshape(-1).view(torch.uint8), b[k].contiguous().reshape(-1).view(torch.uint8)), (rel, k)
    for rel in ("trainer_state.json", os.path.join("controlnet", "config.json")):
        assert json.load(open(os.path.join(src, rel))) == json.load(open(os.path.join(out, rel))), rel
    state = json.load(open(os.path.join(out, "trainer_state.json")))
    assert ("optimizer" in state, "optimizer_block_size" in state) == ((True, True) if kind == "adamw8bit" else (False, False))
