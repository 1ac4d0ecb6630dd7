"""``--use_ema`` on the host: the decay schedule of ``training_utils.EMAModel`` against a restatement of diffusers 0.24.0's formula,
its state dict over a CPU-resident ``ParamStore``, the ``controlnet_ema/`` folder of a checkpoint and the loader's two mixed cases,
and the two C entry points.  No kernel is launched here."""
import json
import os
import types

import pytest
import torch

EMA_KEYS = {"decay", "min_decay", "optimization_step", "update_after_step", "use_ema_warmup", "inv_gamma", "power"}


def restated_decay(k, decay=0.9999, min_decay=0.0, update_after_step=0, use_ema_warmup=False, inv_gamma=1.0, power=2 / 3):
    """diffusers 0.24.0 ``EMAModel.get_decay`` (restated from memory), Python doubles."""
    step = max(0, k - update_after_step - 1)
    if step <= 0:
        return 0.0
    d = 1 - (1 + step / inv_gamma) ** -power if use_ema_warmup else (1 + step) / (10 + step)
    return max(min(d, decay), min_decay)


def _sd():
    g = torch.Generator().manual_seed(0)
    return {"conv_in.weight": torch.randn(6, 5, 3, 3, generator=g), "conv_in.bias": torch.randn(6, generator=g),
            "mid.proj.weight": torch.randn(7, 6, generator=g), "mid.mix_factor": torch.tensor([0.25])}


def _trainer(use_ema, **ema_kw):
    """The attribute-less stand-in of tests/test_host_cpu.py, with or without an ``ema``."""
    from posetraj_amd import optim
    from posetraj_amd.autodiff import ParamStore
    from posetraj_amd.training_utils import EMAModel
    P = ParamStore(_sd(), "cpu")
    opt = optim.AdamW(P, lr=1e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    t = types.SimpleNamespace(params=P, optimizer=opt, config={"in_channels": 5, "_name_or_path": "x"}, optimizer_steps=0, skipped_steps=0, loss_scale=65536.0,
                              _clean=0, growth_interval=2000, _micro=0, _accum_scale=None, lr=1e-5, betas=(0.9, 0.999), weight_decay=1e-2,
                              eps=1e-8, accumulation=2)
    if use_ema:
        t.ema = EMAModel(P, model_config=t.config, **ema_kw)
    return t


@pytest.mark.parametrize("kw", [dict(), dict(use_ema_warmup=True), dict(use_ema_warmup=True, inv_gamma=2.0, power=0.75, decay=0.999),
                                dict(update_after_step=5), dict(update_after_step=3, use_ema_warmup=True, min_decay=0.3),
                                dict(min_decay=0.5), dict(decay=0.9)])
def test_get_decay_follows_the_restated_schedule(kw):
    from posetraj_amd.autodiff import ParamStore
    from posetraj_amd.training_utils import EMAModel
    ema = EMAModel(ParamStore(_sd(), "cpu"), **kw)
    for k in list(range(21)) + [100, 1000, 12345, 10 ** 6, 10 ** 9]:
        assert ema.get_decay(k) == restated_decay(k, **kw), (kw, k)
    # the first step's decay is 0 (the shadow becomes the parameters), and so is every step's up to update_after_step + 1: min_decay
    # does not lift those; from there the decay is at least min_decay and ends at `decay`
    uas = kw.get("update_after_step", 0)
    assert all(ema.get_decay(k) == 0.0 for k in range(uas + 2))
    assert all(kw.get("min_decay", 0.0) <= ema.get_decay(k) <= kw.get("decay", 0.9999) and ema.get_decay(k) > 0.0 for k in range(uas + 2, uas + 40))
    assert ema.get_decay(10 ** 9) == kw.get("decay", 0.9999)
    assert ema.optimization_step == 0 and ema.cur_decay_value is None
    omd = ema.begin_step()
    assert ema.optimization_step == 1 and ema.cur_decay_value == restated_decay(1, **kw) and omd == 1.0 - ema.cur_decay_value


def test_defaults_and_attributes_are_diffusers():
    from posetraj_amd.autodiff import ParamStore
    from posetraj_amd.training_utils import EMAModel
    P = ParamStore(_sd(), "cpu")
    ema = EMAModel(P)
    assert (ema.decay, ema.min_decay, ema.update_after_step, ema.use_ema_warmup, ema.inv_gamma, ema.power) == (0.9999, 0.0, 0, False, 1.0, 2 / 3)
    assert torch.equal(ema.shadow, P.flat) and ema.shadow.data_ptr() != P.flat.data_ptr()         # a clone at construction
    assert set(ema.scalars()) == EMA_KEYS


def test_state_dict_round_trip_over_a_cpu_store():
    """The shadow travels by parameter name in torch's layout: a conv weight (tap-major in the store), a matrix, a vector, a scalar."""
    from posetraj_amd.autodiff import ParamStore
    from posetraj_amd.training_utils import EMAModel
    sd = _sd()
    a = EMAModel(ParamStore(sd, "cpu"), decay=0.99, update_after_step=2, use_ema_warmup=True, inv_gamma=3.0, power=0.5, min_decay=0.1)
    a.shadow.mul_(1.5)
    a.optimization_step = 41
    st = a.state_dict()
    assert set(st) == EMA_KEYS | {"shadow_params"} and set(st["shadow_params"]) == set(sd)
    for k, v in sd.items():
        got = st["shadow_params"][k]
        assert got.shape == v.shape and got.is_contiguous() and torch.equal(got, v * 1.5)
    raw = a.params.raw(a.shadow, "conv_in.weight").view(9, 6, 5)                                     # the buffer itself is tap-major
    assert torch.equal(raw[5], sd["conv_in.weight"][:, :, 1, 2] * 1.5)
    b = EMAModel(ParamStore(sd, "cpu"))
    b.load_state_dict(st)
    assert b.scalars() == a.scalars() and b.optimization_step == 41
    for k in sd:                                                  # padding between parameters is not part of the state
        assert torch.equal(a.params.raw(a.shadow, k), b.params.raw(b.shadow, k))
    assert torch.equal(b.params.flat, ParamStore(sd, "cpu").flat)                                  # the parameters themselves are untouched
    with pytest.raises(KeyError):
        b.load_state_dict(dict(st, shadow_params={k: v for k, v in st["shadow_params"].items() if k != "conv_in.bias"}))
    with pytest.raises(ValueError):
        b.load_state_dict(dict(st, decay=1.5))
    with pytest.raises(ValueError):
        b.load_state_dict(dict(st, optimization_step=1.0))


def test_copy_to_store_restore_on_the_host_buffers():
    from posetraj_amd.autodiff import ParamStore
    from posetraj_amd.training_utils import EMAModel
    sd = _sd()
    P = ParamStore(sd, "cpu")
    ema = EMAModel(P)
    ema.shadow.mul_(2.0)
    with pytest.raises(RuntimeError, match="store"):
        ema.restore()
    master, v0 = P.flat.clone(), P.version
    ema.store()
    ema.copy_to()
    assert torch.equal(P.flat, ema.shadow) and P.version > v0
    assert torch.equal(P.half_view("conv_in.bias"), (2 * sd["conv_in.bias"]).half())               # the fp16 mirror followed
    v1 = P.version
    ema.restore()
    assert torch.equal(P.flat, master) and P.version > v1 and ema.temp_stored is None
    assert torch.equal(P.half_view("conv_in.bias"), sd["conv_in.bias"].half())


def test_checkpoint_file_set_with_and_without_ema(tmp_path):
    from safetensors.torch import load_file
    from posetraj_amd import ControlNetSDVModel, train_state as TS
    from posetraj_amd.modeling import EMA_CONFIG_KEYS
    from posetraj_amd.training_utils import EMAModel
    assert set(EMA_CONFIG_KEYS) == EMA_KEYS
    off = _trainer(False)
    ck_off = str(tmp_path / "off" / "checkpoint-1")
    TS.save_state(off, ck_off)
    assert sorted(os.listdir(ck_off)) == ["controlnet", "optimizer.safetensors", "trainer_state.json"]
    assert "ema" not in json.load(open(os.path.join(ck_off, "trainer_state.json")))
    assert json.load(open(os.path.join(ck_off, "controlnet", "config.json"))) == {"in_channels": 5, "_class_name": "ControlNetSDVModel"}
    on = _trainer(True, decay=0.999, use_ema_warmup=True, power=0.75)
    on.ema.shadow.mul_(0.5)
    on.ema.optimization_step, on.ema.cur_decay_value = 7, on.ema.get_decay(7)
    ck_on = str(tmp_path / "on" / "checkpoint-7")
    TS.save_state(on, ck_on)
    assert sorted(os.listdir(ck_on)) == ["controlnet", "controlnet_ema", "optimizer.safetensors", "trainer_state.json"]
    assert sorted(os.listdir(os.path.join(ck_on, "controlnet_ema"))) == ["config.json", "diffusion_pytorch_model.safetensors"]
    cfg = json.load(open(os.path.join(ck_on, "controlnet_ema", "config.json")))
    assert cfg == {"in_channels": 5, "_class_name": "ControlNetSDVModel", "decay": 0.999, "min_decay": 0.0, "optimization_step": 7,
                   "update_after_step": 0, "use_ema_warmup": True, "inv_gamma": 1.0, "power": 0.75}
    state = json.load(open(os.path.join(ck_on, "trainer_state.json")))
    assert state["format"] == 1 and {k: state["ema"][k] for k in EMA_KEYS} == on.ema.scalars() and state["ema"]["cur_decay_value"] == on.ema.cur_decay_value
    assert json.load(open(os.path.join(ck_on, "controlnet", "config.json"))) == {"in_channels": 5, "_class_name": "ControlNetSDVModel"}
    w = load_file(os.path.join(ck_on, "controlnet_ema", "diffusion_pytorch_model.safetensors"))
    sd = _sd()
    assert set(w) == set(sd) and all(torch.equal(w[k], sd[k] * 0.5) and w[k].is_contiguous() for k in sd)
    # the model class reads a config with the seven keys: they are no constructor arguments
    from oracle import nets as ON
    m = ControlNetSDVModel.from_config(dict(ON.tiny_config(), **on.ema.scalars(), _class_name="ControlNetSDVModel"))
    assert not (set(dict(m.config)) & EMA_KEYS) and dict(m.config) == dict(ControlNetSDVModel.from_config(ON.tiny_config()).config)
    with pytest.raises(TypeError):
        ControlNetSDVModel.from_config(dict(ON.tiny_config(), not_a_key=1))
    # EMAModel.from_pretrained over another trainer's store
    other = _trainer(False)
    e = EMAModel.from_pretrained(os.path.join(ck_on, "controlnet_ema"), other)
    assert e.scalars() == on.ema.scalars() and e.model_config == {"in_channels": 5}
    assert all(torch.equal(e.params.raw(e.shadow, k), on.params.raw(on.ema.shadow, k)) for k in sd)


def test_loader_with_and_without_the_ema_folder(tmp_path):
    from posetraj_amd import train_state as TS
    on = _trainer(True, decay=0.99, update_after_step=1)
    on.ema.shadow.add_(1.0)
    on.ema.optimization_step, on.ema.cur_decay_value = 12, on.ema.get_decay(12)
    on.optimizer_steps = 11
    ck_on, ck_off = str(tmp_path / "checkpoint-11"), str(tmp_path / "checkpoint-3")
    TS.save_state(on, ck_on)
    TS.save_state(_trainer(False), ck_off)
    # EMA on <- EMA on: shadow and counters (the constructor's decay / update_after_step are replaced by the stored ones, as in diffusers)
    b = _trainer(True)
    TS.load_state(b, ck_on)
    assert b.ema.scalars() == on.ema.scalars() and b.ema.cur_decay_value == on.ema.cur_decay_value and b.optimizer_steps == 11
    for k in _sd():
        assert torch.equal(b.params.raw(b.ema.shadow, k), on.params.raw(on.ema.shadow, k))
        assert torch.equal(b.params.raw(b.params.flat, k), on.params.raw(on.params.flat, k))
    # EMA on <- a checkpoint without the folder: an error that names it
    with pytest.raises(RuntimeError, match="controlnet_ema"):
        TS.load_state(_trainer(True), ck_off)
    # EMA off <- a checkpoint with the folder: ignored
    c = _trainer(False)
    state = TS.load_state(c, ck_on)
    assert not hasattr(c, "ema") and c.optimizer_steps == 11 and "ema" in state


def test_library_exports_the_ema_entry_points():
    import ctypes as C
    from posetraj_amd import hip
    hip.build()
    lib = hip.lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "posetraj_hip.h")).read()
    fused = hip.SIGNATURES["pt_adamw_fused_f32"]
    assert hip.SIGNATURES["pt_adamw_ema_f32"] == (C.c_int, fused[1][:-1] + [C.c_void_p, C.c_float, C.c_void_p])
    assert hip.SIGNATURES["pt_ema_update_f32"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p])
    for name in ("pt_adamw_ema_f32", "pt_ema_update_f32"):
        assert hasattr(lib, name) and f"int {name}(" in hdr
    # argument checks run before any launch: no device is needed to see them
    assert lib.pt_ema_update_f32(None, None, 8, 0.5, None) != 0 and b"pt_ema_update_f32" in lib.pt_last_error()
    assert lib.pt_ema_update_f32(16, 32, 6, 0.5, None) != 0 and b"multiple of 4" in lib.pt_last_error()
    assert lib.pt_ema_update_f32(16, 36, 8, 0.5, None) != 0 and b"16-byte aligned" in lib.pt_last_error()
    assert lib.pt_adamw_ema_f32(16, 32, 48, 64, 8, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1, 1.0, None, 0, None, 0.5, None) != 0
    assert b"ema_shadow" in lib.pt_last_error()
    assert lib.pt_adamw_ema_f32(16, 32, 48, 64, 8, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1, 1.0, None, 0, 84, 0.5, None) != 0
    assert b"pt_adamw_ema_f32: buffers must be 16-byte aligned" in lib.pt_last_error()
