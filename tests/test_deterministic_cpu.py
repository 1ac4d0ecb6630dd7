"""``ControlNetTrainer(deterministic=True)`` on the host: the bindings of include/posetraj_det.h the product relies on, the product's
call sites, the refusals that need no launch.  No kernel runs here (tests/test_deterministic_gpu.py)."""
import ast
import ctypes
import inspect
import os

import pytest

@pytest.fixture(scope="module")
def hip():
    from posetraj_amd import hip
    hip.build()
    return hip


def test_bindings_of_the_gemm_entries(hip):
    """ctypes: the gemm entries take the main header's struct; sizes come back as 64-bit integers.  (The header's contract with the
    library: tests/test_abi_cpu.py.)  The fold's source feeds the rebuild check and the build's digest."""
    sigs = hip.ABIS["det"].signatures
    assert sigs["ptd_gemm_f16"][1][0] == ctypes.POINTER(hip.GemmParams) and sigs["ptd_gemm_ws_floats"][0] is ctypes.c_int64
    assert "pt_fold.h" in hip.HEADERS


def test_size_queries(hip):
    """The documented formulas, at the shapes the GPU tests use."""
    L = hip.lib()
    assert L.ptd_colsum_ws_floats(256, 1, 64) == 4 * 64 and L.ptd_colsum_ws_floats(256, 3, 100) == 4 * 3 * 100
    assert L.ptd_groupnorm_bwd_ws_floats(320, 32, 256, 1, 1) == 4 * (2 * 32 * 2 + 2 * 320) and L.ptd_groupnorm_bwd_ws_floats(320, 32, 256, 1, 0) == 4 * 2 * 32 * 2
    assert L.ptd_layernorm_bwd_ws_floats(1000, 320) == 16 * 2 * 320 and L.ptd_layernorm_bwd_ws_floats(1000, 1280) == 125 * 2 * 1280
    assert L.ptd_dot_diff_ws_floats(65536) == 256 and L.ptd_sumsq_ws_floats(1_000_003) == 2 * 2048
    p = hip.GemmParams()
    p.M, p.N, p.K, p.sc_m, p.sc_n, p.nb0, p.nb1, p.nb2, p.bc2, p.splits = 32, 32, 1100, 32, 1, 1, 1, 9, 1024, 4
    assert L.ptd_gemm_ws_floats(ctypes.byref(p)) == 4 * 9 * 32 * 32
    p.splits = 1
    assert L.ptd_gemm_ws_floats(ctypes.byref(p)) == 0
    p.splits, p.sc_m = 4, 40                                  # rows 40 apart: C no longer covers one dense block
    assert L.ptd_gemm_ws_floats(ctypes.byref(p)) == 0


def test_refusals_on_the_host(hip):
    """Null pointers or a short workspace: non-zero status, no launch (no device is needed for this to return), the entry point named
    in pt_last_error()."""
    L = hip.lib()
    buf = (ctypes.c_float * 4096)()                           # host memory: only ever compared against NULL and for alignment
    a = ctypes.addressof(buf)

    def refused(name, rc):
        assert rc != 0 and name.encode() in L.pt_last_error(), (name, rc, L.pt_last_error())

    refused("ptd_groupnorm_bwd", L.ptd_groupnorm_bwd(None, None, 64, 0, 32, 256, 1, 1e-5, None, None, 1, None, None, None, None, None, None, None, 0, None))
    refused("ptd_groupnorm_bwd", L.ptd_groupnorm_bwd(a, None, 64, 0, 32, 256, 1, 1e-5, a, a, 1, a, a, None, a, a, a, None, 0, None))
    refused("ptd_groupnorm_bwd", L.ptd_groupnorm_bwd(a, None, 64, 0, 32, 256, 1, 1e-5, a, a, 1, a, a, None, a, a, a, a, L.ptd_groupnorm_bwd_ws_floats(64, 32, 256, 1, 1) - 1, None))
    assert b"workspace" in L.pt_last_error()
    refused("ptd_layernorm_bwd", L.ptd_layernorm_bwd(None, 1000, 320, None, 1e-5, None, None, None, None, None, None, 0, None))
    refused("ptd_layernorm_bwd", L.ptd_layernorm_bwd(a, 1000, 320, a, 1e-5, a, a, a, a, a, a, L.ptd_layernorm_bwd_ws_floats(1000, 320) - 1, None))
    refused("ptd_layernorm_bwd", L.ptd_layernorm_bwd(a, 1000, 1280, a, 1e-5, a, a, a, a, a, None, 1 << 30, None))
    refused("ptd_colsum_f16", L.ptd_colsum_f16(None, 256, 1, 64, 64, None, None, 0, None))
    refused("ptd_colsum_f16", L.ptd_colsum_f16(a, 256, 1, 64, 64, a, a, 255, None))
    refused("ptd_dot_diff", L.ptd_dot_diff(None, None, None, 65536, 1.0, None, None, 0, None))
    refused("ptd_dot_diff", L.ptd_dot_diff(a, a, a, 65536, 1.0, a, a, 255, None))
    refused("ptd_dot_diff_dev", L.ptd_dot_diff_dev(a, a, a, 65536, None, a, a, 256, None))
    refused("ptd_dot_diff_dev", L.ptd_dot_diff_dev(a, a, a, 65536, a, a, a, 255, None))
    refused("ptd_sumsq_f32", L.ptd_sumsq_f32(None, 1000, None, None, 0, None))
    refused("ptd_sumsq_f32", L.ptd_sumsq_f32(a, 1_000_003, a, a, 4095, None))
    refused("ptd_sumsq_f32", L.ptd_sumsq_f32(a, 1_000_003, a, a + 4, 4096, None))             # the doubles' alignment
    p = hip.GemmParams()
    refused("ptd_gemm_f16", L.ptd_gemm_f16(ctypes.byref(p), None, 0, None))
    p.A = p.B = p.C = a
    p.M, p.N, p.K, p.sa_m, p.sa_k, p.sb_k, p.sb_n, p.sc_m, p.sc_n, p.nb0, p.nb1, p.nb2, p.alpha, p.splits = 32, 32, 2048, 1, 32, 32, 1, 32, 1, 1, 1, 1, 1.0, 4
    p.out_mode = 1
    refused("ptd_gemm_f16", L.ptd_gemm_f16(ctypes.byref(p), a, 4096, None))                    # a plain store is not this entry's business
    p.out_mode = 2
    refused("ptd_gemm_f16", L.ptd_gemm_f16(ctypes.byref(p), None, 4096, None))
    refused("ptd_gemm_f16", L.ptd_gemm_f16(ctypes.byref(p), a, 4 * 32 * 32 - 1, None))
    assert b"workspace" in L.pt_last_error()
    p.sc_m = 40
    refused("ptd_gemm_f16", L.ptd_gemm_f16(ctypes.byref(p), a, 1 << 20, None))
    assert b"dense" in L.pt_last_error()
    with pytest.raises(RuntimeError, match="ptd_colsum_f16"):                                 # ... and through checked() they raise
        hip.checked().ptd_colsum_f16(None, 256, 1, 64, 64, None, None, 0, None)


def test_product_call_sites_pass_as_many_arguments_as_declared(hip):
    """Every ``ptd_`` call in the package: positional arguments only, none starred, as many as the header declares - and every status-
    returning entry point has a call site (autodiff.py: the five reductions of the reverse pass; training.py: the gradient norm)."""
    pkg = os.path.dirname(hip.__file__)
    sigs = hip.ABIS["det"].signatures
    called = set(sigs) - {"ptd_abi_version"}
    sites = {}
    for f in sorted(os.listdir(pkg)):
        if f.endswith(".py"):
            for node in ast.walk(ast.parse(open(os.path.join(pkg, f)).read())):
                if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in called:
                    assert not node.keywords and not any(isinstance(a, ast.Starred) for a in node.args), (f, node.lineno)
                    assert len(node.args) == len(sigs[node.func.attr][1]), (f, node.lineno, node.func.attr)
                    sites.setdefault(node.func.attr, []).append(f)
    assert set(sites) == called and len(called) == 13, called - set(sites)
    assert all(len(v) == 1 for v in sites.values()), sites
    assert sites["ptd_sumsq_f32"] == ["training.py"] and all(v == ["autodiff.py"] for k, v in sites.items() if "sumsq" not in k)


def test_trainer_keyword_without_a_device():
    """``deterministic=True, use_graph=True`` is refused before anything touches a device; the store's flag defaults to off and a
    checkpoint's metadata does not mention the mode."""
    import types
    import torch
    from posetraj_amd import autodiff as AD, train_state
    from posetraj_amd.training import ControlNetTrainer
    unet = types.SimpleNamespace(device=torch.device("cpu"))
    with pytest.raises(ValueError, match="deterministic"):
        ControlNetTrainer({}, {}, unet, deterministic=True, use_graph=True)
    assert inspect.signature(ControlNetTrainer.__init__).parameters["deterministic"].default is False
    assert AD.DETERMINISTIC is False and AD.ParamStore({"w": torch.zeros(4, 4)}, "cpu").deterministic is False
    assert "deterministic" not in inspect.getsource(train_state)
    assert "deterministic" in ControlNetTrainer.__doc__ and "all-reduce" in ControlNetTrainer.__doc__
