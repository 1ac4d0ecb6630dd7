"""Temporal attention for clips of 33 - 128 frames on the host: the extension header include/posetraj_temporal.h and its binding, and the
refusals that need no launch.  No kernel runs here (tests/test_temporal_attn_long_gpu.py)."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest

ENTRIES = {"ptt_abi_version", "ptt_attn_temporal_bwd_long_f16"}


@pytest.fixture(scope="module")
def hip():
    from posetraj_amd import hip
    hip.build()
    return hip


def test_extension_header_binding_and_symbols(hip, tmp_path):
    """The header the way tests/test_deterministic_cpu.py treats include/posetraj_det.h: a C++ compiler confirms the prototypes the parser
    read, the library defines every declared ``ptt_`` symbol and no other, the new entry point has the old one's signature."""
    assert hip.TEMPORAL_ABI_VERSION == 1 and set(hip.TEMPORAL_SIGNATURES) == ENTRIES
    assert not set(hip.TEMPORAL_SIGNATURES) & (set(hip.SIGNATURES) | set(hip.OPTIM_SIGNATURES) | set(hip.DET_SIGNATURES))
    hdr = re.sub(r"/\*.*?\*/", " ", open(hip.TEMPORAL_HEADER).read(), flags=re.S)
    assert set(re.findall(r"\b(ptt_[a-z0-9_]+)\s*\(", hdr)) == ENTRIES
    assert hip.TEMPORAL_PROTOTYPES["ptt_attn_temporal_bwd_long_f16"] == hip.PROTOTYPES["pt_attn_temporal_bwd_f16"]
    tu = ["#include <type_traits>", '#include "posetraj_temporal.h"']
    for fn, (ret, params) in hip.TEMPORAL_PROTOTYPES.items():
        tu.append(f"static_assert(std::is_same_v<decltype(&{fn}), {ret} (*)({', '.join(params) or 'void'})>, \"{fn}\");")
    tu.append(f"static_assert(PT_TEMPORAL_ABI_VERSION == {hip.TEMPORAL_ABI_VERSION} && PT_ABI_VERSION == {hip.ABI_VERSION}, \"versions\");")
    src = tmp_path / "temporal_abi_probe.cpp"
    src.write_text("\n".join(tu) + "\n")
    cxx = shutil.which("c++") or shutil.which("clang++") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", os.path.dirname(hip.TEMPORAL_HEADER), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    out = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("ptt_")}
    assert defined == ENTRIES, defined ^ ENTRIES
    L, C = hip.lib(), hip.checked()
    assert L.ptt_abi_version() == C.ptt_abi_version() == 1
    assert C.ptt_attn_temporal_bwd_long_f16.errcheck is hip._raise_on_status and not C.ptt_abi_version.errcheck
    assert not L.ptt_attn_temporal_bwd_long_f16.errcheck
    # the header feeds the rebuild check and the build's digest
    assert "TEMPORAL_HEADER" in inspect.getsource(hip.build) and "TEMPORAL_HEADER" in inspect.getsource(hip.source_digest)


def test_refusals_on_the_host(hip):
    """Frame counts and head sizes outside the ranges: non-zero status and the stated message, before any launch (no device is needed
    for this to return)."""
    L = hip.lib()
    buf = (ctypes.c_float * 4096)()                           # host memory: only ever compared against NULL and for alignment
    a = (ctypes.addressof(buf) + 15) & ~15
    hd = 64

    def forward(Fr):
        return L.pt_attn_temporal_f16(a, 3 * hd, hd, 2 * hd, a, hd, 1, Fr, 1, 1, hd, hd ** -0.5, None)

    def backward(fn, Fr, head_dim=hd):
        return fn(a, 3 * head_dim, head_dim, 2 * head_dim, a, head_dim, a, 3 * head_dim, 1, Fr, 1, 1, head_dim, head_dim ** -0.5, None)

    for Fr in (129, 0):
        assert forward(Fr) != 0
        msg = L.pt_last_error().decode()
        assert "pt_attn_temporal_f16" in msg and "1..128" in msg and f"{Fr} frames" in msg, msg
    for Fr in (32, 129):
        assert backward(L.ptt_attn_temporal_bwd_long_f16, Fr) != 0
        msg = L.pt_last_error().decode()
        assert "ptt_attn_temporal_bwd_long_f16" in msg and "33..128" in msg and f"{Fr} frames" in msg, msg
    assert backward(L.ptt_attn_temporal_bwd_long_f16, 40, head_dim=80) != 0
    assert "head_dim 80" in L.pt_last_error().decode()
    assert L.ptt_attn_temporal_bwd_long_f16(None, 3 * hd, hd, 2 * hd, None, hd, None, 3 * hd, 1, 40, 1, 1, hd, hd ** -0.5, None) != 0
    assert "null pointer" in L.pt_last_error().decode()
    assert backward(L.pt_attn_temporal_bwd_f16, 33) != 0
    msg = L.pt_last_error().decode()
    assert "1..32" in msg and "33 frames" in msg, msg
    with pytest.raises(RuntimeError, match="33..128"):
        backward(hip.checked().ptt_attn_temporal_bwd_long_f16, 32)
