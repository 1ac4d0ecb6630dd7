"""Temporal attention for clips of 33 - 128 frames on the host: the binding of include/posetraj_temporal.h's entry point and the
refusals that need no launch.  No kernel runs here (tests/test_temporal_attn_long_gpu.py)."""
import ctypes

import pytest

@pytest.fixture(scope="module")
def hip():
    from posetraj_amd import hip
    hip.build()
    return hip


def test_the_long_entry_point_has_the_short_ones_signature(hip):
    """(The header's contract with the library: tests/test_abi_cpu.py.)"""
    assert hip.ABIS["temporal"].prototypes["ptt_attn_temporal_bwd_long_f16"] == hip.PROTOTYPES["pt_attn_temporal_bwd_f16"]


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
