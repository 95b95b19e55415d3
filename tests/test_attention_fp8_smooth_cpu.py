"""CPU-side checks of the smooth-K fp8 attention: the two entry points exist in the library, the header and the ctypes table with
the argument lists of their plain counterparts, the workspace size covers the means, the ABI version did not move, the Python
switches exist and default to off, and the seeded inputs of the GPU test's offset-key case do cost the plain quantiser at least
2 x the smoothed one (torch emulation, tests/attn_fp8_ref.py)."""
import inspect
import os
import re

import pytest
import torch

from frameino_amd import _lib
from tests.attn_fp8_ref import OFFSET_SHAPES, emulated, offset_inputs, sdpa
from tests.parity import rel_rms


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _header_args(name):
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/frameino_hip.h"
    return m.group(1), [" ".join(a.split()) for a in m.group(2).split(",")]


def test_the_new_symbols_are_in_the_library_the_header_and_the_ctypes_table(lib):
    for new, old in (("fino_attn_fp8_smooth_kv_bytes", "fino_attn_fp8_kv_bytes"), ("fino_attn_fwd_fp8_smooth", "fino_attn_fwd_fp8")):
        assert hasattr(lib, new) and new in _lib.declared_symbols()
        assert _header_args(new) == _header_args(old)                      # return type and argument list of the plain entry
        assert _lib.SIGNATURES[new] == _lib.SIGNATURES[old]
        assert getattr(lib, new).restype == getattr(lib, old).restype
    assert _header_args("fino_attn_fp8_smooth_kv_bytes") == ("int64_t", ["int batch", "int heads", "int64_t lk", "int head_dim"])
    assert len(_header_args("fino_attn_fwd_fp8_smooth")[1]) == 23


def test_the_abi_version_did_not_move(lib):
    assert lib.fino_version() == 103 == _lib.ABI_VERSION


@pytest.mark.parametrize("b,heads,lk,dh", [(1, 1, 1, 64), (1, 2, 65, 64), (2, 48, 19126, 64), (2, 24, 12320, 128), (3, 5, 257, 128)])
def test_the_workspace_covers_the_plain_layout_and_the_means(lib, b, heads, lk, dh):
    plain, smooth = lib.fino_attn_fp8_kv_bytes(b, heads, lk, dh), lib.fino_attn_fp8_smooth_kv_bytes(b, heads, lk, dh)
    assert plain > 0 and smooth >= plain + 4 * b * heads * dh
    # ... and one fp32 partial per (batch element, 256-key chunk, channel) behind them, from a 16-byte boundary
    assert smooth == (plain + 15) // 16 * 16 + 4 * b * heads * dh * (1 + (lk + 255) // 256)


def test_unsupported_arguments_size_to_zero_and_are_refused(lib):
    import ctypes
    assert lib.fino_attn_fp8_smooth_kv_bytes(1, 2, 100, 96) == 0
    assert lib.fino_attn_fp8_smooth_kv_bytes(0, 2, 100, 64) == 0 and lib.fino_attn_fp8_smooth_kv_bytes(1, 2, 0, 64) == 0
    f1 = ctypes.c_float(1.0)
    rc = lib.fino_attn_fwd_fp8_smooth(16, 16, 16, 16, 1, 1, 8, 8, 96, *([64] * 8), f1, 0, 0, 16, 1 << 20, 0)
    assert rc == -3 and b"fino_attn_fwd_fp8_smooth: head_dim" in lib.fino_last_error()
    # a workspace sized for the plain call is too small for the smoothed one: refused before any launch
    plain = lib.fino_attn_fp8_kv_bytes(1, 1, 64, 64)
    rc = lib.fino_attn_fwd_fp8_smooth(16, 16, 16, 16, 1, 1, 8, 64, 64, *([64] * 8), f1, 0, 0, 16, plain, 0)
    assert rc == -1 and b"workspace" in lib.fino_last_error()


def test_the_python_switches_exist_and_default_to_off():
    from frameino_amd import ops
    from frameino_amd.cogvideox_transformer_3d import CogVideoXTransformer3DModel
    from frameino_amd.transformer_wan import WanTransformer3DModel
    for fn in (ops.attention_fp8, WanTransformer3DModel.enable_fp8_attention, CogVideoXTransformer3DModel.enable_fp8_attention):
        assert inspect.signature(fn).parameters["smooth_k"].default is False, fn


@pytest.mark.parametrize("b,heads,lq,lk", OFFSET_SHAPES)
@pytest.mark.parametrize("dh", [64, 128])
def test_the_offset_keys_cost_the_plain_emulation_twice_the_smoothed_one(b, heads, lq, lk, dh):
    """the condition the GPU test asserts on the same seeded inputs (K = N(0, 1) + 8 N(0, 1) per channel)"""
    heads = heads if dh == 64 else max(1, heads // 2)
    for dtype in (torch.bfloat16, torch.float16):
        q, k, v = offset_inputs(b, heads, lq, lk, dh, dtype)
        ref = sdpa(q, k, v, heads)
        for p_mode in ("exp2", "ramp"):
            plain, smooth = rel_rms(emulated(q, k, v, heads, p_mode), ref), rel_rms(emulated(q, k, v, heads, p_mode, smooth_k=True), ref)
            assert plain >= 2 * smooth and smooth < 8e-2, (p_mode, dtype, plain, smooth)
