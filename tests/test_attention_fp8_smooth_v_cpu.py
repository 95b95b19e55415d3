"""CPU-side checks of smooth V in the fp8 attention (fino_attn_fwd_fp8_smoothed): the new entry points and flag bits exist in the
library, the header and the ctypes table; the ABI version did not move; the flag-word size function equals the plain and smooth-K
sizes for flags 0 and 1 and adds V's mean and partials from a 16-byte boundary for flags 2 and 3; unsupported arguments size to
zero and are refused, a workspace that is too small is refused before any launch; the Python switches exist and default to off;
and the seeded inputs of the GPU test's offset-value case do cost the plain emulation what that test's condition asks
(tests/attn_fp8_smooth_v_ref.py; measured worst cases on these seeds: 1.53 in bf16, 3.41 in fp16)."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from frameino_amd import _lib
from tests.attn_fp8_smooth_v_ref import CONDITION, OFFSET_SHAPES, emulated, offset_v_inputs, plan_split, sdpa
from tests.parity import rel_rms


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _header():
    return open(_lib.HEADER_PATH).read()


def _header_args(name):
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/frameino_hip.h"
    return m.group(1), [" ".join(a.split()) for a in m.group(2).split(",")]


def test_the_new_symbols_are_in_the_library_the_header_and_the_ctypes_table(lib):
    for new, old, extra in (("fino_attn_fp8_smoothed_kv_bytes", "fino_attn_fp8_kv_bytes", "int smooth"),
                            ("fino_attn_fwd_fp8_smoothed", "fino_attn_fwd_fp8", "int smooth")):
        assert hasattr(lib, new) and new in _lib.declared_symbols()
        rt_new, args_new = _header_args(new)
        rt_old, args_old = _header_args(old)
        assert rt_new == rt_old and args_new == args_old + [extra]        # the plain entry's arguments, then the flag word
        assert _lib.SIGNATURES[new] == _lib.SIGNATURES[old] + [ctypes.c_int]
        assert getattr(lib, new).restype == getattr(lib, old).restype
    assert len(_header_args("fino_attn_fwd_fp8_smoothed")[1]) == 24
    text = _header()
    assert re.search(r"^#define\s+FINO_FP8_SMOOTH_K\s+1\s*$", text, flags=re.M)
    assert re.search(r"^#define\s+FINO_FP8_SMOOTH_V\s+2\s*$", text, flags=re.M)
    # the pinned entries kept their argument lists
    assert len(_header_args("fino_attn_fwd_fp8_smooth")[1]) == 23 and len(_header_args("fino_attn_fwd_fp8_ranges")[1]) == 25
    assert "int smooth_k" in _header_args("fino_attn_fwd_fp8_ranges")[1]


def test_the_abi_version_did_not_move(lib):
    assert lib.fino_version() == 103 == _lib.ABI_VERSION


SIZES = [(1, 1, 1, 64), (1, 2, 65, 64), (2, 48, 19126, 64), (2, 24, 12320, 128), (3, 5, 257, 128)]


@pytest.mark.parametrize("b,heads,lk,dh", SIZES)
def test_flags_0_and_1_are_the_plain_and_the_smooth_k_sizes(lib, b, heads, lk, dh):
    assert lib.fino_attn_fp8_smoothed_kv_bytes(b, heads, lk, dh, 0) == lib.fino_attn_fp8_kv_bytes(b, heads, lk, dh) > 0
    assert lib.fino_attn_fp8_smoothed_kv_bytes(b, heads, lk, dh, 1) == lib.fino_attn_fp8_smooth_kv_bytes(b, heads, lk, dh) > 0


@pytest.mark.parametrize("b,heads,lk,dh", SIZES)
def test_flags_2_and_3_add_the_value_mean_and_its_partials_from_a_16_byte_boundary(lib, b, heads, lk, dh):
    add = 4 * b * heads * dh * (1 + (lk + 255) // 256)
    for flags in (2, 3):
        base = lib.fino_attn_fp8_smoothed_kv_bytes(b, heads, lk, dh, flags & 1)
        assert lib.fino_attn_fp8_smoothed_kv_bytes(b, heads, lk, dh, flags) == (base + 15) // 16 * 16 + add


def test_unsupported_arguments_size_to_zero_and_are_refused(lib):
    for flags in (0, 1, 2, 3):
        assert lib.fino_attn_fp8_smoothed_kv_bytes(1, 2, 100, 96, flags) == 0
        assert lib.fino_attn_fp8_smoothed_kv_bytes(0, 2, 100, 64, flags) == 0
        assert lib.fino_attn_fp8_smoothed_kv_bytes(1, 2, 0, 64, flags) == 0
    assert lib.fino_attn_fp8_smoothed_kv_bytes(1, 2, 100, 64, 4) == 0 and lib.fino_attn_fp8_smoothed_kv_bytes(1, 2, 100, 64, -1) == 0
    f1 = ctypes.c_float(1.0)
    rc = lib.fino_attn_fwd_fp8_smoothed(16, 16, 16, 16, 1, 1, 8, 8, 96, *([64] * 8), f1, 0, 0, 16, 1 << 20, 0, 2)
    assert rc == -3 and b"fino_attn_fwd_fp8_smoothed: head_dim" in lib.fino_last_error()
    rc = lib.fino_attn_fwd_fp8_smoothed(16, 16, 16, 16, 1, 1, 8, 8, 64, *([64] * 8), f1, 0, 0, 16, 1 << 20, 0, 4)
    assert rc == -1 and b"smooth" in lib.fino_last_error()


def test_a_workspace_that_is_too_small_is_refused_before_any_launch(lib):
    """(the pointers are not device memory: a launch would not return an argument error)"""
    f1 = ctypes.c_float(1.0)
    for dh in (64, 128):
        for flags in (2, 3):
            below = lib.fino_attn_fp8_smoothed_kv_bytes(1, 1, 64, dh, flags & 1)          # the size without V's part
            need = lib.fino_attn_fp8_smoothed_kv_bytes(1, 1, 64, dh, flags)
            for given in (below, need - 1):
                rc = lib.fino_attn_fwd_fp8_smoothed(16, 16, 16, 16, 1, 1, 8, 64, dh, *([128] * 8), f1, 0, 0, 16, given, 0, flags)
                assert rc == -1 and b"workspace" in lib.fino_last_error(), (dh, flags, given)
    # the range walk takes 2 and 3 as the same flag word and checks against the same size
    for flags in (2, 3):
        given = lib.fino_attn_fp8_smoothed_kv_bytes(1, 1, 64, 64, flags) - 1
        rc = lib.fino_attn_fwd_fp8_ranges(16, 16, 16, 16, 1, 1, 8, 64, 64, *([64] * 8), f1, 0, 0, 16, given, flags, 16, 0)
        assert rc == -1 and b"workspace" in lib.fino_last_error()
    # ... while 1 keeps the smooth-K size (a workspace of exactly that size passes the size check and stops at lq = 0)
    given = lib.fino_attn_fp8_smooth_kv_bytes(1, 1, 64, 64)
    assert lib.fino_attn_fwd_fp8_ranges(16, 16, 16, 16, 1, 1, 0, 64, 64, *([64] * 8), f1, 0, 0, 16, given, 1, 16, 0) == 0
    assert lib.fino_attn_fwd_fp8_ranges(16, 16, 16, 16, 1, 1, 0, 64, 64, *([64] * 8), f1, 0, 0, 16, given, 3, 16, 0) == -1


def test_the_python_switches_exist_and_default_to_off():
    from frameino_amd import ops
    from frameino_amd.cogvideox_transformer_3d import CogVideoXTransformer3DModel
    from frameino_amd.transformer_wan import WanTransformer3DModel
    for fn in (ops.attention_fp8, ops.attention_fp8_ranges, WanTransformer3DModel.enable_fp8_attention,
               CogVideoXTransformer3DModel.enable_fp8_attention):
        assert inspect.signature(fn).parameters["smooth_v"].default is False, fn
        assert inspect.signature(fn).parameters["smooth_k"].default is False, fn


def test_the_examples_take_smooth_v_next_to_smooth_k():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name in os.listdir(os.path.join(root, "examples")):
        if name.endswith(".py"):
            text = open(os.path.join(root, "examples", name)).read()
            assert '"--smooth-k"' in text and '"--smooth-v"' in text, name


def test_the_tail_split_plan_gives_the_gpu_test_one_shape_of_each_kind():
    """tests/test_attention_fp8_smooth_v_gpu.py's head_dim 128 shapes on a 256-CU device: 16 key tiles split, 4 do not"""
    assert plan_split(2, 4, 1, 16, 256) == (0, 1, 2, 8)
    assert plan_split(2, 4, 1, 4, 256)[1] == 0


@pytest.mark.parametrize("b,heads,lq,lk", OFFSET_SHAPES)
@pytest.mark.parametrize("dh", [64, 128])
def test_the_offset_values_cost_the_plain_emulation_what_the_gpu_test_s_condition_asks(b, heads, lq, lk, dh):
    """the condition the GPU test asserts on the same seeded inputs (V = N(0, 1) + 8 N(0, 1) per (batch element, channel)),
    emulations rounded to the storage dtype: plain >= 3 x smoothed in fp16, >= 1.45 x in bf16"""
    heads = heads if dh == 64 else max(1, heads // 2)
    for dtype in (torch.bfloat16, torch.float16):
        q, k, v = offset_v_inputs(b, heads, lq, lk, dh, dtype)
        ref = sdpa(q, k, v, heads)
        for p_mode in ("exp2", "ramp"):
            plain = rel_rms(emulated(q, k, v, heads, p_mode), ref)
            smooth = rel_rms(emulated(q, k, v, heads, p_mode, smooth_v=True), ref)
            both = rel_rms(emulated(q, k, v, heads, p_mode, smooth_k=True, smooth_v=True), ref)
            print(f"dh {dh} {(b, heads, lq, lk)} {dtype} {p_mode}: plain {plain:.5f} smooth V {smooth:.5f} both {both:.5f}")
            assert plain >= CONDITION[dtype] * smooth, (p_mode, dtype, plain, smooth)
            assert plain >= CONDITION[dtype] * both, (p_mode, dtype, plain, both)
