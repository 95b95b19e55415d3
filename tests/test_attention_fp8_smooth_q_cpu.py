"""CPU-side checks of smooth Q in the fp8 attention (fino_attn_fwd_fp8_smooth_q): the new entry points and the flag bit exist in the
library, the header and the ctypes table; the ABI version did not move; the size function equals fino_attn_fp8_smoothed_kv_bytes
below bit 4 and adds the q-block means and the bias table behind it, each from a 16-byte boundary; unsupported arguments size to
zero and are refused, a workspace that is too small is refused before any launch, and the older entry points keep refusing bit 4;
the Python switches exist and default to off; window and sparse attention refuse it in either order on both models; both examples
take --smooth-q; and THE CONDITION of the GPU tests: on the seeded offset-query inputs the plain emulation's rel-RMS against fp32
SDPA is at least 2 x the smoothed emulation's (tests/attn_fp8_smooth_q_ref.py)."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from frameino_amd import _lib
from tests.attn_fp8_smooth_q_ref import CONDITION, CONDITION_SHAPES, SHAPES, emulated, heads_at, offset_q_inputs, sdpa
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


def test_the_new_symbols_and_the_flag_bit_are_in_the_library_the_header_and_the_ctypes_table(lib):
    for new in ("fino_attn_fp8_smooth_q_kv_bytes", "fino_attn_fwd_fp8_smooth_q"):
        assert hasattr(lib, new) and new in _lib.declared_symbols()
    # the forward: fino_attn_fwd_fp8's arguments, then the flag word -- the list of fino_attn_fwd_fp8_smoothed
    rt, args = _header_args("fino_attn_fwd_fp8_smooth_q")
    assert (rt, args) == _header_args("fino_attn_fwd_fp8_smoothed")
    assert args == _header_args("fino_attn_fwd_fp8")[1] + ["int smooth"] and len(args) == 24
    assert _lib.SIGNATURES["fino_attn_fwd_fp8_smooth_q"] == _lib.SIGNATURES["fino_attn_fwd_fp8"] + [ctypes.c_int]
    assert lib.fino_attn_fwd_fp8_smooth_q.restype == lib.fino_attn_fwd_fp8.restype
    # the size function: the smoothed one's arguments with lq in front of lk
    rt, args = _header_args("fino_attn_fp8_smooth_q_kv_bytes")
    assert rt == "int64_t" and args == ["int batch", "int heads", "int64_t lq", "int64_t lk", "int head_dim", "int smooth"]
    assert _lib.SIGNATURES["fino_attn_fp8_smooth_q_kv_bytes"] == [ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int64,
                                                                 ctypes.c_int, ctypes.c_int]
    assert lib.fino_attn_fp8_smooth_q_kv_bytes.restype == ctypes.c_int64
    text = _header()
    assert re.search(r"^#define\s+FINO_FP8_SMOOTH_Q\s+4\s*$", text, flags=re.M)
    assert re.search(r"^#define\s+FINO_FP8_SMOOTH_K\s+1\s*$", text, flags=re.M)
    assert re.search(r"^#define\s+FINO_FP8_SMOOTH_V\s+2\s*$", text, flags=re.M)


def test_the_abi_version_did_not_move(lib):
    assert lib.fino_version() == 103 == _lib.ABI_VERSION
    assert re.search(r"^#define\s+FINO_VERSION\s+103\s*$", _header(), flags=re.M)


SIZES = [(1, 1, 1, 1, 64), (1, 2, 33, 65, 64), (2, 48, 19126, 19126, 64), (2, 24, 12320, 12320, 128), (3, 5, 300, 257, 128),
         (1, 2, 0, 64, 64)]


@pytest.mark.parametrize("b,heads,lq,lk,dh", SIZES)
def test_below_bit_4_the_size_is_the_smoothed_size(lib, b, heads, lq, lk, dh):
    for flags in (0, 1, 2, 3):
        assert lib.fino_attn_fp8_smooth_q_kv_bytes(b, heads, lq, lk, dh, flags) == \
            lib.fino_attn_fp8_smoothed_kv_bytes(b, heads, lk, dh, flags) > 0


@pytest.mark.parametrize("b,heads,lq,lk,dh", SIZES)
def test_bit_4_adds_the_means_and_the_table_behind_everything_else_from_16_byte_boundaries(lib, b, heads, lq, lk, dh):
    nqb, nt = (lq + 255) // 256, (lk + 63) // 64
    for flags in (4, 5, 6, 7):
        base = lib.fino_attn_fp8_smoothed_kv_bytes(b, heads, lk, dh, flags & 3)
        means_at = (base + 15) // 16 * 16
        table_at = (means_at + 4 * b * nqb * heads * dh + 15) // 16 * 16
        assert lib.fino_attn_fp8_smooth_q_kv_bytes(b, heads, lq, lk, dh, flags) == table_at + 4 * b * heads * nqb * nt * 64


def test_unsupported_arguments_size_to_zero_and_are_refused(lib):
    for flags in range(8):
        assert lib.fino_attn_fp8_smooth_q_kv_bytes(1, 2, 100, 100, 96, flags) == 0
        assert lib.fino_attn_fp8_smooth_q_kv_bytes(0, 2, 100, 100, 64, flags) == 0
        assert lib.fino_attn_fp8_smooth_q_kv_bytes(1, 2, 100, 0, 64, flags) == 0
        assert lib.fino_attn_fp8_smooth_q_kv_bytes(1, 2, -1, 100, 64, flags) == 0
    assert lib.fino_attn_fp8_smooth_q_kv_bytes(1, 2, 100, 100, 64, 8) == 0
    assert lib.fino_attn_fp8_smooth_q_kv_bytes(1, 2, 100, 100, 64, -1) == 0
    f1 = ctypes.c_float(1.0)
    rc = lib.fino_attn_fwd_fp8_smooth_q(16, 16, 16, 16, 1, 1, 8, 8, 96, *([64] * 8), f1, 0, 0, 16, 1 << 20, 0, 4)
    assert rc == -3 and lib.fino_last_error().startswith(b"fino_attn_fwd_fp8_smooth_q: head_dim")
    for bad in (8, -1):
        rc = lib.fino_attn_fwd_fp8_smooth_q(16, 16, 16, 16, 1, 1, 8, 8, 64, *([64] * 8), f1, 0, 0, 16, 1 << 20, 0, bad)
        assert rc == -1 and lib.fino_last_error().startswith(b"fino_attn_fwd_fp8_smooth_q: smooth")


def test_a_workspace_that_is_too_small_is_refused_before_any_launch(lib):
    """(the pointers are not device memory: a launch would not return an argument error)"""
    f1 = ctypes.c_float(1.0)
    for dh in (64, 128):
        for flags in (4, 5, 6, 7):
            below = lib.fino_attn_fp8_smoothed_kv_bytes(1, 1, 64, dh, flags & 3)            # the size without Q's part
            need = lib.fino_attn_fp8_smooth_q_kv_bytes(1, 1, 8, 64, dh, flags)
            assert need > below
            for given in (below, need - 1):
                rc = lib.fino_attn_fwd_fp8_smooth_q(16, 16, 16, 16, 1, 1, 8, 64, dh, *([128] * 8), f1, 0, 0, 16, given, 0, flags)
                assert rc == -1 and lib.fino_last_error().startswith(b"fino_attn_fwd_fp8_smooth_q: workspace"), (dh, flags, given)
    # a workspace of exactly the size passes the size check and stops at lq = 0
    need = lib.fino_attn_fp8_smooth_q_kv_bytes(1, 1, 0, 64, 64, 7)
    assert lib.fino_attn_fwd_fp8_smooth_q(16, 16, 16, 16, 1, 1, 0, 64, 64, *([64] * 8), f1, 0, 0, 16, need, 0, 7) == 0


def test_the_older_entry_points_keep_refusing_bit_4(lib):
    f1 = ctypes.c_float(1.0)
    assert lib.fino_attn_fp8_smoothed_kv_bytes(1, 2, 100, 64, 4) == 0
    rc = lib.fino_attn_fwd_fp8_smoothed(16, 16, 16, 16, 1, 1, 8, 8, 64, *([64] * 8), f1, 0, 0, 16, 1 << 20, 0, 4)
    assert rc == -1 and b"fino_attn_fwd_fp8_smoothed: smooth flags 4 not in 0 .. 3" in lib.fino_last_error()
    rc = lib.fino_attn_fwd_fp8_tiles(16, 16, 16, 16, 1, 1, 8, 64, 128, *([128] * 8), f1, 0, 0, 16, 1 << 24, 4, 16, 0, 0, 1, 0)
    assert rc == -1 and b"smooth" in lib.fino_last_error()


def test_the_python_switches_exist_and_default_to_off():
    from frameino_amd import ops
    from frameino_amd.cogvideox_transformer_3d import CogVideoXTransformer3DModel
    from frameino_amd.transformer_wan import WanTransformer3DModel
    for fn in (ops.attention_fp8, WanTransformer3DModel.enable_fp8_attention, CogVideoXTransformer3DModel.enable_fp8_attention):
        assert inspect.signature(fn).parameters["smooth_q"].default is False, fn
    for fn in (ops.attention_fp8_ranges, ops.attention_fp8_tiles):          # the walks have no smooth Q
        assert "smooth_q" not in inspect.signature(fn).parameters, fn


def _tiny(which):
    if which == "wan":
        from frameino_amd.transformer_wan import WanTransformer3DModel
        return WanTransformer3DModel(num_attention_heads=2, attention_head_dim=128, in_channels=4, out_channels=4, text_dim=32,
                                     freq_dim=32, ffn_dim=64, num_layers=2)
    from frameino_amd.cogvideox_transformer_3d import CogVideoXTransformer3DModel
    from tests.cog_window_attn_ref import TINY_CFG
    return CogVideoXTransformer3DModel(**TINY_CFG)


@pytest.mark.parametrize("which", ["wan", "cog"])
def test_window_and_sparse_attention_refuse_smooth_q_in_either_order(which):
    from frameino_amd.window_attention import SparseAttentionConfig, WindowAttentionConfig
    window = WindowAttentionConfig(window_frames=1)
    # fp8 with smooth Q first, then the walk
    m = _tiny(which).enable_fp8_attention(smooth_q=True)
    assert m.fp8_attention and m.fp8_smooth_q is True
    with pytest.raises(NotImplementedError, match="smooth_q"):
        m.enable_window_attention(window)
    assert not m.is_window_attention_enabled
    # the walk first, then fp8 with smooth Q: refused, and the state stays what it was
    m = _tiny(which).enable_window_attention(window)
    with pytest.raises(NotImplementedError, match="smooth_q"):
        m.enable_fp8_attention(smooth_q=True)
    assert not m.fp8_attention and m.fp8_smooth_q is False
    if which == "wan":                   # (the sparse attention is the Wan model's)
        sparse = SparseAttentionConfig(cdf_threshold=0.9)
        m = _tiny(which).enable_fp8_attention(smooth_q=True)
        with pytest.raises(NotImplementedError, match="smooth_q"):
            m.enable_sparse_attention(sparse)
        assert not m.is_sparse_attention_enabled
        m = _tiny(which).enable_sparse_attention(sparse)
        with pytest.raises(NotImplementedError, match="smooth_q"):
            m.enable_fp8_attention(smooth_q=True)
        assert not m.fp8_attention
        m.enable_fp8_attention()                     # without smooth Q the combination is what it was
        assert m.fp8_attention and m.fp8_smooth_q is False
    # switching smooth Q off again lets the window in
    m = _tiny(which).enable_fp8_attention(smooth_q=True).enable_fp8_attention(smooth_q=False)
    assert m.fp8_smooth_q is False


def test_attend_passes_smooth_q_on_the_dense_route_only_and_only_when_it_is_on():
    """`_attend` with recording ops: without the switch the keyword is absent (the call every earlier version made); with it the dense
    fp8 call gets smooth_q=True; a walk reached with it is refused before anything is called"""
    from frameino_amd.window_attention import SelfAttentionOptionsMixin
    calls = []

    class Ops:
        def __getattr__(self, name):
            return lambda *a, **kw: calls.append((name, kw))

    m = SelfAttentionOptionsMixin()
    m._init_self_attention_options()
    m.fp8_attention = True
    m._attend(Ops(), None, None, None, 2, fp8=True)
    assert calls == [("attention_fp8", dict(p_mode=None, smooth_k=False, smooth_v=False))]
    m.fp8_smooth_q = True
    m._attend(Ops(), None, None, None, 2, fp8=True)
    assert calls[1] == ("attention_fp8", dict(p_mode=None, smooth_k=False, smooth_v=False, smooth_q=True))
    m._attend(Ops(), None, None, None, 2, fp8=False)
    assert calls[2] == ("attention", {})
    for walk in (dict(ranges=object()), dict(tiles=object())):
        with pytest.raises(NotImplementedError, match="smooth_q"):
            m._attend(Ops(), None, None, None, 2, fp8=True, **walk)
    assert len(calls) == 3


def test_the_examples_take_smooth_q_next_to_smooth_k_and_smooth_v():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name in os.listdir(os.path.join(root, "examples")):
        if name.endswith(".py"):
            text = open(os.path.join(root, "examples", name)).read()
            assert '"--smooth-k"' in text and '"--smooth-v"' in text and '"--smooth-q"' in text, name
            assert "smooth_q=a.smooth_q" in text, name


@pytest.mark.parametrize("b,heads,lq,lk", CONDITION_SHAPES)
@pytest.mark.parametrize("dh", [64, 128])
def test_the_condition_offset_queries_cost_the_plain_emulation_twice_the_smoothed_one(b, heads, lq, lk, dh):
    """the seeded inputs of the GPU test (q = N(0, 1) + 8 N(0, 1) per (256-row block, head, channel)), both p_modes, bf16 and fp16:
    plain emulation >= 2 x smoothed emulation, rel-RMS against fp32 SDPA (measured on these seeds: 2.88 .. 6.94).  smooth K alone does not help
    these inputs (printed, not asserted)."""
    heads = heads_at(heads, dh)
    for dtype in (torch.bfloat16, torch.float16):
        q, k, v = offset_q_inputs(b, heads, lq, lk, dh, dtype)
        ref = sdpa(q, k, v, heads)
        for p_mode in ("exp2", "ramp"):
            plain = rel_rms(emulated(q, k, v, heads, p_mode), ref)
            sk = rel_rms(emulated(q, k, v, heads, p_mode, smooth_k=True), ref)
            smooth = rel_rms(emulated(q, k, v, heads, p_mode, smooth_q=True), ref)
            print(f"dh {dh} {(b, heads, lq, lk)} {dtype} {p_mode}: plain {plain:.5f} smooth K {sk:.5f} smooth Q {smooth:.5f} "
                  f"ratio {plain / smooth:.2f}")
            assert plain >= CONDITION * smooth, (p_mode, dtype, plain, smooth)


def test_without_an_offset_the_two_emulations_are_close_and_the_one_hot_shape_takes_closeness_only():
    """N(0, 1) queries: the block mean is small and smoothing changes little; the (33, 65) shape of the GPU test is nearly one-hot,
    where both emulations measure the same (so it is excluded from the ratio above)"""
    b, heads, lq, lk = SHAPES[0]
    q, k, v = offset_q_inputs(b, heads, lq, lk, 64, torch.bfloat16, c=0.0)
    ref = sdpa(q, k, v, heads)
    plain, smooth = rel_rms(emulated(q, k, v, heads), ref), rel_rms(emulated(q, k, v, heads, smooth_q=True), ref)
    print(f"no offset: plain {plain:.5f} smooth Q {smooth:.5f}")
    assert 0.8 * plain <= smooth <= 1.2 * plain
    b, heads, lq, lk = SHAPES[2]
    q, k, v = offset_q_inputs(b, heads, lq, lk, 64, torch.bfloat16)
    ref = sdpa(q, k, v, heads)
    plain, smooth = rel_rms(emulated(q, k, v, heads), ref), rel_rms(emulated(q, k, v, heads, smooth_q=True), ref)
    print(f"(33, 65): plain {plain:.5f} smooth Q {smooth:.5f}")
    assert smooth <= 1.2 * plain
