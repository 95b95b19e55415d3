"""Block-sparse fp8 self-attention, everything that needs no GPU: the C ABI's surface and error paths
(fino_attn_fp8_tiles_supported, fino_attn_fwd_fp8_tiles), the refusals in both orders -- accepted at head_dim 128, refused at any
other -- the dispatch of `_attend(fp8=True, tiles=...)` with a recording stand-in for `ops`, and the calibration's refusal."""
import ctypes
import os
from types import SimpleNamespace

import pytest
import torch

from frameino_amd.window_attention import SparseAttentionConfig, WindowAttentionConfig

FINO_ERR_ARG, FINO_ERR_UNSUPPORTED = -1, -3


def _tiny_model(head_dim=128):
    from frameino_amd.transformer_wan import WanTransformer3DModel
    return WanTransformer3DModel(num_attention_heads=2, attention_head_dim=head_dim, in_channels=4, out_channels=4, text_dim=32,
                                 freq_dim=32, ffn_dim=64, num_layers=2)


def test_the_header_the_signatures_and_the_library_carry_the_entry_points():
    from frameino_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "frameino_hip.h")).read()
    lib = _lib.load()
    for n in ("fino_attn_fp8_tiles_supported", "fino_attn_fwd_fp8_tiles"):
        assert n + "(" in header and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert "#define FINO_VERSION 103" in header and lib.fino_version() == 103
    # fino_attn_fwd_fp8_smoothed's arguments (..., stream, smooth), then the four of the mask, the stream last as everywhere
    smoothed, tiles = _lib.SIGNATURES["fino_attn_fwd_fp8_smoothed"], _lib.SIGNATURES["fino_attn_fwd_fp8_tiles"]
    assert smoothed[-2:] == [ctypes.c_void_p, ctypes.c_int]
    mask_args = _lib.SIGNATURES["fino_attn_fwd_tiles"][-5:-1]
    assert mask_args == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int]
    assert tiles == smoothed[:-2] + [ctypes.c_int] + mask_args + [ctypes.c_void_p]
    assert _lib.SIGNATURES["fino_attn_fp8_tiles_supported"] == _lib.SIGNATURES["fino_attn_fp8_ranges_supported"]


def test_abi_support_and_error_paths_come_before_any_launch():
    from frameino_amd import _lib
    lib = _lib.load()
    sup = lib.fino_attn_fp8_tiles_supported
    assert sup(2, 24, 12320, 12320, 128) == 1 and sup(1, 1, 1, 1, 128) == 1 and sup(1, 2, 8, 65536, 128) == 1
    assert sup(2, 24, 12320, 12320, 64) == 0 and sup(1, 2, 8, 8, 96) == 0
    assert sup(1, 2, 8, 65537, 128) == 0 and sup(0, 2, 8, 8, 128) == 0 and sup(1, 2, 8, 0, 128) == 0     # 1025 key tiles; bad shapes
    f1 = ctypes.c_float(1.0)

    def call(lk, head_dim, mask, words):
        # q k v o | b heads lq lk dh | 8 strides | scale dtype p_mode | workspace bytes | smooth | mask bs hs words | stream
        return lib.fino_attn_fwd_fp8_tiles(16, 16, 16, 16, 1, 1, 8, lk, head_dim, *([8] * 8), f1, 0, 0, 16, 1 << 30, 0,
                                           mask, 0, 0, words, 0)
    assert call(8, 64, 16, 1) == FINO_ERR_UNSUPPORTED
    msg = lib.fino_last_error()
    assert b"fino_attn_fwd_fp8_tiles" in msg and b"head_dim 64" in msg and b"128 only" in msg
    assert call(8, 128, 0, 1) == FINO_ERR_ARG and b"null mask" in lib.fino_last_error()
    assert call(8, 128, 18, 1) == FINO_ERR_ARG and b"4-byte aligned" in lib.fino_last_error()
    assert call(64 * 33, 128, 16, 1) == FINO_ERR_ARG and b"mask words" in lib.fino_last_error()          # 33 tiles need 2 words
    assert call(8, 128, 16, 0) == FINO_ERR_ARG and b"mask words" in lib.fino_last_error()
    assert call(64 * 1025, 128, 16, 64) == FINO_ERR_UNSUPPORTED and b"key tiles" in lib.fino_last_error()


def test_sparse_and_fp8_are_accepted_in_both_orders_at_head_dim_128_only():
    cfg = SparseAttentionConfig(0.5)
    m = _tiny_model(128)
    assert m.enable_sparse_attention(cfg) is m
    assert m.enable_fp8_attention(p_mode="ramp", smooth_k=True, smooth_v=True) is m                  # sparse, then fp8
    assert m.fp8_attention and m.is_sparse_attention_enabled and (m.fp8_smooth_k, m.fp8_smooth_v) == (True, True)
    m.enable_fp8_attention(False)
    m.disable_sparse_attention()
    m.enable_fp8_attention()                                                                         # fp8, then sparse
    m.enable_sparse_attention(cfg)
    assert m.fp8_attention and m.is_sparse_attention_enabled
    m._sparse_refusals(True, True, None)                     # what the forward repeats before any launch: nothing to refuse
    # any other head_dim: both orders still refused, and a refused enable leaves the switch off
    for dh in (64, 96):
        m = _tiny_model(dh)
        m.enable_sparse_attention(cfg)
        with pytest.raises(NotImplementedError, match="fp8 attention.*head_dim 128 only"):
            m.enable_fp8_attention()
        assert m.fp8_attention is False
        m.disable_sparse_attention()
        m.enable_fp8_attention()
        with pytest.raises(NotImplementedError, match="fp8 attention.*head_dim 128 only"):
            m.enable_sparse_attention(cfg)
        assert not m.is_sparse_attention_enabled
        with pytest.raises(NotImplementedError, match="fp8 attention.*head_dim 128 only"):
            m._sparse_refusals(True, True, None)


def test_the_other_refusals_are_unchanged_with_fp8_on():
    from frameino_amd.step_cache import PyramidAttentionBroadcastConfig, TaylorSeerCacheConfig
    cfg = SparseAttentionConfig(0.5)
    pab = PyramidAttentionBroadcastConfig(spatial_attention_block_skip_range=2, current_timestep_callback=lambda: 500)
    m = _tiny_model(128)
    m.enable_fp8_attention()
    m.enable_sparse_attention(cfg)
    with pytest.raises(NotImplementedError, match="sparse attention"):                              # window attention, either order
        m.enable_window_attention(WindowAttentionConfig(1))
    assert not m.is_window_attention_enabled
    with pytest.raises(NotImplementedError, match="Pyramid Attention Broadcast"):
        m.enable_cache(pab)
    with pytest.raises(NotImplementedError, match="sparse attention"):
        m.enable_cache(TaylorSeerCacheConfig(cache_interval=3))
    m.disable_sparse_attention()
    m.enable_cache(pab)
    with pytest.raises(NotImplementedError, match="Pyramid Attention Broadcast"):
        m.enable_sparse_attention(cfg)
    m.disable_cache()
    m.enable_cache(TaylorSeerCacheConfig(cache_interval=3))
    with pytest.raises(NotImplementedError, match="TaylorSeer"):
        m.enable_sparse_attention(cfg)
    m.disable_cache()
    m.parallel = type("Shard", (), {"active": True})()
    with pytest.raises(NotImplementedError, match="token-sharded"):
        m.enable_sparse_attention(cfg)
    m.parallel = None
    m.enable_sparse_attention(cfg)
    assert m.fp8_attention and m.is_sparse_attention_enabled


class _Ops:
    """records which front end `_attend` picked, with what"""

    def __init__(self):
        self.calls = []

    def _rec(name):                                          # noqa: N805
        def f(self, *a, **kw):
            self.calls.append((name, a, kw))
            return name
        return f

    attention, attention_fp8 = _rec("attention"), _rec("attention_fp8")
    attention_tiles, attention_fp8_tiles = _rec("attention_tiles"), _rec("attention_fp8_tiles")
    attention_tile_plan = _rec("attention_tile_plan")


def test_attend_dispatches_the_fp8_tile_walk_and_keeps_the_bf16_route():
    m = _tiny_model(128)
    q, k, v = (torch.zeros(2, 600, 256) for _ in range(3))
    table, out = torch.zeros(3, 3, 2, dtype=torch.int32), torch.zeros(2, 600, 256)
    m.enable_sparse_attention(SparseAttentionConfig(0.5, keep_masks=True))
    sp = SimpleNamespace(keep=lambda q_rows: table, skip=frozenset({1}), cdf=0.5, words=1, lk=1100,
                         mask=torch.arange(64, dtype=torch.int32), workspace="ws", keep_masks=True)
    tiles = m._sparse_tiles(sp, 0, (0, 600))
    m.enable_fp8_attention(p_mode="exp2", smooth_k=True, smooth_v=True)
    o = _Ops()
    assert m._attend(o, q, k, v, 2, fp8=True, tiles=tiles, out=out, scale=-1.0) == "attention_fp8_tiles"
    (n0, a0, kw0), (n1, a1, kw1) = o.calls
    assert n0 == "attention_tile_plan" and a0[0] is q and a0[1] is k and a0[2:] == (2, 0.5)         # on the bf16 / fp16 q and k
    assert kw0["keep_ranges"] is table and kw0["scale"] == -1.0 and kw0["workspace"] == "ws"
    mask = kw0["out"]
    assert mask.shape == (2, 2, 3, 1) and mask.data_ptr() == sp.mask.data_ptr()                      # the one mask buffer's leading rows
    assert n1 == "attention_fp8_tiles" and a1[:4] == (q, k, v, 2) and a1[4] is mask
    assert kw1 == dict(out=out, scale=-1.0, p_mode="exp2", smooth_k=True, smooth_v=True)
    assert torch.equal(m.sparse_attention_masks[0], mask) and m._sparse_mask_keys[0] == 600          # keep_masks works as before
    # fp8 = False: exactly the calls of today, no fp8 keyword
    o = _Ops()
    assert m._attend(o, q, k, v, 2, fp8=False, tiles=tiles, out=out, scale=-1.0) == "attention_tiles"
    (n0, a0, kw0), (n1, a1, kw1) = o.calls
    assert n0 == "attention_tile_plan" and set(kw0) == {"keep_ranges", "scale", "out", "workspace"}
    assert n1 == "attention_tiles" and a1[:4] == (q, k, v, 2) and kw1 == dict(out=out, scale=-1.0)
    # the dense fall-backs (a skipped layer, forced tiles that cover everything) take ops.attention_fp8 with the model's options
    o = _Ops()
    assert m._sparse_tiles(sp, 1, (0, 600)) is None
    assert m._attend(o, q, k, v, 2, fp8=True, tiles=m._sparse_tiles(sp, 1, (0, 600)), out=out) == "attention_fp8"
    assert o.calls == [("attention_fp8", (q, k, v, 2), dict(out=out, p_mode="exp2", smooth_k=True, smooth_v=True))]


def test_calibration_refuses_fp8_attention_before_any_launch():
    from frameino_amd.sparse_calibration import calibrate_sparse_attention
    m = _tiny_model(128)
    m.enable_fp8_attention()
    ran = []
    with pytest.raises(NotImplementedError, match="fp8 attention.*bf16 / fp16"):
        calibrate_sparse_attention(m, lambda: ran.append(1), l1_bound=0.05)
    assert not ran and not m.is_sparse_attention_enabled and not m.is_sparse_calibrating
    # fp8 switched on inside the calibration's run(): the tile route refuses, no launch either
    m.enable_fp8_attention(False)
    m.enable_sparse_attention(SparseAttentionConfig(0.5))
    m._sparse_calib = object()
    o = _Ops()
    with pytest.raises(NotImplementedError, match="fp8 attention"):
        m._attend_tiles(o, None, None, None, 2, SimpleNamespace(), fp8=True)
    assert o.calls == []
