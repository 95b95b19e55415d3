"""Dynamic block-sparse self-attention (frameino_amd/window_attention.py: SparseAttentionConfig, the mixin's host path;
DESIGN.md section 6j): everything that needs no GPU -- the config, every refusal in both orders, the dispatch in `_attend` with
a recording stand-in for `ops`, the pipeline's rule, the C ABI's surface, and the float64 reference's own properties."""
import ctypes
import os
from types import SimpleNamespace

import pytest
import torch

from frameino_amd.window_attention import SparseAttentionConfig, WindowAttentionConfig
from tests import sparse_attn_ref as R


def test_config_validation():
    c = SparseAttentionConfig()
    assert (c.cdf_threshold, c.window_frames, c.sink_frames, c.skip_layers, c.keep_masks) == (0.9, 0, (0,), (), False)
    c = SparseAttentionConfig(cdf_threshold=1, sink_frames=[0, -1], skip_layers=[0, 3], keep_masks=1)
    assert c.cdf_threshold == 1.0 and c.sink_frames == (0, -1) and c.skip_layers == (0, 3) and c.keep_masks is True
    assert SparseAttentionConfig(cdf_threshold=2.5).cdf_threshold == 2.5                 # >= 1: dense
    for bad in (dict(cdf_threshold=0), dict(cdf_threshold=-0.5), dict(cdf_threshold=float("inf")), dict(cdf_threshold=float("nan")),
                dict(cdf_threshold="0.9"), dict(cdf_threshold=True), dict(window_frames=-1), dict(window_frames=1.5),
                dict(window_frames=True), dict(skip_layers=(-1,)), dict(sink_frames=3)):
        with pytest.raises(ValueError):
            SparseAttentionConfig(**bad)


def _tiny_model():
    from frameino_amd.transformer_wan import WanTransformer3DModel
    return WanTransformer3DModel(num_attention_heads=2, attention_head_dim=64, in_channels=4, out_channels=4, text_dim=32,
                                 freq_dim=32, ffn_dim=64, num_layers=2)


def test_enable_time_refusals_in_both_orders():
    from frameino_amd.attention_processor import MI355WanAttnProcessor
    from frameino_amd.step_cache import FirstBlockCacheConfig, PyramidAttentionBroadcastConfig
    cfg = SparseAttentionConfig(0.5)
    m = _tiny_model()
    with pytest.raises(TypeError):
        m.enable_sparse_attention({"cdf_threshold": 0.5})
    with pytest.raises(TypeError):
        m.enable_sparse_attention(WindowAttentionConfig(1))
    with pytest.raises(ValueError, match="skip_layers"):
        m.enable_sparse_attention(SparseAttentionConfig(0.5, skip_layers=(2,)))
    assert not m.is_sparse_attention_enabled
    # window attention, either order
    m.enable_window_attention(WindowAttentionConfig(1))
    with pytest.raises(NotImplementedError, match="window attention"):
        m.enable_sparse_attention(cfg)
    m.disable_window_attention()
    assert m.enable_sparse_attention(cfg) is m and m.is_sparse_attention_enabled
    with pytest.raises(NotImplementedError, match="sparse attention"):
        m.enable_window_attention(WindowAttentionConfig(1))
    assert not m.is_window_attention_enabled
    # fp8 attention, either order
    with pytest.raises(NotImplementedError, match="fp8 attention"):
        m.enable_fp8_attention()
    assert not m.fp8_attention
    m.enable_fp8_attention(False)
    m.disable_sparse_attention()
    m.enable_fp8_attention()
    with pytest.raises(NotImplementedError, match="fp8 attention"):
        m.enable_sparse_attention(cfg)
    m.enable_fp8_attention(False)
    # Pyramid Attention Broadcast, either order; first-block caching is accepted
    pab = PyramidAttentionBroadcastConfig(spatial_attention_block_skip_range=2, current_timestep_callback=lambda: 500)
    m.enable_sparse_attention(cfg)
    with pytest.raises(NotImplementedError, match="Pyramid Attention Broadcast"):
        m.enable_cache(pab)
    m.enable_cache(FirstBlockCacheConfig(threshold=0.05))
    m.disable_cache()
    m.disable_sparse_attention()
    assert not m.is_sparse_attention_enabled
    m.enable_cache(pab)
    with pytest.raises(NotImplementedError, match="Pyramid Attention Broadcast"):
        m.enable_sparse_attention(cfg)
    m.disable_cache()
    # a token-sharded plan
    m.parallel = type("Shard", (), {"active": True})()
    with pytest.raises(NotImplementedError, match="token-sharded"):
        m.enable_sparse_attention(cfg)
    m.parallel = None

    # a user-installed attention processor
    class Mine(MI355WanAttnProcessor):
        pass

    m.blocks[1].attn1.set_processor(Mine())
    with pytest.raises(NotImplementedError, match="attention processor"):
        m.enable_sparse_attention(cfg)
    m.blocks[1].attn1.set_processor(MI355WanAttnProcessor())
    m.enable_sparse_attention(cfg)
    assert m.sparse_attention_masks == {} and m.sparse_attention_density() == {}


def test_the_existing_refusals_are_what_they_were():
    """window attention with fp8 / Pyramid Attention Broadcast, with sparse attention off: the messages of before"""
    from frameino_amd.step_cache import PyramidAttentionBroadcastConfig
    m = _tiny_model()
    m.enable_window_attention(WindowAttentionConfig(1))
    with pytest.raises(NotImplementedError, match=r"window attention \(enable_window_attention\) with fp8 attention"):
        m.enable_fp8_attention()
    with pytest.raises(NotImplementedError, match="Pyramid Attention Broadcast with window attention"):
        m.enable_cache(PyramidAttentionBroadcastConfig(spatial_attention_block_skip_range=2, current_timestep_callback=lambda: 500))


def test_cogvideox_is_not_wired():
    from frameino_amd.cogvideox_transformer_3d import CogVideoXTransformer3DModel
    m = CogVideoXTransformer3DModel(num_attention_heads=2, attention_head_dim=64, in_channels=4, out_channels=4, num_layers=1,
                                    text_embed_dim=32, time_embed_dim=32, sample_width=8, sample_height=8, sample_frames=5,
                                    use_rotary_positional_embeddings=True)
    assert not m.is_sparse_attention_enabled
    with pytest.raises(NotImplementedError, match="not wired on this model"):
        m.enable_sparse_attention(SparseAttentionConfig(0.5))
    assert not m.is_sparse_attention_enabled


class _Ops:
    """records which front end `_attend` picked, with what"""

    def __init__(self):
        self.calls = []

    def _rec(name):                       # noqa: N805
        def f(self, *a, **kw):
            self.calls.append((name, a, kw))
            return name
        return f

    attention, attention_ranges = _rec("attention"), _rec("attention_ranges")
    attention_fp8, attention_fp8_ranges = _rec("attention_fp8"), _rec("attention_fp8_ranges")
    attention_tiles = _rec("attention_tiles")

    def attention_tile_plan(self, q, k, heads, cdf, keep_ranges=None, scale=None, out=None, workspace=None):
        self.calls.append(("attention_tile_plan", (q, k, heads, cdf), dict(keep_ranges=keep_ranges, scale=scale, out=out,
                                                                           workspace=workspace)))
        out.fill_(7)
        return out


def test_attend_routes():
    m = _tiny_model()
    q, k, v = torch.zeros(2, 600, 128), torch.zeros(2, 1100, 128), torch.zeros(2, 1100, 128)
    table, out = torch.zeros(3, 3, 2, dtype=torch.int32), torch.zeros(2, 600, 128)
    # the four routes of before, their keywords as before
    o = _Ops()
    assert m._attend(o, q, k, v, 2, fp8=False, out=out, scale=-1.0) == "attention"
    assert m._attend(o, q, k, v, 2, fp8=False, ranges=table, out=out) == "attention_ranges"
    m.fp8_attention, m.fp8_p_mode, m.fp8_smooth_k, m.fp8_smooth_v = True, "ramp", True, False
    assert m._attend(o, q, k, v, 2, fp8=True, out=out) == "attention_fp8"
    assert m._attend(o, q, k, v, 2, fp8=True, ranges=table) == "attention_fp8_ranges"
    assert m._attend(o, q, k, v, 2, fp8=False, tiles=None) == "attention"
    fp8_kw = dict(p_mode="ramp", smooth_k=True, smooth_v=False)
    assert o.calls == [("attention", (q, k, v, 2), dict(out=out, scale=-1.0)),
                       ("attention_ranges", (q, k, v, 2, table), dict(out=out)),
                       ("attention_fp8", (q, k, v, 2), dict(out=out, **fp8_kw)),
                       ("attention_fp8_ranges", (q, k, v, 2, table), fp8_kw),
                       ("attention", (q, k, v, 2), {})]
    # the tile route: the plan on this call's q and k into the buffer's leading rows, then the walk over that mask
    m.fp8_attention = False
    m.enable_sparse_attention(SparseAttentionConfig(0.5, keep_masks=True))
    o = _Ops()
    sp = SimpleNamespace(keep=lambda q_rows: table, skip=frozenset({1}), cdf=0.5, words=1, lk=1100,
                         mask=torch.zeros(2 * 2 * 5 * 1, dtype=torch.int32), workspace="ws", keep_masks=True)
    assert m._sparse_tiles(None, 0, (0, 600)) is None and m._sparse_tiles(sp, 1, (0, 600)) is None          # off; a skipped layer
    sp_dense = SimpleNamespace(keep=lambda q_rows: None, skip=frozenset())
    assert m._sparse_tiles(sp_dense, 0, (0, 600)) is None                                                    # forced tiles cover all
    tiles = m._sparse_tiles(sp, 0, (0, 600))
    assert m._attend(o, q, k, v, 2, fp8=False, tiles=tiles, out=out, scale=-1.0) == "attention_tiles"
    (n0, a0, kw0), (n1, a1, kw1) = o.calls
    assert n0 == "attention_tile_plan" and a0[0] is q and a0[1] is k and a0[2:] == (2, 0.5)
    assert kw0["keep_ranges"] is table and kw0["scale"] == -1.0 and kw0["workspace"] == "ws"
    assert tuple(kw0["out"].shape) == (2, 2, 3, 1) and kw0["out"].data_ptr() == sp.mask.data_ptr()
    assert n1 == "attention_tiles" and a1[:4] == (q, k, v, 2) and a1[4] is kw0["out"] and kw1 == dict(out=out, scale=-1.0)
    assert sp.mask.tolist() == [7] * 12 + [0] * 8
    assert list(m.sparse_attention_masks) == [0] and m.sparse_attention_masks[0].tolist() == kw0["out"].tolist()
    assert m.sparse_attention_masks[0].data_ptr() != sp.mask.data_ptr()


def test_a_threshold_of_one_is_dense_and_plans_nothing():
    m = _tiny_model()
    ws = SimpleNamespace()
    for tau in (1.0, 3.0):
        m.enable_sparse_attention(SparseAttentionConfig(tau))
        assert m._sparse_begin(4, 99, 0, "cpu", ws, 1, 2, 64) is None and not hasattr(ws, "sparse_mask")
        m.disable_sparse_attention()
    assert m._sparse_begin(4, 99, 0, "cpu", ws, 1, 2, 64) is None                       # off
    o = _Ops()
    m._attend(o, torch.zeros(1, 8, 128), torch.zeros(1, 8, 128), torch.zeros(1, 8, 128), 2, fp8=False,
              tiles=m._sparse_tiles(None, 0, (0, 8)))
    assert [c[0] for c in o.calls] == ["attention"]


def test_sparse_begin_builds_the_forced_tables_and_reuses_the_table_cache():
    from frameino_amd.window_attention import frame_window_ranges
    m = _tiny_model()
    m.ops = SimpleNamespace(attention_tile_plan_bytes=lambda b, h, lq, lk, dh: 4 * b * h * dh * (-(-lq // 256) + -(-lk // 64)))
    m.enable_sparse_attention(SparseAttentionConfig(0.5, window_frames=0, skip_layers=(1,)))
    ws = SimpleNamespace()
    sp = m._sparse_begin(12, 99, 1, "cpu", ws, 2, 2, 64)
    L = 12 * 99
    assert sp.cdf == 0.5 and sp.skip == frozenset({1}) and sp.words == 1 and sp.lk == L
    assert sp.mask is ws.sparse_mask and sp.mask.numel() == 2 * 2 * 5 * 1 and sp.mask.dtype == torch.int32
    assert sp.workspace is ws.sparse_plan and sp.workspace.numel() * 4 == 4 * 2 * 2 * 64 * (5 + 19)
    want = frame_window_ranges(12, 99, 0, (0, 11))                                   # the config's sink + the ID frame
    assert torch.equal(sp.keep((0, L)), want) and sp.keep((0, L)) is sp.keep((0, L))
    live = (99, 11 * 99)
    assert torch.equal(sp.keep(live), frame_window_ranges(12, 99, 0, (0, 11), q_rows=live))
    assert sum(k[0] == "sparse" for k in m._rope_cache) == 2
    again = m._sparse_begin(12, 99, 1, "cpu", ws, 2, 2, 64)
    assert again.mask is sp.mask and again.workspace is sp.workspace                 # allocated once per workspace
    ws.sparse_plan = ws.sparse_plan[:8]                                              # the two buffers are sized independently
    grown = m._sparse_begin(12, 99, 1, "cpu", ws, 2, 2, 64)
    assert grown.mask is sp.mask and grown.workspace.numel() == sp.workspace.numel()
    m.sparse_attention_masks[0], m._sparse_mask_keys[0] = sp.mask, L
    m.disable_sparse_attention()
    assert m.sparse_attention_masks == {} and m._sparse_mask_keys == {}
    m.enable_sparse_attention(SparseAttentionConfig(0.5, window_frames=0, skip_layers=(1,)))
    m.reset_caches()
    assert not any(k[0] == "sparse" for k in m._rope_cache)
    with pytest.raises(ValueError, match="id_frames"):
        m._sparse_begin(12, 99, 12, "cpu", ws, 2, 2, 64)
    # forced tiles that cover everything: the dense call
    m.enable_sparse_attention(SparseAttentionConfig(0.5, window_frames=12))
    assert m._sparse_begin(12, 99, 1, "cpu", ws, 2, 2, 64).keep((0, L)) is None


def test_the_pipeline_keeps_the_graph_loop_and_refuses_a_parallel_plan():
    from frameino_amd.pipeline_wan_i2v_motion_frameino import WanImageToVideoPipeline as Pipe
    m = _tiny_model()
    pipe = Pipe.__new__(Pipe)
    pipe.transformer, pipe.use_hip_graph = m, True
    m.enable_sparse_attention(SparseAttentionConfig(0.5))
    assert pipe._window_attention_check() is False                 # no timestep gate: the step is captured as it is
    pipe.parallel = object()
    with pytest.raises(NotImplementedError, match="sparse attention runs on one GPU"):
        pipe._window_attention_check()
    m.disable_sparse_attention()
    assert pipe._window_attention_check() is False


def test_the_header_the_signatures_and_the_library_carry_the_entry_points():
    from frameino_amd import _lib
    names = ("fino_attn_tiles_supported", "fino_attn_fwd_tiles", "fino_attn_tile_plan_bytes", "fino_attn_tile_plan")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "frameino_hip.h")).read()
    lib = _lib.load()
    for n in names:
        assert n + "(" in header and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert "#define FINO_VERSION 103" in header and lib.fino_version() == 103
    assert len(_lib.SIGNATURES["fino_attn_fwd_tiles"]) == 28 and len(_lib.SIGNATURES["fino_attn_tile_plan"]) == 22
    assert lib.fino_attn_tiles_supported(2, 24, 12320, 12320, 128) == 1 and lib.fino_attn_tiles_supported(1, 2, 8, 8, 64) == 1
    assert lib.fino_attn_tiles_supported(1, 2, 8, 8, 96) == 0 and lib.fino_attn_tiles_supported(1, 2, 8, 65537, 64) == 0
    assert lib.fino_attn_tile_plan_bytes(2, 24, 12320, 12320, 128) == 2 * 24 * (49 + 193) * 128 * 4
    assert lib.fino_attn_tile_plan_bytes(2, 24, 12320, 12320, 96) == 0
    # argument checks come before any launch
    f1, h = ctypes.c_float(1.0), ctypes.c_float(0.5)
    rc = lib.fino_attn_fwd_tiles(16, 16, 16, 16, 1, 1, 8, 8, 128, *([8] * 12), f1, 0, 0, 0, 0, 1, 0)
    assert rc == -1 and b"null mask" in lib.fino_last_error()
    rc = lib.fino_attn_fwd_tiles(16, 16, 16, 16, 1, 1, 8, 64 * 33, 128, *([8] * 12), f1, 0, 16, 0, 0, 1, 0)
    assert rc == -1 and b"mask words" in lib.fino_last_error()
    rc = lib.fino_attn_tile_plan(16, 16, 1, 1, 8, 8, 128, *([8] * 6), f1, 0, h, 0, 0, 1, 16, 1 << 20, 0)
    assert rc == -1 and b"null pointer" in lib.fino_last_error()
    rc = lib.fino_attn_tile_plan(16, 16, 1, 1, 8, 8, 128, *([8] * 6), f1, 0, h, 0, 16, 1, 16, 64, 0)
    assert rc == -1 and b"workspace of" in lib.fino_last_error()
    rc = lib.fino_attn_tile_plan(16, 16, 1, 1, 8, 8, 128, *([8] * 6), f1, 0, ctypes.c_float(0.0), 0, 16, 1, 16, 1 << 20, 0)
    assert rc == -1 and b"cdf" in lib.fino_last_error()
    rc = lib.fino_attn_tile_plan(16, 16, 1, 1, 8, 8, 96, *([8] * 6), f1, 0, h, 0, 16, 1, 16, 1 << 20, 0)
    assert rc == -3 and b"head_dim" in lib.fino_last_error()


def test_reference_properties():
    """the float64 reference: kept mass >= cdf, minimal (dropping the smallest kept free tile falls below cdf), forced tiles
    kept, m_F >= cdf keeps F alone, ties kept together"""
    g = torch.Generator().manual_seed(5)
    for trial in range(40):
        nt = int(torch.randint(1, 40, (1,), generator=g))
        p = torch.rand(nt, generator=g, dtype=torch.float64) ** 3
        if trial % 4 == 0 and nt > 3:
            p[1] = p[2] = p[0]                                     # ties
        p = p / p.sum()
        forced = torch.rand(nt, generator=g) < 0.2
        for cdf in (0.2, 0.5, 0.9, 0.999):
            keep = R.select_row(p, forced, cdf)
            m_f, mass = float(p[forced].sum()), float(p[keep].sum())
            assert bool(keep[forced].all()) and (mass >= cdf or bool(keep.all()))
            extra = keep & ~forced
            if m_f >= cdf:
                assert not extra.any()
            elif extra.any():
                theta = float(p[extra].min())
                assert mass - float(p[extra & (p == theta)].sum()) < cdf               # without theta's tiles: below cdf
                assert bool(keep[~forced & (p >= theta)].all()) and not keep[~forced & (p < theta)].any()
    assert R.select_row(torch.tensor([0.5, 0.5], dtype=torch.float64), torch.zeros(2, dtype=torch.bool), 0.25).all()
