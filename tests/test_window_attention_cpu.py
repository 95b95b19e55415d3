"""frameino_amd/window_attention.py on the CPU: the range tables against a brute-force token-level restatement, the densities
DESIGN.md section 6f quotes, the config's validation and the refusals that need no GPU."""
import math

import pytest
import torch

from frameino_amd.window_attention import (WindowAttentionConfig, block_mask, frame_window_ranges, ranges_cover_all,
                                           ranges_density)


def brute_force_tiles(frames, tpf, w, sinks, q_rows=None):
    """per q-block the SET of key tiles: the union, over the block's rows, of the key frames a row may see (its own frame +- w,
    the sinks), every key token mapped to its tile -- i.e. the frames rounded outward to tiles.  Token by token, no intervals."""
    L = frames * tpf
    s0, s1 = q_rows or (0, L)
    sink_set = {s % frames for s in sinks}
    frame_tiles = [{tok // 64 for tok in range(f * tpf, (f + 1) * tpf)} for f in range(frames)]
    out = []
    for r0 in range(s0, s1, 256):
        key_frames = set(sink_set)
        for row in range(r0, min(r0 + 256, s1)):
            f = row // tpf
            key_frames.update(range(max(0, f - w), min(frames, f + w + 1)))
        out.append(set().union(*(frame_tiles[f] for f in key_frames)))
    return out


def table_tiles(table):
    return [{t for a, b in blk for t in range(a, b)} for blk in table.tolist()]


def check_table_form(table, ntall):
    """int32 [nqb, 3, 2]; ranges ascending, disjoint AND not touching (merged), inside [0, ntall], unused entries (0, 0) last"""
    assert table.dtype == torch.int32 and table.shape[1:] == (3, 2) and not table.is_cuda
    for blk in table.tolist():
        used = [(a, b) for a, b in blk if (a, b) != (0, 0)]
        assert blk[:len(used)] == [list(u) for u in used]
        assert all(0 <= a < b <= ntall for a, b in used)
        assert all(used[i][1] < used[i + 1][0] for i in range(len(used) - 1))


@pytest.mark.parametrize("tpf", [60, 99, 880])
@pytest.mark.parametrize("frames", [1, 2, 7, 14, 22])
def test_tables_equal_the_token_level_restatement(frames, tpf):
    L = frames * tpf
    ntall = math.ceil(L / 64)
    offsets = [None, (tpf, L)] + ([(tpf, L - tpf), (37, L - 5)] if frames > 2 else [])
    for w in (0, 1, 2, 3, frames):
        for sinks in ((), (0,), (0, -1), (-1,)):
            for q_rows in offsets:
                if q_rows is not None and q_rows[0] >= q_rows[1]:
                    continue
                table = frame_window_ranges(frames, tpf, w, sinks, q_rows)
                s0, s1 = q_rows or (0, L)
                assert table.shape[0] == math.ceil((s1 - s0) / 256)
                check_table_form(table, ntall)
                assert table_tiles(table) == brute_force_tiles(frames, tpf, w, sinks, q_rows), (w, sinks, q_rows)


def test_densities_of_the_bench_geometry():
    """14 latent frames x 880 tokens (49 q-blocks, 193 key tiles), sinks = first and last frame; 81 frames at 704 x 1280 = 21
    latent frames + the ID frame"""
    want = {1: 0.350, 2: 0.458, 3: 0.558}
    for w, dens in want.items():
        table = frame_window_ranges(14, 880, w, (0, -1))
        assert table.shape == (49, 3, 2)
        assert round(ranges_density(table, 14 * 880), 3) == dens
        assert int((table[:, :, 1] - table[:, :, 0]).sum(1).min()) >= 42
    assert round(ranges_density(frame_window_ranges(22, 880, 2, (0, -1)), 22 * 880), 3) == 0.309


def test_a_covering_window_is_the_full_table_and_block_mask_expands_it():
    table = frame_window_ranges(7, 99, 7, (0,))
    assert ranges_cover_all(table, 7 * 99) and ranges_density(table, 7 * 99) == 1.0
    assert block_mask(table, 7 * 99, 7 * 99).all()
    table = frame_window_ranges(7, 99, 1, (0, -1))
    assert not ranges_cover_all(table, 7 * 99)
    mask = block_mask(table, 7 * 99, 7 * 99)
    tiles = brute_force_tiles(7, 99, 1, (0, -1))
    for row in (0, 255, 256, 600, 692):
        for key in (0, 63, 64, 300, 500, 692):
            assert bool(mask[row, key]) == (key // 64 in tiles[row // 256])


def test_sinks_in_the_middle_need_four_ranges():
    with pytest.raises(ValueError, match="4 key ranges"):
        frame_window_ranges(22, 880, 0, (0, 8, -1), q_rows=(15 * 880, 16 * 880))
    with pytest.raises(ValueError, match="key ranges"):
        frame_window_ranges(22, 880, 1, (0, 10, -1))
    with pytest.raises(ValueError, match="outside"):
        frame_window_ranges(4, 99, 1, (4,))
    with pytest.raises(ValueError, match="q_rows"):
        frame_window_ranges(4, 99, 1, (0,), q_rows=(10, 10))
    with pytest.raises(ValueError, match="window_frames"):
        frame_window_ranges(4, 99, -1, (0,))


def test_config_validation():
    c = WindowAttentionConfig(window_frames=2, sink_frames=[0, -1], skip_layers=[0, 3])
    assert c.sink_frames == (0, -1) and c.skip_layers == (0, 3) and c.timestep_range is None
    assert WindowAttentionConfig(1).sink_frames == (0,)
    for bad in (dict(window_frames=-1), dict(window_frames=1.5), dict(window_frames=True), dict(skip_layers=(-1,)),
                dict(timestep_range=(800, 100), current_timestep_callback=lambda: 0), dict(timestep_range=(100,)),
                dict(timestep_range=(100, 800))):                          # the last: a range without the callback
        with pytest.raises(ValueError):
            WindowAttentionConfig(**{"window_frames": 1, **bad})
    c = WindowAttentionConfig(1, timestep_range=(100, 800), current_timestep_callback=lambda: 500)
    assert c.timestep_range == (100.0, 800.0)


# ------------------------------------------------------------------ the model's and the pipeline's refusals that need no GPU
def _tiny_model():
    from frameino_amd.transformer_wan import WanTransformer3DModel
    return WanTransformer3DModel(num_attention_heads=2, attention_head_dim=64, in_channels=4, out_channels=4, text_dim=32,
                                 freq_dim=32, ffn_dim=64, num_layers=2)


def test_enable_time_refusals():
    from frameino_amd.step_cache import FirstBlockCacheConfig, PyramidAttentionBroadcastConfig
    cfg = WindowAttentionConfig(1)
    m = _tiny_model()
    with pytest.raises(TypeError):
        m.enable_window_attention({"window_frames": 1})
    with pytest.raises(ValueError, match="skip_layers"):
        m.enable_window_attention(WindowAttentionConfig(1, skip_layers=(2,)))
    assert not m.is_window_attention_enabled
    # fp8 attention, either order
    m.enable_fp8_attention()
    with pytest.raises(NotImplementedError, match="fp8 attention"):
        m.enable_window_attention(cfg)
    m.enable_fp8_attention(False)
    m.enable_window_attention(cfg)
    assert m.is_window_attention_enabled
    with pytest.raises(NotImplementedError, match="fp8 attention"):
        m.enable_fp8_attention()
    # Pyramid Attention Broadcast, either order; first-block caching is accepted
    pab = PyramidAttentionBroadcastConfig(spatial_attention_block_skip_range=2, current_timestep_callback=lambda: 500)
    with pytest.raises(NotImplementedError, match="Pyramid Attention Broadcast"):
        m.enable_cache(pab)
    m.enable_cache(FirstBlockCacheConfig(threshold=0.05))
    m.disable_cache()
    m.disable_window_attention()
    assert not m.is_window_attention_enabled
    m.enable_cache(pab)
    with pytest.raises(NotImplementedError, match="Pyramid Attention Broadcast"):
        m.enable_window_attention(cfg)
    m.disable_cache()
    # a token-sharded plan
    m.parallel = type("Shard", (), {"active": True})()
    with pytest.raises(NotImplementedError, match="token-sharded"):
        m.enable_window_attention(cfg)
    m.parallel = None
    # a user-installed attention processor
    from frameino_amd.attention_processor import MI355WanAttnProcessor

    class Mine(MI355WanAttnProcessor):
        pass

    m.blocks[1].attn1.set_processor(Mine())
    with pytest.raises(NotImplementedError, match="attention processor"):
        m.enable_window_attention(cfg)
    m.blocks[1].attn1.set_processor(MI355WanAttnProcessor())
    m.enable_window_attention(cfg)
    assert m.window_attention_log == []


def test_the_pipeline_refuses_a_required_graph_under_a_timestep_range():
    from frameino_amd.pipeline_wan_i2v_motion_frameino import WanImageToVideoPipeline as Pipe
    m = _tiny_model()
    pipe = Pipe.__new__(Pipe)
    pipe.transformer, pipe.use_hip_graph = m, True
    assert pipe._window_attention_check() is False                           # off
    m.enable_window_attention(WindowAttentionConfig(1))
    assert pipe._window_attention_check() is False                           # no range: the step is captured as it is
    m.disable_window_attention()
    m.enable_window_attention(WindowAttentionConfig(1, timestep_range=(100, 800), current_timestep_callback=lambda: 500))
    with pytest.raises(RuntimeError, match="use_hip_graph=True with window attention"):
        pipe._window_attention_check()
    pipe.use_hip_graph = None
    assert pipe._window_attention_check() is True                            # eager loop
    pipe.parallel = object()
    with pytest.raises(NotImplementedError, match="one GPU"):
        pipe._window_attention_check()


def test_the_c_abi_checks_before_any_launch():
    import ctypes
    from frameino_amd import _lib
    lib = _lib.load()
    assert lib.fino_attn_ranges_supported(2, 24, 12320, 12320, 128) == 1 and lib.fino_attn_ranges_supported(1, 2, 8, 8, 64) == 1
    assert lib.fino_attn_ranges_supported(1, 2, 8, 8, 96) == 0 and lib.fino_attn_ranges_supported(1, 2, 0, 8, 64) == 0
    f1 = ctypes.c_float(1.0)
    rc = lib.fino_attn_fwd_ranges(16, 16, 16, 16, 1, 1, 8, 8, 128, *([8] * 12), f1, 0, 0, 0)
    assert rc == -1 and b"ranges" in lib.fino_last_error()
    rc = lib.fino_attn_fwd_ranges(16, 16, 16, 16, 1, 1, 8, 8, 96, *([8] * 12), f1, 0, 16, 0)
    assert rc == -3 and b"head_dim" in lib.fino_last_error()                # what fino_attn_fwd rejects
    rc = lib.fino_attn_fwd_ranges(16, 16, 16, 16, 1, 1, 8, 8, 128, *([8] * 12), f1, 7, 16, 0)
    assert rc == -1 and b"dtype" in lib.fino_last_error()
    rc = lib.fino_attn_fwd_ranges(16, 16, 16, 24, 1, 1, 8, 8, 128, *([8] * 12), f1, 0, 16, 0)
    assert rc == -1 and b"aligned" in lib.fino_last_error()
