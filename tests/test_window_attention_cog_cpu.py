"""Window attention on the CogVideoX backbone, the part that needs no GPU: `prefix_rows` of frameino_amd/window_attention.py (the
text rows in front of frame 0), the densities of the config-5 geometry, the model's and the pipeline's enable / disable / refusal
surface on a CPU-constructed tiny model, and the new entry points in header and ctypes table."""
import pytest
import torch

from frameino_amd.window_attention import (KEY_TILE, Q_BLOCK, WindowAttentionConfig, block_mask, frame_window_ranges,
                                           ranges_cover_all, ranges_density)


@pytest.mark.parametrize("frames,tpf,w,sinks,q_rows", [(14, 880, 2, (0, -1), None), (12, 99, 1, (0, 11), None), (5, 64, 0, (0,), None),
                                                       (12, 99, 1, (0, 11), (99, 1089)), (3, 7, 5, (), None)])
def test_prefix_rows_0_reproduces_the_existing_tables_bit_for_bit(frames, tpf, w, sinks, q_rows):
    old = frame_window_ranges(frames, tpf, w, sinks, q_rows)
    new = frame_window_ranges(frames, tpf, w, sinks, q_rows, prefix_rows=0)
    assert torch.equal(old, new) and new.dtype == torch.int32
    L = frames * tpf
    lq = L if q_rows is None else q_rows[1] - q_rows[0]
    assert torch.equal(block_mask(old, lq, L), block_mask(new, lq, L, prefix_rows=0))
    with pytest.raises(ValueError, match="prefix_rows"):
        frame_window_ranges(frames, tpf, w, sinks, q_rows, prefix_rows=-1)


# BASELINE config 5: [2, 14, 48, 60, 90] -> 14 latent frames (13 + the ID frame) of 30 x 45 = 1350 tokens behind 226 text rows
C5_FRAMES, C5_TPF, C5_TEXT = 14, 1350, 226
C5_L = C5_TEXT + C5_FRAMES * C5_TPF


@pytest.mark.parametrize("w,density,min_tiles", [(1, 0.359, 68), (2, 0.467, 89), (3, 0.565, 110)])
def test_config5_geometry_densities(w, density, min_tiles):
    table = frame_window_ranges(C5_FRAMES, C5_TPF, w, (0, -1), prefix_rows=C5_TEXT)
    assert C5_L == 19126 and table.shape == (75, 3, 2) and -(-C5_L // KEY_TILE) == 299
    n = table[:, :, 1] - table[:, :, 0]
    assert (n >= 0).all() and all(len([1 for a, b in blk if b > a]) <= 3 for blk in table.tolist())
    assert torch.equal(table[0], torch.tensor([[0, 299], [0, 0], [0, 0]], dtype=torch.int32))      # holds the text rows: dense
    assert round(ranges_density(table, C5_L), 3) == density
    assert int(n.sum(1).min()) == min_tiles
    assert not ranges_cover_all(table, C5_L)
    assert ranges_cover_all(frame_window_ranges(C5_FRAMES, C5_TPF, C5_FRAMES, (0, -1), prefix_rows=C5_TEXT), C5_L)


def _brute_force(frames, tpf, p, w, sinks, q_rows):
    """the definition per q-block, row interval by row interval, each rounded outward to tiles: no sorting, no merging"""
    L = p + frames * tpf
    s0, s1 = (0, L) if q_rows is None else q_rows
    mask = torch.zeros(s1 - s0, L, dtype=torch.bool)
    sinks = [s + frames if s < 0 else s for s in sinks]
    for r0 in range(s0, s1, Q_BLOCK):
        r1 = min(r0 + Q_BLOCK, s1)
        if r0 < p:
            mask[r0 - s0:r1 - s0] = True
            continue
        f0, f1 = (r0 - p) // tpf, (r1 - 1 - p) // tpf
        rows = [(p + max(0, f0 - w) * tpf, p + min(frames, f1 + w + 1) * tpf)] + [(p + s * tpf, p + (s + 1) * tpf) for s in sinks]
        if p:
            rows.append((0, p))
        for a, b in rows:
            mask[r0 - s0:r1 - s0, a // KEY_TILE * KEY_TILE:min(L, -(-b // KEY_TILE) * KEY_TILE)] = True
    return mask


@pytest.mark.parametrize("frames,tpf,p,w,sinks,q_rows", [
    (9, 150, 8, 1, (0, -1), None),           # the GPU tests' tiny geometry
    (9, 150, 8, 1, (0, -1), (8, 8 + 8 * 150)),      # the last block's live rows under live_frames
    (9, 150, 8, 0, (0,), None), (6, 99, 226, 1, (0, 5), None), (7, 64, 64, 2, (0,), None), (5, 200, 300, 1, (), None),
    (14, 1350, 226, 2, (0, -1), None)])
def test_block_mask_with_a_prefix_equals_the_brute_force_definition(frames, tpf, p, w, sinks, q_rows):
    L = p + frames * tpf
    table = frame_window_ranges(frames, tpf, w, sinks, q_rows, prefix_rows=p)
    lq = L if q_rows is None else q_rows[1] - q_rows[0]
    assert table.shape[0] == -(-lq // Q_BLOCK)
    got = block_mask(table, lq, L, prefix_rows=p)
    assert torch.equal(got, _brute_force(frames, tpf, p, w, sinks, q_rows))
    for blk in table.tolist():               # ascending, disjoint, merged where they touch
        used = [(a, b) for a, b in blk if b > a]
        assert all(used[i][1] < used[i + 1][0] for i in range(len(used) - 1))
    if p and q_rows is None:
        assert got[:, :p].all() and got[:p].all()              # text keys for every query, every key for text queries
    with pytest.raises(ValueError, match="prefix_rows"):
        block_mask(table, lq, L, prefix_rows=L + 1)


def test_the_tiny_geometry_of_the_gpu_tests():
    from tests.cog_window_attn_ref import FRAMES, L, SINKS, TEXT, TPF
    table = frame_window_ranges(FRAMES, TPF, 1, SINKS, prefix_rows=TEXT)
    assert L == 1358 and table.shape[0] == 6 and -(-L // KEY_TILE) == 22 and L - 21 * KEY_TILE == 14
    assert round(ranges_density(table, L), 3) == 0.735
    assert table[0].tolist() == [[0, 22], [0, 0], [0, 0]]
    assert len([1 for a, b in table[2].tolist() if b > a]) == 3
    with pytest.raises(ValueError, match="ranges"):            # a sink in the middle of the clip: four ranges for some q-block
        frame_window_ranges(FRAMES, TPF, 0, (0, 3, 8), prefix_rows=TEXT)


# ------------------------------------------------------------------ the model's and the pipeline's surface without a GPU
def _tiny_model(**over):
    from frameino_amd.cogvideox_transformer_3d import CogVideoXTransformer3DModel
    from tests.cog_window_attn_ref import TINY_CFG
    return CogVideoXTransformer3DModel(**{**TINY_CFG, **over})


def test_enable_disable_and_refusals():
    from frameino_amd.attention_processor import MI355CogVideoXAttnProcessor
    cfg = WindowAttentionConfig(1)
    m = _tiny_model()
    assert not m.is_window_attention_enabled and m.window_attention_log == []
    with pytest.raises(TypeError):
        m.enable_window_attention({"window_frames": 1})
    with pytest.raises(ValueError, match="skip_layers"):
        m.enable_window_attention(WindowAttentionConfig(1, skip_layers=(2,)))
    assert not m.is_window_attention_enabled
    # fp8 attention at head_dim 64 combines, either order
    m.enable_fp8_attention(smooth_k=True)
    assert m.enable_window_attention(cfg) is m and m.is_window_attention_enabled
    m.enable_fp8_attention(False)
    m.enable_fp8_attention()
    assert m.disable_window_attention() is m and not m.is_window_attention_enabled
    # ... and is refused, with the reason, at any other head_dim
    m128 = _tiny_model(num_attention_heads=1, attention_head_dim=128)
    m128.enable_fp8_attention()
    with pytest.raises(NotImplementedError, match="head_dim 128"):
        m128.enable_window_attention(cfg)
    m128.enable_fp8_attention(False)
    m128.enable_window_attention(cfg)                           # (bf16 / fp16 ranges exist at head_dim 128)
    # a user-installed attention processor

    class Mine(MI355CogVideoXAttnProcessor):
        pass

    m.transformer_blocks[1].attn1.set_processor(Mine())
    with pytest.raises(NotImplementedError, match="attention processor"):
        m.enable_window_attention(cfg)
    m.transformer_blocks[1].attn1.set_processor(MI355CogVideoXAttnProcessor())
    m.enable_window_attention(cfg)
    assert m.window_attention_log == []


def test_the_forward_refuses_before_any_launch_what_enable_could_not_see():
    """a processor installed, or fp8 attention switched on at head_dim 128, AFTER enable_window_attention: the forward raises
    before it touches `ops` (a stand-in that fails on any use)"""
    from frameino_amd.attention_processor import MI355CogVideoXAttnProcessor

    class NoOps:
        def __getattr__(self, name):
            raise AssertionError(f"ops.{name} was reached")

    class Mine(MI355CogVideoXAttnProcessor):
        pass

    x, txt, ts = torch.zeros(1, 9, 6, 20, 30), torch.zeros(1, 8, 16), torch.zeros(1)
    m = _tiny_model()
    m.ops = NoOps()
    m.enable_window_attention(WindowAttentionConfig(1))
    m.transformer_blocks[0].attn1.set_processor(Mine())
    with pytest.raises(NotImplementedError, match="attention processor"):
        m(x, txt, ts, id_frames=1)
    m128 = _tiny_model(num_attention_heads=1, attention_head_dim=128)
    m128.ops = NoOps()
    m128.enable_window_attention(WindowAttentionConfig(1))
    m128.enable_fp8_attention()
    with pytest.raises(NotImplementedError, match="head_dim 128"):
        m128(x, txt, ts, id_frames=1)
    assert m.window_attention_log == [] and m128.window_attention_log == []


def test_tables_are_cached_per_geometry_and_dropped_with_the_other_caches():
    m = _tiny_model()
    m.enable_window_attention(WindowAttentionConfig(1))
    win = m._window_begin(9, 150, 8, 1, torch.device("cpu"))
    t = win.table((0, 1358))
    assert t.dtype == torch.int32 and tuple(t.shape) == (6, 3, 2) and win.table((0, 1358)) is t
    assert torch.equal(t, frame_window_ranges(9, 150, 1, (0, 8), prefix_rows=8))
    assert tuple(win.table((8, 1208)).shape) == (5, 3, 2)
    assert sum(1 for k in m._pos_cache if k[0] == "window") == 2
    assert m._window_begin(9, 150, 8, 0, torch.device("cpu")).table((0, 1358)) is not t     # id_frames is part of the key
    assert m.window_attention_log == [(0, None, True), (1, None, True)]
    m.reset_caches()
    assert not any(k[0] == "window" for k in m._pos_cache)
    # a window at least as large as the clip: no table, the dense call
    m.enable_window_attention(WindowAttentionConfig(9))
    assert m._window_begin(9, 150, 8, 1, torch.device("cpu")).table((0, 1358)) is None
    with pytest.raises(ValueError, match="id_frames"):
        m._window_begin(9, 150, 8, 9, torch.device("cpu"))
    # the timestep range: read once per forward, strict bounds, logged
    clock = {"t": 500.0, "reads": 0}

    def now():
        clock["reads"] += 1
        return clock["t"]

    m.enable_window_attention(WindowAttentionConfig(1, timestep_range=(100, 800), current_timestep_callback=now))
    assert m._window_begin(9, 150, 8, 1, torch.device("cpu")) is not None
    clock["t"] = 800.0
    assert m._window_begin(9, 150, 8, 1, torch.device("cpu")) is None
    assert m.window_attention_log == [(0, 500.0, True), (1, 800.0, False)] and clock["reads"] == 2


def test_the_pipeline_refuses_a_required_graph_under_a_timestep_range():
    from frameino_amd.pipeline_cogvideox_i2v_motion import CogVideoXImageToVideoPipeline as Stage1
    from frameino_amd.pipeline_cogvideox_i2v_motion_frameino import CogVideoXImageToVideoPipeline as Pipe
    for cls in (Pipe, Stage1):
        m = _tiny_model()
        pipe = cls(transformer=m)
        assert pipe.current_timestep is None
        pipe.use_hip_graph = True
        assert pipe._window_attention_check() is False                       # off
        m.enable_window_attention(WindowAttentionConfig(1))
        assert pipe._window_attention_check() is False                       # a static table: the step captures
        m.enable_window_attention(WindowAttentionConfig(1, timestep_range=(100, 800),
                                                        current_timestep_callback=lambda: pipe.current_timestep))
        with pytest.raises(RuntimeError, match="use_hip_graph=True"):
            pipe._window_attention_check()
        pipe.use_hip_graph = None
        assert pipe._window_attention_check() is True                        # the loop runs eagerly


def test_the_new_entry_points_are_in_header_and_ctypes_table():
    from frameino_amd import _lib, ops
    declared = _lib.declared_symbols()
    for name in ("fino_attn_fp8_ranges_supported", "fino_attn_fwd_fp8_ranges"):
        assert name in declared and name in _lib.SIGNATURES
    fwd, dense = _lib.SIGNATURES["fino_attn_fwd_fp8_ranges"], _lib.SIGNATURES["fino_attn_fwd_fp8"]
    assert fwd[:len(dense) - 1] == dense[:-1] and len(fwd) == len(dense) + 2           # + int smooth_k, const int* ranges
    assert _lib.ABI_VERSION == 103
    assert callable(ops.attention_fp8_ranges) and callable(ops.attention_fp8_ranges_supported)
