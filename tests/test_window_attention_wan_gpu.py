"""Sliding-window self-attention over frames on the Wan DiT (WanTransformer3DModel.enable_window_attention) against the
restatement in tests/window_attn_ref.py: the oracle's pieces in bf16 with the self-attention under the boolean block mask expanded
from the same range table.  Tiny random model (4 heads x 128, 2 blocks), 12 latent frames of 9 x 11 = 99 tokens (not a multiple
of the 64-key tile; 1188 rows = five q-blocks, the last ragged; the middle q-blocks walk three ranges), window_frames = 1,
sink frame 0, the last frame an ID frame.  Tolerance of a forward against the bf16 oracle: the one
tests/test_wan_model_gpu.py and tests/test_pab_wan_gpu.py state, rel-RMS < 1.5e-2."""
import pytest
import torch

from frameino_amd.window_attention import WindowAttentionConfig, frame_window_ranges, ranges_cover_all
from oracle import wan_dit as W
from tests.parity import bf16_state_dict, hip_wan_model, rel_rms
from tests.window_attn_ref import layer_masks, window_forward

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOUND = 1.5e-2
CFG = dict(W.WAN22_5B_CFG, num_attention_heads=4, attention_head_dim=128, in_channels=16, out_channels=8, text_dim=256,
           ffn_dim=1024, num_layers=2)
FRAMES, TPF = 12, 99
L = FRAMES * TPF
TS = torch.tensor([811.0])
SINKS = (0, FRAMES - 1)                     # config sink (0,) + id_frames = 1


def _inputs(v_scale):
    """weights with the self-attention's value projection scaled by `v_scale`, a latent whose frames differ by an offset"""
    sd = W.wan_random_state_dict(CFG, seed=11, dtype=torch.float32, std=0.04)
    for k in sd:
        if ".attn1.to_v.weight" in k:
            sd[k] = sd[k] * v_scale
    g = torch.Generator().manual_seed(12)
    x = torch.randn(1, 16, FRAMES, 18, 22, generator=g) + torch.randn(1, 16, FRAMES, 1, 1, generator=g)
    txt = torch.randn(2, 77, 256, generator=g)
    return sd, bf16_state_dict(sd), x, txt


@pytest.fixture(scope="module")
def setup():
    """inputs on which the restatement's windowed and dense outputs differ by at least 5 x BOUND (on the CPU, the restatement
    alone): otherwise no assertion below could tell a window from none.  The inputs are scaled until they do."""
    masks = layer_masks(2, FRAMES, TPF, 1, SINKS)
    for v_scale in (4.0, 8.0, 16.0):
        sd, sdb, x, txt = _inputs(v_scale)
        dense = window_forward(sdb, CFG, x.bfloat16(), TS, txt[:1].bfloat16(), {})
        windowed = window_forward(sdb, CFG, x.bfloat16(), TS, txt[:1].bfloat16(), masks)
        gap = rel_rms(windowed, dense)
        print(f"restatement: windowed vs dense rel-RMS {gap:.3e} at value scale {v_scale} (needs >= {5 * BOUND:.3e})")
        if gap >= 5 * BOUND:
            return sd, sdb, x, txt, dense, windowed, gap
    raise AssertionError(f"no scale separates the window from the dense model: last gap {gap}")


def _model(sd, **cfg):
    m = hip_wan_model(CFG, sd, DEV)
    if cfg:
        m.enable_window_attention(WindowAttentionConfig(**{"window_frames": 1, "sink_frames": (0,), **cfg}))
    return m


def _fwd(m, x, txt, ts=TS, **kw):
    return m(x.to(DEV, torch.bfloat16), ts.to(DEV), txt.to(DEV, torch.bfloat16), return_dict=False, **kw)[0]


def test_the_geometry_is_the_one_the_issue_asks_for():
    table = frame_window_ranges(FRAMES, TPF, 1, SINKS)
    assert TPF % 64 != 0 and table.shape[0] >= 4 and not ranges_cover_all(table, L)
    assert any(len([1 for a, b in blk if b > a]) == 3 for blk in table.tolist())       # some q-block walks three ranges


def test_windowed_forward_matches_the_restatement(setup):
    sd, sdb, x, txt, dense, windowed, gap = setup
    assert gap >= 5 * BOUND
    m = _model(sd, window_frames=1)
    out = _fwd(m, x, txt[:1], id_frames=1)
    err, far = rel_rms(out, windowed), rel_rms(out, dense)
    print(f"windowed forward: rel-RMS {err:.3e} against the restatement, {far:.3e} against the dense restatement")
    assert err < BOUND
    assert far > 3 * BOUND                                   # (and so it is not the dense model)
    assert m.window_attention_log == [(0, None, True)]
    # the dense model on the same weights is within the bound of the DENSE restatement
    assert rel_rms(_fwd(_model(sd), x, txt[:1]), dense) < BOUND
    # without id_frames the last frame is no sink: another mask, another result
    assert not torch.equal(_fwd(m, x, txt[:1]), out)


def test_an_all_covering_window_is_the_dense_forward_bit_for_bit(setup):
    sd, _, x, txt = setup[:4]
    want = _fwd(_model(sd), x, txt[:1])
    m = _model(sd, window_frames=FRAMES)
    assert torch.equal(_fwd(m, x, txt[:1], id_frames=1), want)
    m.disable_window_attention()
    m.enable_window_attention(WindowAttentionConfig(window_frames=1, skip_layers=(0, 1)))      # every layer dense
    assert torch.equal(_fwd(m, x, txt[:1], id_frames=1), want)
    m.disable_window_attention()
    assert torch.equal(_fwd(m, x, txt[:1], id_frames=1), want) and not m.is_window_attention_enabled


@pytest.mark.parametrize("skip", [(0,), (1,)])
def test_skip_layers_stay_dense(setup, skip):
    sd, sdb, x, txt, dense, windowed, _ = setup
    want = window_forward(sdb, CFG, x.bfloat16(), TS, txt[:1].bfloat16(), layer_masks(2, FRAMES, TPF, 1, SINKS, skip_layers=skip))
    out = _fwd(_model(sd, window_frames=1, skip_layers=skip), x, txt[:1], id_frames=1)
    err = rel_rms(out, want)
    print(f"skip_layers {skip}: rel-RMS {err:.3e} against the restatement; restatement vs all-windowed "
          f"{rel_rms(want, windowed):.3e}, vs dense {rel_rms(want, dense):.3e}")
    assert err < BOUND
    assert not torch.equal(out, _fwd(_model(sd, window_frames=1), x, txt[:1], id_frames=1))


def test_live_rows_match_the_restatement(setup):
    """the last block's queries start at the first live row: its table is built with q_rows = the live rows"""
    sd, sdb, x, txt = setup[:4]
    live = (TPF, (FRAMES - 1) * TPF)                                        # the caller drops the first frame and the ID frame
    want = window_forward(sdb, CFG, x.bfloat16(), TS, txt[:1].bfloat16(), layer_masks(2, FRAMES, TPF, 1, SINKS, live_rows=live))
    m = _model(sd, window_frames=1)
    out = _fwd(m, x, txt[:1], id_frames=1, live_rows=live)
    err = rel_rms(out[:, :, 1:FRAMES - 1], want[:, :, 1:FRAMES - 1])
    print(f"live rows: rel-RMS {err:.3e} against the restatement")
    assert err < BOUND
    assert float(out[:, :, 0].abs().max()) == 0.0 and float(out[:, :, FRAMES - 1].abs().max()) == 0.0
    assert any(k[0] == "window" and k[5] == live for k in m._rope_cache)     # (the table of the live query rows was built)
    m.reset_caches()
    assert not any(k[0] == "window" for k in m._rope_cache)


def test_the_cfg_batch_with_the_shared_prefix_equals_two_single_calls(setup):
    sd, _, x, txt = setup[:4]
    m = _model(sd, window_frames=1)
    xd = x.to(DEV, torch.bfloat16)
    both = m(xd.expand(2, -1, -1, -1, -1), TS.to(DEV), txt.to(DEV, torch.bfloat16), return_dict=False, id_frames=1)[0]
    for i in range(2):
        assert torch.equal(both[i:i + 1], _fwd(m, x, txt[i:i + 1], id_frames=1)), i


def test_first_block_caching_keeps_working(setup):
    from frameino_amd.step_cache import FirstBlockCacheConfig
    sd, _, x, txt = setup[:4]
    want = _fwd(_model(sd, window_frames=1), x, txt[:1], id_frames=1)
    m = _model(sd, window_frames=1)
    m.enable_cache(FirstBlockCacheConfig(threshold=0.05))
    with m.cache_context("c"):
        assert torch.equal(_fwd(m, x, txt[:1], id_frames=1), want)           # the first forward always computes
        again = _fwd(m, x, txt[:1], id_frames=1)                             # unchanged input: skips the tail blocks
    assert [e[3] for e in m.cache_log] == [True, False] and rel_rms(again, want) < BOUND


def test_the_timestep_range_and_its_log(setup):
    sd, _, x, txt = setup[:4]
    clock = {"t": 999.0}
    dense, windowed = _model(sd), _model(sd, window_frames=1)
    m = _model(sd, window_frames=1, timestep_range=(100, 800), current_timestep_callback=lambda: clock["t"])
    seen = []
    for t in (999.0, 800.0, 500.0, 100.0, 50.0):                             # (800 and 100: the bounds are strict)
        clock["t"] = t
        ts = torch.tensor([t])
        out = _fwd(m, x, txt[:1], ts, id_frames=1)
        on = 100 < t < 800
        assert torch.equal(out, _fwd(windowed if on else dense, x, txt[:1], ts, id_frames=1)), t
        seen.append(on)
    assert m.window_attention_log == [(i, t, on) for i, (t, on) in enumerate(zip((999.0, 800.0, 500.0, 100.0, 50.0), seen))]
    assert seen == [False, False, True, False, False]


def test_refusals(setup):
    from frameino_amd.attention_processor import MI355WanAttnProcessor
    from frameino_amd.step_cache import PyramidAttentionBroadcastConfig
    sd, _, x, txt = setup[:4]
    cfg = WindowAttentionConfig(window_frames=1)
    m = _model(sd)
    m.enable_fp8_attention()
    with pytest.raises(NotImplementedError, match="fp8 attention"):
        m.enable_window_attention(cfg)
    m.enable_fp8_attention(False)
    m.enable_cache(PyramidAttentionBroadcastConfig(spatial_attention_block_skip_range=2, current_timestep_callback=lambda: 500))
    with pytest.raises(NotImplementedError, match="Pyramid Attention Broadcast"):
        m.enable_window_attention(cfg)
    m.disable_cache()
    m.enable_window_attention(cfg)
    with pytest.raises(NotImplementedError, match="fp8 attention"):
        m.enable_fp8_attention()
    with pytest.raises(NotImplementedError, match="Pyramid Attention Broadcast"):
        m.enable_cache(PyramidAttentionBroadcastConfig(spatial_attention_block_skip_range=2, current_timestep_callback=lambda: 500))
    # what can only be seen by the forward: a processor installed afterwards, a shard passed to the call
    class Mine(MI355WanAttnProcessor):
        pass

    m.blocks[0].attn1.set_processor(Mine())
    with pytest.raises(NotImplementedError, match="attention processor"):
        _fwd(m, x, txt[:1], id_frames=1)
    m.blocks[0].attn1.set_processor(MI355WanAttnProcessor())
    m.parallel = type("Shard", (), {"active": True, "rows": lambda self, n: (0, n, n), "gemm_tile_m": 0})()
    with pytest.raises(NotImplementedError, match="token-sharded"):
        _fwd(m, x, txt[:1], id_frames=1)
    m.parallel = None
    with pytest.raises(ValueError, match="id_frames"):
        _fwd(m, x, txt[:1], id_frames=FRAMES)
    assert _fwd(m, x, txt[:1], id_frames=1).shape == (1, 8, FRAMES, 18, 22)
