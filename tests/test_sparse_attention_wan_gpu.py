"""Dynamic block-sparse self-attention on the Wan DiT (WanTransformer3DModel.enable_sparse_attention) against the restatement
in tests/window_attn_ref.py run under the per-head boolean masks expanded from the masks the model kept
(`model.sparse_attention_masks`, `keep_masks=True`): what is held here is the model's host path and the tile walk -- that every
block attends exactly the tiles of its mask.  The predictor that makes the masks is pinned by
tests/test_attention_tile_plan_gpu.py.  Model, geometry, inputs and tolerance are those of tests/test_window_attention_wan_gpu.py:
4 heads x 128, 2 blocks, 12 latent frames of 99 tokens (1188 rows, five q-blocks, the last ragged, 19 key tiles), the last frame
an ID frame, rel-RMS < 1.5e-2; cdf_threshold = 0.5, window_frames = 0."""
import pytest
import torch

from frameino_amd.window_attention import SparseAttentionConfig, frame_window_ranges, ranges_density
from tests.parity import hip_wan_model, rel_rms
from tests.sparse_attn_ref import expand_mask, unpack_mask
from tests.test_window_attention_wan_gpu import BOUND, CFG, DEV, FRAMES, L, SINKS, TPF, TS, _fwd, _inputs
from tests.window_attn_ref import window_forward

pytestmark = pytest.mark.gpu
NT = -(-L // 64)
FORCED = ranges_density(frame_window_ranges(FRAMES, TPF, 0, SINKS), L)


def _model(sd, sparse=True, **cfg):
    m = hip_wan_model(CFG, sd, DEV)
    if sparse:
        m.enable_sparse_attention(SparseAttentionConfig(**{"cdf_threshold": 0.5, "window_frames": 0, "keep_masks": True, **cfg}))
    return m


def _masks(m, live_rows=None):
    """{layer: bool [heads, L, L]} from the masks the model kept (a layer without one: dense).  Under `live_rows` the last
    block's mask covers the live query rows only; its other rows are not queries (left dense: never compared)."""
    out = {}
    for li, mk in m.sparse_attention_masks.items():
        keep = unpack_mask(mk, NT)
        assert keep.shape[0] == 1 and keep.shape[1] == CFG["num_attention_heads"]
        if live_rows is not None and keep.shape[2] != -(-L // 256):
            s0, s1 = live_rows
            full = torch.ones(keep.shape[1], L, L, dtype=torch.bool)
            full[:, s0:s1] = expand_mask(keep, s1 - s0, L)[0]
            out[li] = full
        else:
            out[li] = expand_mask(keep, L, L)[0]
    return out


@pytest.fixture(scope="module")
def setup():
    """inputs on which the restatement under the model's masks and the dense restatement differ by at least 5 x BOUND:
    otherwise no assertion below could tell a tile walk from none.  The value projection is scaled until they do (the scaling
    of tests/test_window_attention_wan_gpu.py)."""
    for v_scale in (4.0, 8.0, 16.0):
        sd, sdb, x, txt = _inputs(v_scale)
        m = _model(sd, cdf_threshold=0.5)
        out = _fwd(m, x, txt[:1], id_frames=1)
        masks = _masks(m)
        dense = window_forward(sdb, CFG, x.bfloat16(), TS, txt[:1].bfloat16(), {})
        sparse = window_forward(sdb, CFG, x.bfloat16(), TS, txt[:1].bfloat16(), masks)
        gap = rel_rms(sparse, dense)
        print(f"restatement: sparse vs dense rel-RMS {gap:.3e} at value scale {v_scale} (needs >= {5 * BOUND:.3e})")
        if gap >= 5 * BOUND:
            return sd, sdb, x, txt, dense, sparse, gap, m, out
    raise AssertionError(f"no scale separates the sparse from the dense model: last gap {gap}")


def test_sparse_forward_matches_the_restatement_under_its_own_masks(setup):
    sd, sdb, x, txt, dense, sparse, gap, m, out = setup
    err, far = rel_rms(out, sparse), rel_rms(out, dense)
    print(f"sparse forward: rel-RMS {err:.3e} against the restatement under its masks, {far:.3e} against the dense restatement")
    assert err < BOUND
    assert far > 3 * BOUND                                   # (and so it is not the dense model)
    dens = m.sparse_attention_density()
    print(f"densities {dens}; forced {FORCED:.3f}")
    assert sorted(dens) == [0, 1] and all(FORCED < d < 1.0 for d in dens.values())
    for li, mk in m.sparse_attention_masks.items():          # every forced tile is in every head's mask
        keep = unpack_mask(mk, NT)
        for i, blk in enumerate(frame_window_ranges(FRAMES, TPF, 0, SINKS).tolist()):
            for a, b in blk:
                assert bool(keep[:, :, i, a:b].all()), (li, i, a, b)
    assert not torch.equal(keep[0, 0], keep[0, 1]) or not torch.equal(keep[0, 0], keep[0, 2])      # the heads differ
    # the dense model on the same weights is within the bound of the DENSE restatement
    assert rel_rms(_fwd(_model(sd, sparse=False), x, txt[:1]), dense) < BOUND
    # deterministic: the same forward again, the same bits and the same masks
    before = {li: mk.clone() for li, mk in m.sparse_attention_masks.items()}
    assert torch.equal(_fwd(m, x, txt[:1], id_frames=1), out)
    assert all(torch.equal(before[li], m.sparse_attention_masks[li]) for li in before)


def test_dense_settings_are_the_dense_forward_bit_for_bit(setup):
    sd, _, x, txt = setup[:4]
    want = _fwd(_model(sd, sparse=False), x, txt[:1])
    m = _model(sd, cdf_threshold=1.0)
    assert torch.equal(_fwd(m, x, txt[:1], id_frames=1), want) and m.sparse_attention_masks == {}
    m.disable_sparse_attention()
    m.enable_sparse_attention(SparseAttentionConfig(0.5, skip_layers=(0, 1), keep_masks=True))       # every layer dense
    assert torch.equal(_fwd(m, x, txt[:1], id_frames=1), want) and m.sparse_attention_masks == {}
    m.disable_sparse_attention()
    m.enable_sparse_attention(SparseAttentionConfig(0.5, window_frames=FRAMES))                      # forced tiles cover all
    assert torch.equal(_fwd(m, x, txt[:1], id_frames=1), want)
    m.disable_sparse_attention()
    m.enable_sparse_attention(SparseAttentionConfig(0.5))
    assert not torch.equal(_fwd(m, x, txt[:1], id_frames=1), want)
    m.disable_sparse_attention()                                                                    # ... and off again
    assert torch.equal(_fwd(m, x, txt[:1], id_frames=1), want) and not m.is_sparse_attention_enabled


@pytest.mark.parametrize("skip", [(0,), (1,)])
def test_skip_layers_stay_dense(setup, skip):
    sd, sdb, x, txt = setup[:4]
    m = _model(sd, skip_layers=skip)
    out = _fwd(m, x, txt[:1], id_frames=1)
    assert sorted(m.sparse_attention_masks) == [1 - skip[0]]
    want = window_forward(sdb, CFG, x.bfloat16(), TS, txt[:1].bfloat16(), _masks(m))
    err = rel_rms(out, want)
    print(f"skip_layers {skip}: rel-RMS {err:.3e} against the restatement")
    assert err < BOUND
    assert not torch.equal(out, setup[8])


def test_live_rows_match_the_restatement(setup):
    """the last block's queries start at the first live row: its q-blocks, forced tiles and mask rows are counted from there"""
    sd, sdb, x, txt = setup[:4]
    live = (TPF, (FRAMES - 1) * TPF)                                        # the caller drops the first frame and the ID frame
    m = _model(sd)
    out = _fwd(m, x, txt[:1], id_frames=1, live_rows=live)
    assert m.sparse_attention_masks[1].shape[2] == -(-(live[1] - live[0]) // 256) and m.sparse_attention_masks[0].shape[2] == 5
    want = window_forward(sdb, CFG, x.bfloat16(), TS, txt[:1].bfloat16(), _masks(m, live))
    err = rel_rms(out[:, :, 1:FRAMES - 1], want[:, :, 1:FRAMES - 1])
    print(f"live rows: rel-RMS {err:.3e} against the restatement")
    assert err < BOUND
    assert float(out[:, :, 0].abs().max()) == 0.0 and float(out[:, :, FRAMES - 1].abs().max()) == 0.0
    assert any(k[0] == "sparse" and k[5] == live for k in m._rope_cache)     # (the forced table of the live query rows was built)
    m.reset_caches()
    assert not any(k[0] == "sparse" for k in m._rope_cache)


def test_the_cfg_batch_with_the_shared_prefix_equals_two_single_calls(setup):
    sd, _, x, txt = setup[:4]
    m = _model(sd)
    xd = x.to(DEV, torch.bfloat16)
    both = m(xd.expand(2, -1, -1, -1, -1), TS.to(DEV), txt.to(DEV, torch.bfloat16), return_dict=False, id_frames=1)[0]
    assert m.sparse_attention_masks[0].shape[0] == 1 and m.sparse_attention_masks[1].shape[0] == 2      # layer 0 ran once
    for i in range(2):
        assert torch.equal(both[i:i + 1], _fwd(m, x, txt[i:i + 1], id_frames=1)), i


def test_first_block_caching_keeps_working(setup):
    from frameino_amd.step_cache import FirstBlockCacheConfig
    sd, _, x, txt = setup[:4]
    want = setup[8]
    m = _model(sd)
    m.enable_cache(FirstBlockCacheConfig(threshold=0.05))
    with m.cache_context("c"):
        assert torch.equal(_fwd(m, x, txt[:1], id_frames=1), want)           # the first forward always computes
        again = _fwd(m, x, txt[:1], id_frames=1)                             # unchanged input: skips the tail blocks
    assert [e[3] for e in m.cache_log] == [True, False] and rel_rms(again, want) < BOUND


def test_forward_time_refusals(setup):
    from frameino_amd.attention_processor import MI355WanAttnProcessor
    sd, _, x, txt = setup[:4]
    m = _model(sd)

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
    assert torch.equal(_fwd(m, x, txt[:1], id_frames=1), setup[8])
