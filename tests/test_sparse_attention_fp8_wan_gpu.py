"""Sparse attention with fp8 attention on the Wan DiT: the model, geometry, inputs and restatement of
tests/test_sparse_attention_wan_gpu.py (4 heads x 128, 2 blocks, 1188 rows: five q-blocks, 19 key tiles, the last frame an ID frame)
with `enable_fp8_attention()` on top of `enable_sparse_attention(keep_masks=True)`.  The masks are predicted from the bf16 q and k;
the walk over them runs on the fp8 operands (ops.attention_fp8_tiles).

The forward is compared with the float restatement under the masks the model kept.  Bound: 1.5 x the error the dense fp8 forward
(no sparse attention: the code path of before) shows against the dense restatement, measured in the same test on the same weights
-- the margin covers the different key subset, it is not a tuned number.  The dense fall-backs equal the dense fp8 forward bit for
bit."""
import pytest
import torch

from frameino_amd.window_attention import SparseAttentionConfig
from tests.parity import record, rel_rms
from tests.test_sparse_attention_wan_gpu import _masks, _model, setup  # noqa: F401  (the fixture: weights that separate sparse from dense)
from tests.test_window_attention_wan_gpu import CFG, TS, _fwd
from tests.window_attn_ref import window_forward

pytestmark = pytest.mark.gpu
MARGIN = 1.5


def _fp8_model(sd, fp8=None, sparse=True, **cfg):
    m = _model(sd, sparse=sparse, **cfg)
    m.enable_fp8_attention(**(fp8 or {}))
    return m


@pytest.fixture(scope="module")
def dense_fp8(setup):  # noqa: F811
    """the dense fp8 forward (default options) and its error against the dense restatement"""
    sd, _, x, txt, dense = setup[:5]
    out = _fwd(_fp8_model(sd, sparse=False), x, txt[:1])
    return out, rel_rms(out, dense)


@pytest.mark.parametrize("fp8", [{}, dict(smooth_k=True, smooth_v=True)], ids=["plain", "smooth-k-v"])
def test_fp8_sparse_forward_matches_the_restatement_under_its_own_masks(setup, dense_fp8, fp8):  # noqa: F811
    sd, sdb, x, txt, dense = setup[:5]
    base = dense_fp8[1]
    if fp8:
        base = rel_rms(_fwd(_fp8_model(sd, fp8, sparse=False), x, txt[:1]), dense)                  # the dense forward with these flags
    m = _fp8_model(sd, fp8, cdf_threshold=0.5)
    assert m.fp8_attention and m.is_sparse_attention_enabled
    out = _fwd(m, x, txt[:1], id_frames=1)
    dens = m.sparse_attention_density()
    print(f"densities {dens}")
    assert sorted(dens) == [0, 1] and all(0.0 < d < 1.0 for d in dens.values())
    want = window_forward(sdb, CFG, x.bfloat16(), TS, txt[:1].bfloat16(), _masks(m))
    err, far = rel_rms(out, want), rel_rms(out, dense)
    print(f"fp8 {fp8} + sparse forward: rel-RMS {err:.3e} against the restatement under its masks (dense fp8 forward against the "
          f"dense restatement: {base:.3e}; bound {MARGIN} x), {far:.3e} against the dense restatement")
    record(f"wan_sparse_attention_fp8[tiny, {fp8 or 'plain'}, dense fp8 forward vs dense restatement]", "rel_rms", base, 1.0)
    record(f"wan_sparse_attention_fp8[tiny, {fp8 or 'plain'}]", f"rel_rms vs the restatement under the kept masks (bound: {MARGIN} x "
           f"{base:.3e})", err, MARGIN * base)
    assert torch.isfinite(out.float()).all() and err < MARGIN * base, (err, base)
    assert far > err                                         # (it walks its masks: closer to their restatement than to the dense one)
    assert torch.equal(_fwd(m, x, txt[:1], id_frames=1), out)                                        # deterministic
    # the fp8 walk, not the bf16 one, and not the dense fp8 forward
    assert not torch.equal(out, setup[8]) and not torch.equal(out, dense_fp8[0])


def test_dense_fall_backs_are_the_dense_fp8_forward_bit_for_bit(setup, dense_fp8):  # noqa: F811
    sd, _, x, txt = setup[:4]
    want = dense_fp8[0]
    m = _fp8_model(sd, cdf_threshold=1.0)
    assert torch.equal(_fwd(m, x, txt[:1], id_frames=1), want) and m.sparse_attention_masks == {}
    m.disable_sparse_attention()
    m.enable_sparse_attention(SparseAttentionConfig(0.5, skip_layers=(0, 1), keep_masks=True))       # every layer skipped
    assert torch.equal(_fwd(m, x, txt[:1], id_frames=1), want) and m.sparse_attention_masks == {}
    m.disable_sparse_attention()
    m.enable_sparse_attention(SparseAttentionConfig(0.5, head_thresholds={0: (1.0,) * 4, 1: (1.0,) * 4}))    # all-dense layers
    assert torch.equal(_fwd(m, x, txt[:1], id_frames=1), want)
    m.disable_sparse_attention()
    m.enable_sparse_attention(SparseAttentionConfig(0.5, skip_layers=(1,), keep_masks=True))         # one layer skipped: sparse
    out = _fwd(m, x, txt[:1], id_frames=1)
    assert sorted(m.sparse_attention_masks) == [0] and not torch.equal(out, want)
    m.disable_sparse_attention()                                                                    # ... and off again
    assert torch.equal(_fwd(m, x, txt[:1], id_frames=1), want)
