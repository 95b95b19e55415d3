"""The similarity gate and the per-head thresholds of the sparse attention on the Wan DiT and through the
FrameINO Wan denoise loop.  Model, geometry, inputs, restatement and tolerance are those of tests/test_sparse_attention_wan_gpu.py
(4 heads x 128, 2 blocks, 12 latent frames of 99 tokens, the last an ID frame; rel-RMS < 1.5e-2 against tests/window_attn_ref.py
under the masks the model kept); the pipeline is the one of tests/test_sparse_attention_pipeline_gpu.py.  What the masks must be is
pinned by tests/test_attention_tile_plan_gated_gpu.py; held here is that the model's host path hands the two settings to the
predictor layer by layer and walks what it predicts."""
import pytest
import torch

from frameino_amd.window_attention import SparseAttentionConfig
from tests.parity import rel_rms
from tests.sparse_attn_ref import unpack_mask
from tests.test_sparse_attention_wan_gpu import NT, _masks, _model
from tests.test_window_attention_wan_gpu import BOUND, CFG, TS, _fwd, _inputs
from tests.window_attn_ref import window_forward

pytestmark = pytest.mark.gpu
HEADS = CFG["num_attention_heads"]
# this model's blocks have a mean pairwise cosine of 0.13 .. 0.29 (q-blocks of layer 0) and 0.21 .. 0.61 (its key tiles): theta
# sits in a gap of both lists (nearest values 0.213 / 0.251 and 0.217 / 0.230), so that the gate fires on some blocks, not on all
THETA = 0.2235
PIPE_THETA = 0.65


class _CountPlans:
    """counts the plan launches of a model's forwards"""

    def __init__(self, m):
        self.m, self.n, self.kw = m, 0, []

    def __enter__(self):
        real = self.m.ops.attention_tile_plan

        def counted(*a, **kw):
            self.n += 1
            self.kw.append(sorted(set(kw) & {"cdf_heads", "similarity_threshold"}))
            return real(*a, **kw)

        self.real, self.ops = real, self.m.ops
        self.m.ops = type("Ops", (), {"__getattr__": lambda s, n: getattr(self.ops, n)})()
        self.m.ops.__dict__["attention_tile_plan"] = counted
        return self

    def __exit__(self, *exc):
        self.m.ops = self.ops


@pytest.fixture(scope="module")
def setup():
    sd, sdb, x, txt = _inputs(4.0)
    return sd, sdb, x, txt


def test_gated_forward_with_head_thresholds_matches_the_restatement_under_its_masks(setup):
    sd, sdb, x, txt = setup
    table = {0: (0.5, 0.9, 1.0, 0.3), 1: (1.0, 1.0, 1.0, 1.0)}
    m = _model(sd, cdf_threshold=0.5, similarity_threshold=THETA, head_thresholds=table)
    with _CountPlans(m) as c:
        out = _fwd(m, x, txt[:1], id_frames=1)
    assert c.n == 1 and c.kw == [["cdf_heads", "similarity_threshold"]]                    # layer 1 is all >= 1: no plan launch
    assert sorted(m.sparse_attention_masks) == [0]
    keep = unpack_mask(m.sparse_attention_masks[0], NT)
    assert bool(keep[:, 2].all()) and not bool(keep[:, 0].all())                            # the head at 1.0 has full rows
    want = window_forward(sdb, CFG, x.bfloat16(), TS, txt[:1].bfloat16(), _masks(m))
    dense = window_forward(sdb, CFG, x.bfloat16(), TS, txt[:1].bfloat16(), {})
    err, far = rel_rms(out, want), rel_rms(out, dense)
    print(f"gate + head thresholds: rel-RMS {err:.3e} against the restatement under the model's masks, {far:.3e} against dense")
    assert err < BOUND
    sims = m.sparse_attention_similarity()
    print(f"similarity per layer (mean sim_q, mean sim_k, share of q-blocks, of key tiles under theta = {THETA}): {sims}")
    assert sorted(sims) == [0] and all(0.0 <= v <= 1.0 for v in sims[0])
    assert 0.0 < sims[0][2] < 1.0 and 0.0 < sims[0][3] < 1.0                                # the gate fired somewhere, not everywhere
    assert sorted(m.sparse_attention_density()) == [0]
    # deterministic
    again = _fwd(m, x, txt[:1], id_frames=1)
    assert torch.equal(again, out)
    # the gate alone, every layer: the restatement under its masks again; a gate that fires everywhere is the dense forward
    m2 = _model(sd, cdf_threshold=0.5, similarity_threshold=THETA)
    with _CountPlans(m2) as c:
        out2 = _fwd(m2, x, txt[:1], id_frames=1)
    assert c.n == 2 and c.kw == [["similarity_threshold"]] * 2
    want2 = window_forward(sdb, CFG, x.bfloat16(), TS, txt[:1].bfloat16(), _masks(m2))
    assert rel_rms(out2, want2) < BOUND
    m3 = _model(sd, cdf_threshold=0.5, similarity_threshold=1.0)                             # no block reaches a mean cosine of 1
    assert rel_rms(_fwd(m3, x, txt[:1], id_frames=1), dense) < BOUND                        # (the tile walk over every tile)
    assert sorted(m3.sparse_attention_masks) == [0, 1]
    assert all(bool(unpack_mask(mk, NT).all()) for mk in m3.sparse_attention_masks.values())
    assert all(v[2:] == (1.0, 1.0) for v in m3.sparse_attention_similarity().values())


def test_a_uniform_table_without_a_gate_is_the_plain_config_bit_for_bit(setup):
    sd, _, x, txt = setup
    plain = _model(sd, cdf_threshold=0.5)
    want = _fwd(plain, x, txt[:1], id_frames=1)
    m = _model(sd, cdf_threshold=0.5, head_thresholds={li: (0.5,) * HEADS for li in range(CFG["num_layers"])})
    with _CountPlans(m) as c:
        got = _fwd(m, x, txt[:1], id_frames=1)
    assert c.kw == [["cdf_heads"]] * 2
    assert torch.equal(got, want)
    assert all(torch.equal(m.sparse_attention_masks[li], plain.sparse_attention_masks[li]) for li in (0, 1))
    # only one layer named: the other uses the scalar through the old entry
    m = _model(sd, cdf_threshold=0.5, head_thresholds={1: (0.5,) * HEADS})
    with _CountPlans(m) as c:
        got = _fwd(m, x, txt[:1], id_frames=1)
    assert c.kw == [[], ["cdf_heads"]] and torch.equal(got, want)
    # cdf_threshold >= 1 with a table: the layers it does not name are dense
    m = _model(sd, cdf_threshold=1.0, head_thresholds={1: (0.5,) * HEADS})
    with _CountPlans(m) as c:
        got = _fwd(m, x, txt[:1], id_frames=1)
    assert c.n == 1 and sorted(m.sparse_attention_masks) == [1] and not torch.equal(got, want)
    skip0 = _model(sd, cdf_threshold=0.5, skip_layers=(0,))
    assert torch.equal(got, _fwd(skip0, x, txt[:1], id_frames=1))


def test_the_graph_loop_equals_the_eager_loop_with_both_fields_set(golden):
    from tests.test_window_attention_pipeline_gpu import _pipe
    pipe, args = _pipe(golden)
    tr = pipe.transformer
    heads, layers = tr.config.num_attention_heads, len(tr.blocks)
    assert heads >= 2 and layers >= 2
    row = tuple(0.5 if h % 2 else 0.8 for h in range(heads - 1)) + (1.0,)
    cfg = SparseAttentionConfig(0.5, keep_masks=True, similarity_threshold=PIPE_THETA,
                                head_thresholds={li: row for li in range(layers - 1)})
    pipe.use_hip_graph = False
    dense = pipe.denoise(*args)
    tr.enable_sparse_attention(cfg)
    eager = pipe.denoise(*args)
    masks = {li: mk.clone() for li, mk in tr.sparse_attention_masks.items()}
    sims = tr.sparse_attention_similarity()
    print(f"densities {tr.sparse_attention_density()}; similarity {sims}")
    assert sorted(sims) == list(range(layers)) and any(k[0] == "sparse_cdf" for k in tr._rope_cache)
    pipe.use_hip_graph = True                                          # a failed capture is an error
    graphed = pipe.denoise(*args)
    assert torch.equal(eager, graphed)
    assert all(torch.equal(masks[li], tr.sparse_attention_masks[li]) for li in masks)
    assert torch.isfinite(eager).all() and not torch.equal(eager, dense)
    pipe.use_hip_graph = None                                          # the default: still the graph loop
    assert torch.equal(pipe.denoise(*args), eager)
    tr.reset_caches()
    assert not any(k[0] == "sparse_cdf" for k in tr._rope_cache)
