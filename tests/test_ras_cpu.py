"""Region-adaptive sampling without a GPU: the rule (`ras_decide`) against a hand-written table, the config with its validation
and refusals in both orders, the C ABI's new symbols and their argument checks, the forward's dispatch over a recording stand-in
for `ops` (tests/cpu_ops.py plus the five new entries in plain torch), its agreement with the restatement in tests/ras_ref.py,
and the properties of the fixtures the GPU tests share with this file."""
import math

import pytest
import torch

from frameino_amd import _lib
from frameino_amd import step_cache as S
from frameino_amd.step_cache import FirstBlockCacheConfig, RegionAdaptiveSamplingConfig, ras_active_count, ras_decide
from oracle import wan_dit as W
from tests import cpu_ops
from tests import ras_ref as R
from tests.test_fastercache_cpu import _Shard, _first_next, _tiny_model
from tests.test_step_cache_cpu import _pipe

F, P = True, False              # full / partial


# ------------------------------------------------------------------ the rule
def test_the_schedule_of_the_defaults():
    cfg = RegionAdaptiveSamplingConfig()
    got = [ras_decide(s, cfg) for s in range(50)]
    # warm-up 0 .. 3; every fifth forward counted from forward 3: 8, 13, ..., 43; the last two: 48 (also on the grid), 49
    full = {0, 1, 2, 3, 8, 13, 18, 23, 28, 33, 38, 43, 48, 49}
    assert got == [s in full for s in range(50)] and sum(got) == 14
    assert all(isinstance(v, bool) for v in got)
    assert all(ras_decide(s, cfg, has_cache=False) for s in range(50))             # no planes yet: full, whatever the counter
    assert all(ras_decide(s, cfg) for s in range(50, 60))                          # past the call's steps: full


def test_other_schedules_and_a_ratio_of_one():
    cfg = RegionAdaptiveSamplingConfig(warmup_steps=2, full_step_interval=3, full_steps_at_end=2, num_inference_steps=10)
    assert [ras_decide(s, cfg) for s in range(10)] == [F, F, P, P, F, P, P, F, F, F]
    cfg = RegionAdaptiveSamplingConfig(warmup_steps=1, full_step_interval=1, full_steps_at_end=0, num_inference_steps=6)
    assert all(ras_decide(s, cfg) for s in range(6))
    cfg = RegionAdaptiveSamplingConfig(warmup_steps=1, full_step_interval=100, full_steps_at_end=0, num_inference_steps=6)
    assert [ras_decide(s, cfg) for s in range(6)] == [F, P, P, P, P, P]
    cfg = RegionAdaptiveSamplingConfig(sample_ratio=1.0)
    assert all(ras_decide(s, cfg) for s in range(50))
    assert ras_active_count(0.4, 1188) == R.LIST_ROWS and ras_active_count(0.5, 1188) == 594 and ras_active_count(1e-9, 1188) == 1
    assert ras_active_count(0.25, 990) == 248                                      # round(247.5): Python's round, half to even


# ------------------------------------------------------------------ config
def test_defaults():
    c = RegionAdaptiveSamplingConfig()
    assert (c.sample_ratio, c.full_step_interval, c.warmup_steps, c.full_steps_at_end, c.num_inference_steps, c.starvation_scale,
            c.always_active) == (0.5, 5, 4, 2, 50, 0.1, None)


@pytest.mark.parametrize("bad", [dict(sample_ratio=0.0), dict(sample_ratio=1.01), dict(sample_ratio=-0.5), dict(sample_ratio="x"),
                                 dict(sample_ratio=True), dict(full_step_interval=0), dict(full_step_interval=2.0),
                                 dict(warmup_steps=0), dict(warmup_steps=None), dict(full_steps_at_end=-1),
                                 dict(num_inference_steps=0), dict(starvation_scale=-0.1), dict(starvation_scale=float("inf")),
                                 dict(always_active=[True, False]), dict(always_active=torch.zeros(4)),
                                 dict(always_active=torch.zeros(2, 2, dtype=torch.bool))],
                         ids=lambda b: "-".join(f"{k}={v if not isinstance(v, torch.Tensor) else tuple(v.shape)}" for k, v in b.items()))
def test_bad_values_raise_and_name_the_field(bad):
    m = _tiny_model()
    with pytest.raises(ValueError, match=next(iter(bad))):
        m.enable_cache(RegionAdaptiveSamplingConfig(**bad))
    assert not m.is_cache_enabled


def test_a_duck_typed_config_and_a_bare_name():
    class RegionAdaptiveSamplingConfig:                          # noqa: F811
        sample_ratio, full_step_interval, warmup_steps, full_steps_at_end = 0.5, 5, 4, 2
        num_inference_steps, starvation_scale, always_active = 50, 0.1, None

    m = _tiny_model()
    m.enable_cache(RegionAdaptiveSamplingConfig())
    assert m._ras_on and not m._mag_on and not m._pab_on
    m.disable_cache()

    class Bare:
        pass
    Bare.__name__ = "RegionAdaptiveSamplingConfig"
    with pytest.raises(NotImplementedError, match="RegionAdaptiveSamplingConfig.*`sample_ratio`.*`always_active`"):
        m.enable_cache(Bare())


def test_the_policy_and_its_refusals_in_both_orders():
    from frameino_amd.attention_processor import MI355WanAttnProcessor
    from frameino_amd.window_attention import SparseAttentionConfig, WindowAttentionConfig
    policy = S._POLICIES["RegionAdaptiveSamplingConfig"]
    assert policy is S._RegionAdaptivePolicy and policy in S.StepCacheMixin._cache_policies
    assert policy not in S.PyramidAttentionBroadcastMixin._cache_policies
    assert policy.batched and "use_hip_graph=True with region-adaptive sampling" in str(policy.capture_refusal())
    cfg = RegionAdaptiveSamplingConfig()
    m = _tiny_model()
    # window attention
    m.enable_window_attention(WindowAttentionConfig(1))
    with pytest.raises(NotImplementedError, match="region-adaptive sampling with window attention"):
        m.enable_cache(cfg)
    assert not m.is_cache_enabled
    m.disable_window_attention()
    m.enable_cache(cfg)
    with pytest.raises(NotImplementedError, match="window attention.*with region-adaptive sampling"):
        m.enable_window_attention(WindowAttentionConfig(1))
    assert not m.is_window_attention_enabled
    # sparse attention
    with pytest.raises(NotImplementedError, match="sparse attention.*with region-adaptive sampling"):
        m.enable_sparse_attention(SparseAttentionConfig(0.5))
    m.disable_cache()
    m.enable_sparse_attention(SparseAttentionConfig(0.5))
    with pytest.raises(NotImplementedError, match="region-adaptive sampling with sparse attention"):
        m.enable_cache(cfg)
    m.disable_sparse_attention()
    # fp8 attention
    m.enable_fp8_attention()
    with pytest.raises(NotImplementedError, match="region-adaptive sampling with fp8 attention"):
        m.enable_cache(cfg)
    m.enable_fp8_attention(False)
    m.enable_cache(cfg)
    with pytest.raises(NotImplementedError, match="fp8 attention.*with region-adaptive sampling"):
        m.enable_fp8_attention()
    assert not m.fp8_attention
    # a second cache
    with pytest.raises(ValueError, match="already been enabled"):
        m.enable_cache(FirstBlockCacheConfig())
    m.disable_cache()
    m.enable_cache(FirstBlockCacheConfig())
    with pytest.raises(ValueError, match="already been enabled"):
        m.enable_cache(cfg)
    m.disable_cache()
    # a token-sharded plan: on the model at enable time, or handed to the forward (refused before any launch)
    m.parallel = _Shard()
    with pytest.raises(NotImplementedError, match="region-adaptive sampling with a token-sharded plan.*one GPU"):
        m.enable_cache(cfg)
    m.parallel = None
    m.enable_cache(cfg)
    with m.cache_context("c"), pytest.raises(NotImplementedError, match="one GPU"):
        _first_next(m, shard=_Shard())
    assert m.cache_log == () or m.cache_log == []                # refused before the forward counted
    m.disable_cache()

    # a user-installed processor
    class Mine(MI355WanAttnProcessor):
        pass

    m.blocks[1].attn1.set_processor(Mine())
    with pytest.raises(NotImplementedError, match="region-adaptive sampling with a user-installed attention processor"):
        m.enable_cache(cfg)
    m.blocks[1].attn1.set_processor(MI355WanAttnProcessor())
    m.enable_cache(cfg)
    m.blocks[0].attn2.set_processor(Mine())
    with m.cache_context("c"), pytest.raises(NotImplementedError, match="attention processor"):
        _first_next(m)
    assert m.cache_log == () or m.cache_log == []
    m.blocks[0].attn2.set_processor(MI355WanAttnProcessor())
    m.disable_cache()
    # the test hook belongs to this policy
    with pytest.raises(ValueError, match="_active_rows.*region-adaptive sampling"):
        _first_next(m, _active_rows=torch.arange(4))


def test_cogvideox_keeps_refusing_it():
    from frameino_amd.cogvideox_transformer_3d import CogVideoXTransformer3DModel
    m = CogVideoXTransformer3DModel(num_attention_heads=2, attention_head_dim=64, in_channels=4, out_channels=4, num_layers=1,
                                    text_embed_dim=32, time_embed_dim=32, sample_width=8, sample_height=8, sample_frames=5,
                                    use_rotary_positional_embeddings=True)
    with pytest.raises(NotImplementedError, match="RegionAdaptiveSamplingConfig.*PyramidAttentionBroadcastConfig is$"):
        m.enable_cache(RegionAdaptiveSamplingConfig())
    assert not m.is_cache_enabled


def test_pipeline_limits_and_reset():
    pipe = _pipe()
    tr = pipe.transformer
    tr.enable_cache(RegionAdaptiveSamplingConfig())
    assert pipe._step_cache_check(1) is True and pipe._step_cache_check(2) is True        # a batch is allowed
    pipe.use_hip_graph = True
    with pytest.raises(RuntimeError, match="use_hip_graph=True with region-adaptive sampling"):
        pipe._step_cache_check(1)
    pipe.use_hip_graph = None
    pipe.parallel = object()
    with pytest.raises(NotImplementedError, match="region-adaptive sampling runs on one GPU"):
        pipe._step_cache_check(1)
    pipe.parallel = None
    with tr.cache_context("cond"):
        tr._ras_begin(1, 8, 8, 4, torch.bfloat16, "cpu")
    assert tr._step_cache_states and tr.cache_log == [("cond", 0, True, 8)]
    pipe.maybe_free_model_hooks()
    assert tr._step_cache_states == {} and len(tr.cache_log) == 1


# ------------------------------------------------------------------ the state machine
def test_begin_counts_logs_and_shares_one_state_per_call():
    m = _tiny_model()
    m.enable_cache(RegionAdaptiveSamplingConfig(warmup_steps=1, full_step_interval=3, full_steps_at_end=1, num_inference_steps=6,
                                                sample_ratio=0.25))
    with m.cache_context("cfg"):
        plans = []
        for _ in range(6):
            plans.append(m._ras_begin(2, 16, 8, 4, torch.bfloat16, "cpu", ("cond", "uncond")))
            plans[-1].state.valid = True                         # (what the full forward's head leaves)
    assert [p.full for p in plans] == [F, P, P, F, P, F] and [p.rows for p in plans] == [16, 4, 4, 16, 4, 16]
    assert all(p.state is plans[0].state for p in plans) and list(m._step_cache_states) == [("cond", "uncond")]
    assert m.cache_log == [(c, s, f, 16 if f else 4) for s, f in enumerate([F, P, P, F, P, F]) for c in ("cond", "uncond")]
    # rows outside `live_rows` are not eligible and do not count towards La
    m._reset_stateful_cache()
    with m.cache_context("c"):
        p = m._ras_begin(1, 16, 8, 4, torch.bfloat16, "cpu", None, (4, 12))
    assert p.state.eligible.tolist() == [0] * 4 + [1] * 8 + [0] * 4 and ras_active_count(0.25, 8) == 2
    # without planes a forward is full whatever the counter says, and the hook needs them
    with m.cache_context("c"):
        assert m._ras_begin(1, 16, 8, 4, torch.bfloat16, "cpu", None, (4, 12)).full
        with pytest.raises(RuntimeError, match="K / V planes of a full forward"):
            m._ras_begin(1, 16, 8, 4, torch.bfloat16, "cpu", None, (4, 12), torch.arange(3))
        p.state.valid = True
        q = m._ras_begin(1, 16, 8, 4, torch.bfloat16, "cpu", None, (4, 12), torch.arange(3))
    assert not q.full and q.rows == 3 and q.override.dtype == torch.int32
    with m.cache_context("c"), pytest.raises(ValueError, match="_active_rows"):
        m._ras_begin(1, 16, 8, 4, torch.bfloat16, "cpu", None, (4, 12), torch.arange(17))


def test_always_active_pins_rows_and_more_than_la_raises():
    mask = torch.zeros(16, dtype=torch.bool)
    mask[[1, 5, 6]] = True
    m = _tiny_model()
    m.enable_cache(RegionAdaptiveSamplingConfig(sample_ratio=0.25, always_active=mask))
    with m.cache_context("c"):
        p = m._ras_begin(1, 16, 8, 4, torch.bfloat16, "cpu")                       # La = 4 >= 3 pinned rows
        assert p.state.eligible.tolist() == [2 if i in (1, 5, 6) else 1 for i in range(16)] and p.state.n_always == 3
        q = m._ras_begin(1, 16, 8, 4, torch.bfloat16, "cpu", None, (4, 16))        # row 1 is dead: 2 pinned, La = 3
        assert q.state.eligible.tolist() == [0] * 4 + [1, 2, 2] + [1] * 9
    m.disable_cache()
    mask[8:12] = True
    m.enable_cache(RegionAdaptiveSamplingConfig(sample_ratio=0.25, always_active=mask))
    with m.cache_context("c"), pytest.raises(ValueError, match="always_active pins 7 .* La = 4"):
        m._ras_begin(1, 16, 8, 4, torch.bfloat16, "cpu")
    assert m.cache_log == () or m.cache_log == []
    m.disable_cache()
    m.enable_cache(RegionAdaptiveSamplingConfig(always_active=torch.zeros(5, dtype=torch.bool)))
    with m.cache_context("c"), pytest.raises(ValueError, match="always_active has 5 entries"):
        m._ras_begin(1, 16, 8, 4, torch.bfloat16, "cpu")


# ------------------------------------------------------------------ the C ABI
NEW = {"fino_token_score": 11, "fino_token_select": 6, "fino_gather_rows": 9, "fino_scatter_rows": 9,
       "fino_qkv_rmsnorm_rope_rows": 19}


def test_the_new_symbols_are_declared_exported_and_bound():
    lib = _lib.lib()
    for name, nargs in NEW.items():
        assert name in _lib.declared_symbols() and name in _lib.SIGNATURES and hasattr(lib, name)
        assert len(_lib.SIGNATURES[name]) == nargs
    assert lib.fino_version() == 103 == _lib.ABI_VERSION
    from frameino_amd import ops
    assert ops.TOKEN_SELECT_MAX == 65536
    header = open(_lib.HEADER_PATH).read()
    assert "FINO_TOKEN_SELECT_MAX = 65536" in header and "clamped into [0, n)" in header


def test_the_c_abi_checks_before_any_launch():
    lib = _lib.lib()
    a = 4096                                                      # any 16-byte aligned address: nothing is dereferenced
    bad = [
        ("fino_token_select", [a, 65537, 10, a, a, 0], -3, b"above 65536"),
        ("fino_token_select", [a, 100, 0, a, a, 0], -1, b"k=0"),
        ("fino_token_select", [a, 100, 101, a, a, 0], -1, b"k=101"),
        ("fino_token_select", [0, 100, 10, a, a, 0], -1, b"null pointer"),
        ("fino_token_select", [a, 100, 10, 0, a, 0], -1, b"null pointer"),
        ("fino_token_score", [0, 8, 4, 4, 1, a, 0.1, a, a, 0, 0], -1, b"null pointer"),
        ("fino_token_score", [a, 8, 4, 4, 1, a, 0.1, a, a, 2, 0], -1, b"dtype"),
        ("fino_token_score", [a, 0, 4, 4, 1, a, 0.1, a, a, 0, 0], -1, b"rows=0"),
        ("fino_token_score", [a, 8, 4, 3, 1, a, 0.1, a, a, 0, 0], -1, b"ld=3"),
        ("fino_token_score", [a, 8, 4, 4, 0, a, 0.1, a, a, 0, 0], -1, b"batch=0"),
        ("fino_gather_rows", [a, 32, 8, a, 4, 18, a, 32, 0], -1, b"row_bytes=18"),
        ("fino_gather_rows", [a, 16, 8, a, 4, 32, a, 32, 0], -1, b"row stride is below"),
        ("fino_gather_rows", [a, 32, 0, a, 4, 32, a, 32, 0], -1, b"n=0"),
        ("fino_gather_rows", [a + 2, 32, 8, a, 4, 32, a, 32, 0], -1, b"alignment"),
        ("fino_gather_rows", [a, 32, 8, 0, 4, 32, a, 32, 0], -1, b"null pointer"),
        ("fino_scatter_rows", [a, 32, a, 4, 32, a, 32, 0, 0], -1, b"n=0"),
        ("fino_scatter_rows", [a, 32, a, 4, 20, a, 16, 8, 0], -1, b"row stride is below"),
        ("fino_qkv_rmsnorm_rope_rows", [a, 4, 128, 384, a, 1e-6, a, 1e-6, a, a, 64, 1.0, a, 8, 0, a, 128, 0, 0], -1, b"null pointer"),
        ("fino_qkv_rmsnorm_rope_rows", [a, 4, 128, 384, a, 1e-6, a, 1e-6, a, a, 48, 1.0, a, 8, a, a, 128, 0, 0], -1, b"head_dim=48"),
        ("fino_qkv_rmsnorm_rope_rows", [a, 4, 128, 256, a, 1e-6, a, 1e-6, a, a, 64, 1.0, a, 8, a, a, 128, 0, 0], -1, b"row stride"),
        ("fino_qkv_rmsnorm_rope_rows", [a, 4, 128, 384, a, 1e-6, a, 1e-6, a, a, 64, 1.0, a, 8, a, a, 64, 0, 0], -1, b"row stride"),
        ("fino_qkv_rmsnorm_rope_rows", [a, 4, 128, 384, a, 1e-6, a, 1e-6, a, a, 64, 1.0, 0, 2, a, a, 128, 0, 0], -1, b"n=2"),
        ("fino_qkv_rmsnorm_rope_rows", [a, 4, 128, 384, a, 1e-6, a, 1e-6, a, a, 64, 1.0, a, 8, a + 8, a, 128, 0, 0], -1, b"alignment"),
    ]
    for name, args, code, word in bad:
        assert getattr(lib, name)(*args) == code, (name, args)
        err = lib.fino_last_error()
        assert word in err and err.startswith(name.encode()), (name, args, err)


def test_the_ops_check_their_arguments_before_the_library():
    from frameino_amd import ops
    x = torch.zeros(8, 8, dtype=torch.bfloat16)
    idx = torch.zeros(2, dtype=torch.int32)
    for call in (lambda: ops.token_score(x), lambda: ops.gather_rows(x, idx), lambda: ops.scatter_rows(x[:2], idx, x)):
        with pytest.raises((RuntimeError, ValueError), match="no CPU path|device tensor"):
            call()
    with pytest.raises(ValueError, match="device tensor"):
        ops.token_select(torch.zeros(8), 2)


# ------------------------------------------------------------------ the forward over a recording stand-in
class _RasOps:
    """tests/cpu_ops.py plus the five entries of region-adaptive sampling in plain torch; notes every call as
    (name, rows of its first tensor argument) -- an attention call as ("attention", lq, lk)"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(cpu_ops, name)
        if not callable(fn):
            return fn

        def call(*a, **kw):
            first = next((t for t in a if isinstance(t, torch.Tensor)), None)
            if name == "attention":
                self.calls.append((name, a[0].shape[1], a[1].shape[1]))
            elif name == "patchify":
                self.calls.append((name, None))
            else:
                self.calls.append((name, None if first is None else (first.shape[0] if first.dim() == 2 else first.shape[-2])))
            return fn(*a, **kw)
        return call

    def token_score(self, po, batch=1, counters=None, starvation_scale=0.0, eligible=None, out=None):
        self.calls.append(("token_score", po.shape[0]))
        return out.copy_(R.score_ref(po, batch, counters, starvation_scale, eligible).float())

    def token_select(self, score, k, counters=None, out=None):
        self.calls.append(("token_select", score.shape[0]))
        idx, new = R.select_ref(score, k, counters)
        if counters is not None:
            counters.copy_(new)
        return out.copy_(idx)

    def gather_rows(self, src, idx, out=None):
        self.calls.append(("gather_rows", idx.shape[0]))
        rows = src[idx.long().clamp(0, src.shape[0] - 1)]
        return rows if out is None else out.copy_(rows)

    def scatter_rows(self, src, idx, out):
        self.calls.append(("scatter_rows", idx.shape[0]))
        out[idx.long().clamp(0, out.shape[0] - 1)] = src
        return out

    def qkv_rmsnorm_rope_rows_(self, qkv, dim, q_weight, q_eps, k_weight, k_eps, cos, sin, head_dim, idx, kcache, vcache,
                               q_out_scale=1.0):
        self.calls.append(("qkv_rmsnorm_rope_rows_", qkv.shape[0]))
        cpu_ops.qkv_rmsnorm_rope_(qkv, dim, q_weight, q_eps, k_weight, k_eps, cos, sin, head_dim, q_out_scale=q_out_scale)
        rows = torch.arange(qkv.shape[0]) if idx is None else idx.long().clamp(0, kcache.shape[0] - 1)
        kcache[rows] = qkv[:, dim:2 * dim]
        vcache[rows] = qkv[:, 2 * dim:]
        return qkv


CFG = dict(W.WAN22_5B_CFG, num_attention_heads=2, attention_head_dim=64, in_channels=4, out_channels=4, text_dim=32, freq_dim=32,
           ffn_dim=64, num_layers=2)
N = 3 * 4 * 5                   # 3 latent frames of 4 x 5 tokens


def _setup(b=2, **cfg):
    from tests.parity import model_cfg
    from frameino_amd.transformer_wan import WanTransformer3DModel
    sd = W.wan_random_state_dict(CFG, seed=21, dtype=torch.float32, std=0.2)
    m = WanTransformer3DModel(**model_cfg(CFG))
    m.load_reference_state_dict(sd, dtype=torch.float32)
    m.eval()
    m.ops = _RasOps()
    if cfg:
        m.enable_cache(RegionAdaptiveSamplingConfig(**cfg))
    g = torch.Generator().manual_seed(22)
    xs = [torch.randn(b, 4, 3, 8, 10, generator=g) for _ in range(4)]
    txt = torch.randn(b, 6, 32, generator=g)
    ts = torch.tensor([811.0, 650.0][:b])
    return sd, m, xs, txt, ts


def _fwd(m, x, ts, txt, ctxs=("cond", "uncond"), **kw):
    with m.cache_context("cfg"):
        return m(x, ts, txt, return_dict=False, _cache_contexts=ctxs[:x.shape[0]], **kw)[0]


def test_a_full_forward_and_an_all_rows_list_are_the_uncached_forward():
    sd, m, xs, txt, ts = _setup(sample_ratio=0.4, warmup_steps=1, full_step_interval=50)
    plain = _setup()[1]
    want = [plain(x, ts, txt, return_dict=False)[0] for x in xs[:2]]
    assert torch.equal(_fwd(m, xs[0], ts, txt), want[0])
    assert torch.equal(_fwd(m, xs[1], ts, txt, _active_rows=torch.arange(N)), want[1])
    assert m.cache_log == [("cond", 0, F, N), ("uncond", 0, F, N), ("cond", 1, P, N), ("uncond", 1, P, N)]


def test_a_partial_forward_dispatches_on_the_compact_rows_and_matches_the_restatement():
    sd, m, xs, txt, ts = _setup(sample_ratio=0.4, warmup_steps=1, full_step_interval=50)
    la = ras_active_count(0.4, N)
    assert la == 24 and 2 * la != 2 * N
    _, po0, kv0 = R.ras_forward(sd, CFG, xs[0], ts, txt)
    first = _fwd(m, xs[0], ts, txt)
    st = m._step_cache_states[("cond", "uncond")]
    assert torch.equal(st.po.view(2, N, -1), po0) or torch.allclose(st.po.view(2, N, -1), po0, atol=1e-5)
    m.ops.calls.clear()
    out = _fwd(m, xs[1], ts, txt)                                  # forward 1: partial, the model's own list
    calls = m.ops.calls
    # the list: from the kept rows, batch-averaged, one for the call
    want_idx, want_counters = R.select_ref(R.score_ref(po0.reshape(2 * N, -1), 2, torch.zeros(N, dtype=torch.int32), 0.1,
                                                       torch.ones(N, dtype=torch.uint8)), la, torch.zeros(N, dtype=torch.int32))
    assert torch.equal(st.idx, want_idx) and torch.equal(st.counters, want_counters)
    names = [c[0] for c in calls]
    i = names.index("token_score")                               # two launches, before anything that needs the list
    assert calls[i:i + 2] == [("token_score", 2 * N), ("token_select", N)] and names.count("token_score") == 1
    assert i < min(names.index(n_) for n_ in ("patchify", "gather_rows", "gemm"))
    # every self-attention: lq = La against all n rows; the text cross-attention: La queries, 6 keys
    attn = [c for c in calls if c[0] == "attention"]
    assert attn == [("attention", la, N), ("attention", la, 6)] * 2
    # nothing but the embedding's patchify, the moves by the list, the list itself and unpatchify sees n rows
    whole = {"patchify", "unpatchify", "token_score", "token_select"}
    for name, rows in (c[:2] for c in calls):
        if name in whole or name == "attention" or rows is None:
            continue
        assert rows != 2 * N and rows != N, (name, rows)
        if name in ("gemm", "adaln_modulate", "layernorm", "gated_residual", "qkv_rmsnorm_rope_rows_", "gather_rows",
                    "scatter_rows", "rmsnorm_rope_"):
            assert rows in (2 * la, 2 * 6, 12), (name, rows)      # compact rows, or the text rows
    assert sum(1 for c in calls if c[0] == "qkv_rmsnorm_rope_rows_") == 2 and ("scatter_rows", 2 * la) in calls
    assert [c for c in calls if c[0] == "gather_rows"] == [("gather_rows", 2 * la)] * 4      # patches, cos, sin, selector
    # against the restatement: inactive rows keep the first forward's prediction, active rows are the partial forward's
    want, po1, _ = R.ras_forward(sd, CFG, xs[1], ts, txt, want_idx, kv0, po0)
    assert torch.allclose(out, want, atol=2e-5, rtol=1e-4)
    inactive = torch.ones(N, dtype=torch.bool)
    inactive[want_idx.long()] = False
    got_rows = st.po.view(2, N, -1)
    assert torch.equal(got_rows[:, inactive], _rows_of(first)[:, inactive])
    assert not torch.allclose(got_rows[:, ~inactive], po0[:, ~inactive], atol=1e-3)
    assert m.cache_log[-2:] == [("cond", 1, P, la), ("uncond", 1, P, la)]


def _rows_of(pred):
    """a prediction [b, C, F, H, W] back as head rows [b, n, C_out * prod(patch)] (the inverse of unpatchify, patch (1, 2, 2))"""
    b, c, f, h, w = pred.shape
    x = pred.reshape(b, c, f, 1, h // 2, 2, w // 2, 2).permute(0, 2, 4, 6, 3, 5, 7, 1)
    return x.reshape(b, f * (h // 2) * (w // 2), -1)


def test_a_second_partial_forward_uses_the_refreshed_planes_and_counters():
    sd, m, xs, txt, ts = _setup(sample_ratio=0.4, warmup_steps=1, full_step_interval=50)
    la = ras_active_count(0.4, N)
    _, po, kv = R.ras_forward(sd, CFG, xs[0], ts, txt)
    _fwd(m, xs[0], ts, txt)
    counters = torch.zeros(N, dtype=torch.int32)
    elig = torch.ones(N, dtype=torch.uint8)
    for x in xs[1:]:
        idx, counters = R.select_ref(R.score_ref(po.reshape(2 * N, -1), 2, counters, 0.1, elig), la, counters)
        want, po, kv = R.ras_forward(sd, CFG, x, ts, txt, idx, kv, po)
        got = _fwd(m, x, ts, txt)
        st = m._step_cache_states[("cond", "uncond")]
        assert torch.equal(st.idx, idx) and torch.equal(st.counters, counters)
        assert torch.allclose(got, want, atol=5e-5, rtol=1e-4)
    assert counters.max() >= 2                                   # somebody has sat out every partial step so far


def test_live_rows_keep_dead_rows_off_the_list():
    sd, m, xs, txt, ts = _setup(b=1, sample_ratio=0.5, warmup_steps=1, full_step_interval=50)
    live = (20, 40)                                              # the middle frame
    _fwd(m, xs[0], ts, txt, live_rows=live)
    _fwd(m, xs[1], ts, txt, live_rows=live)
    st = m._step_cache_states["cond"]
    assert st.idx.shape[0] == 10 and int(st.idx.min()) >= 20 and int(st.idx.max()) < 40
    assert m.cache_log[-1] == ("cond", 1, P, 10)


# ------------------------------------------------------------------ the fixtures the GPU tests share
def test_the_fixtures_have_what_makes_them_bite():
    for n in (1188, 65536):
        s = R.quantised_scores(n)
        assert len(set(s.tolist())) <= 18 and n // len(set(s.tolist())) > 60           # ties everywhere
        assert bool(torch.isinf(s).any()) and bool((s == -math.inf).any()) and bool((s == math.inf).any())
        zeros = s[s == 0]
        assert bool(torch.signbit(zeros).any()) and not bool(torch.signbit(zeros).all())      # both zeros: one tie class
        for k in (1, 64, 475, n - 1, n):
            idx, _ = R.select_ref(s, k)
            assert idx.shape[0] == k and bool((idx[1:] > idx[:-1]).all())
        # a threshold class that is cut: some rows equal to the k-th score are on the list and some are not
        idx, _ = R.select_ref(s, 475)
        on = torch.zeros(n, dtype=torch.bool)
        on[idx.long()] = True
        kth = s[idx.long()].min()
        assert bool((s[on] == kth).any()) and bool((s[~on] == kth).any())
        assert int(((s == kth) & ~on).nonzero().min()) > int(((s == kth) & on).nonzero().max())      # ties go to the lower index
    assert R.LIST_ROWS % 64 != 0 and R.LIST_ROWS % 256 != 0 and R.LIST_ROWS == ras_active_count(0.4, 1188)
    po, counters, row = R.starved_rows()
    plain = R.score_ref(po)
    assert int(plain.argmin()) == row
    without, _ = R.select_ref(plain, R.LIST_ROWS)
    with_counters, new = R.select_ref(R.score_ref(po, 1, counters, 0.1), R.LIST_ROWS, counters)
    assert row not in without.tolist() and row in with_counters.tolist() and int(new[row]) == 0      # starved onto the list
    assert R.starvation_steps(1.0, 2.0, 0.1) == 7 and R.starvation_steps(3.0, 2.0, 0.1) == 0


# ------------------------------------------------------------------ the trajectory mask of the example
def test_trajectory_token_mask_marks_the_patches_under_painted_pixels():
    from frameino_amd.conditions import trajectory_token_mask
    traj = torch.ones(9, 3, 64, 96)                              # 9 pixel frames -> 3 latent frames; tokens of 32 x 32 pixels
    traj[0, 1, 5, 40] = 0.2                                      # frame 0 -> latent 0, token (0, 1)
    traj[3, :, 63, 95] = -1.0                                    # frame 3 -> latent 1, token (1, 2)
    traj[4, 0, 32, 0] = 0.99                                     # frame 4 -> latent 1, token (1, 0)
    traj[5, 2, 0, 64] = 0.0                                      # frame 5 -> latent 2, token (0, 2)
    traj[6, 2, 10, 10] = 1.0 - 0.5 / 255                         # within the tolerance of white: not painted
    mask = trajectory_token_mask(traj, 2, 3, temporal_stride=4, extra_frames=1)
    assert mask.dtype == torch.bool and mask.shape == (4 * 6,)
    assert mask.view(4, 2, 3).nonzero().tolist() == [[0, 0, 1], [1, 1, 0], [1, 1, 2], [2, 0, 2]]
    assert trajectory_token_mask(traj, 2, 3).shape == (18,)
    with pytest.raises(ValueError, match="does not split"):
        trajectory_token_mask(traj, 5, 3)
    m = _tiny_model()
    m.enable_cache(RegionAdaptiveSamplingConfig(always_active=mask))          # what the config takes
