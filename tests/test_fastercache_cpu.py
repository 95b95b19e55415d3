"""FasterCache without a GPU: the config and its validation, the truth tables of the three pure functions against the
restatement in tests/fastercache_ref.py, the duck-typed config, every refusal in both orders, the pipeline's limits, the
forward's three call shapes over a recording stand-in for the stack and the ops, and the C ABI's error paths."""
import re
import warnings

import pytest
import torch

from frameino_amd import _lib, ops
from frameino_amd.step_cache import (FasterCacheConfig, FirstBlockCacheConfig, PyramidAttentionBroadcastConfig, TaylorSeerCacheConfig,
                                     fastercache_attention_decide, fastercache_uncond_decide, fastercache_weights)
from tests import fastercache_ref as R
from tests.test_step_cache_cpu import _model, _pipe


def _cfg(**kw):
    kw.setdefault("current_timestep_callback", lambda: 500)
    kw.setdefault("attention_weight_callback", lambda m: 0.5)
    return FasterCacheConfig(**kw)


# ------------------------------------------------------------------ config
def test_config_defaults_are_diffusers():
    c = FasterCacheConfig()
    assert (c.spatial_attention_block_skip_range, c.spatial_attention_timestep_skip_range) == (2, (-1, 681))
    assert (c.unconditional_batch_skip_range, c.unconditional_batch_timestep_skip_range) == (5, (-1, 641))
    assert (c.low_frequency_weight_update_timestep_range, c.high_frequency_weight_update_timestep_range) == ((99, 901), (-1, 301))
    assert (c.alpha_low_frequency, c.alpha_high_frequency, c.tensor_format, c.is_guidance_distilled) == (1.1, 1.1, "BCFHW", False)
    assert c.attention_weight_callback is c.low_frequency_weight_callback is c.high_frequency_weight_callback is None
    assert c.current_timestep_callback is None and c.temporal_attention_block_skip_range is None
    assert c.temporal_attention_timestep_skip_range == (-1, 681) and c.spatial_attention_block_identifiers


@pytest.mark.parametrize("bad", [dict(spatial_attention_block_skip_range=0), dict(spatial_attention_block_skip_range=2.0),
                                 dict(unconditional_batch_skip_range=0), dict(unconditional_batch_skip_range=True),
                                 dict(unconditional_batch_timestep_skip_range=(5, 5)),
                                 dict(spatial_attention_timestep_skip_range=(1,)),
                                 dict(low_frequency_weight_update_timestep_range="all"),
                                 dict(high_frequency_weight_update_timestep_range=(9, 1)),
                                 dict(alpha_low_frequency=-1.0), dict(alpha_high_frequency=float("inf")),
                                 dict(attention_weight_callback=0.5), dict(tensor_format="BFCHW"),
                                 dict(current_timestep_callback=None)],
                         ids=lambda b: "-".join(f"{k}" for k in b))
def test_bad_values_raise(bad):
    m = _model()
    with pytest.raises(ValueError, match=next(iter(bad))):
        m.enable_cache(_cfg(**bad))
    assert not m.is_cache_enabled


def test_accepted_values_and_the_one_warning():
    for ok in (dict(spatial_attention_block_skip_range=None), dict(unconditional_batch_skip_range=None),
               dict(temporal_attention_block_skip_range=3, temporal_attention_timestep_skip_range=(0, 1)),
               dict(spatial_attention_block_identifiers=("x",)), dict(is_guidance_distilled=True), dict(alpha_low_frequency=0)):
        m = _model()
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            m.enable_cache(_cfg(**ok))
        assert m.is_cache_enabled and m._faster_on and not m._pab_on and not m._taylor_on
        assert m._faster_attention == (ok.get("spatial_attention_block_skip_range", 2) is not None)
        assert m._step_cache_segments(1, 8) is None           # the first-block code is inert
    m = _model()
    with pytest.warns(UserWarning, match="attention_weight_callback.*0.5") as seen:
        m.enable_cache(_cfg(attention_weight_callback=None))
    assert len(seen) == 1 and m._faster_weight(m.blocks[0].attn1) == 0.5
    m = _model()
    with warnings.catch_warnings():                             # attention not hooked: nothing to warn about
        warnings.simplefilter("error")
        m.enable_cache(_cfg(attention_weight_callback=None, spatial_attention_block_skip_range=None))


def test_a_duck_typed_config_is_accepted_and_a_bare_name_is_not():
    class FasterCacheConfig:                                    # noqa: F811  what diffusers' own class looks like from here
        def __init__(self):
            self.spatial_attention_block_skip_range, self.unconditional_batch_skip_range = 3, 4
            self.current_timestep_callback = lambda: 100
            self.attention_weight_callback = lambda m: 0.25

    m = _model()
    cfg = FasterCacheConfig()
    m.enable_cache(cfg)
    assert m.is_cache_enabled and m._faster_on and m._faster_attention and m._faster_weight(None) == 0.25
    # the fields it lacks read as diffusers' defaults
    assert [fastercache_uncond_decide(i, 100.0, True, cfg) for i in range(6)] == [False, True, True, True, False, True]
    assert fastercache_uncond_decide(1, 641.0, True, cfg) is False
    assert fastercache_weights(100.0, 1.0, 1.0, cfg) == (R.f32(1.1), R.f32(1.1))
    m.disable_cache()

    class Bare:
        pass
    Bare.__name__ = "FasterCacheConfig"
    with pytest.raises(NotImplementedError, match="FasterCacheConfig.*unconditional_batch_skip_range"):
        m.enable_cache(Bare())
    assert not m.is_cache_enabled


def test_exclusivity_and_disable_restores_the_model():
    m = _model()
    before = dict(vars(m))
    m.enable_cache(_cfg())
    for other in (FirstBlockCacheConfig(), TaylorSeerCacheConfig(), _cfg(),
                  PyramidAttentionBroadcastConfig(spatial_attention_block_skip_range=2, current_timestep_callback=lambda: 1)):
        with pytest.raises(ValueError, match="already been enabled"):
            m.enable_cache(other)
    with m.cache_context("cond"):
        m._faster_begin(1, (4, 2, 4, 4), torch.bfloat16, "cpu")
    assert m._step_cache_states and m.cache_log == [("cond", 0, 500.0, True, True)]
    m.disable_cache()
    assert not m.is_cache_enabled and not m._faster_on and m._step_cache_states == {}
    assert m._faster_begin(1, (4, 2, 4, 4), torch.bfloat16, "cpu") is None
    after = dict(vars(m))
    for k in ("_step_cache_states", "_step_cache_log_fresh", "cache_log", "_step_cache_config"):
        before.pop(k, None), after.pop(k, None)
    assert after.keys() == before.keys() and all(after[k] is before[k] or after[k] == before[k] for k in before)
    m.enable_cache(TaylorSeerCacheConfig())                    # ... and another cache can follow


def test_cogvideox_keeps_refusing_it():
    from frameino_amd.cogvideox_transformer_3d import CogVideoXTransformer3DModel
    m = CogVideoXTransformer3DModel(num_attention_heads=2, attention_head_dim=64, in_channels=4, out_channels=4, num_layers=1,
                                    text_embed_dim=32, time_embed_dim=32, sample_width=8, sample_height=8, sample_frames=5,
                                    use_rotary_positional_embeddings=True)
    for cfg in (_cfg(), type("FasterCacheConfig", (), {})()):
        with pytest.raises(NotImplementedError, match="FasterCacheConfig.*PyramidAttentionBroadcastConfig is$"):
            m.enable_cache(cfg)
    assert not m.is_cache_enabled


# ------------------------------------------------------------------ the three pure functions
def test_uncond_decide_table():
    c = _cfg()                                                  # N = 5 inside (-1, 641)
    for t in (-1.0, -0.5, 0.0, 300.0, 640.5, 641.0, 900.0):
        for i in range(12):
            for has in (False, True):
                assert fastercache_uncond_decide(i, t, has, c) is R.uncond_skips(i, t, has, c), (i, t, has)
    assert [fastercache_uncond_decide(i, 300.0, True, c) for i in range(11)] == [False] + [True] * 4 + [False] + [True] * 4 + [False]
    assert fastercache_uncond_decide(0, 300.0, True, c) is False                         # i = 0 never skips
    assert fastercache_uncond_decide(3, 300.0, False, c) is False                        # no delta yet
    assert fastercache_uncond_decide(3, -1.0, True, c) is False and fastercache_uncond_decide(3, 641.0, True, c) is False
    assert fastercache_uncond_decide(3, -0.999, True, c) is True and fastercache_uncond_decide(3, 640.999, True, c) is True
    assert not any(fastercache_uncond_decide(i, 300.0, True, _cfg(unconditional_batch_skip_range=None)) for i in range(12))
    assert not any(fastercache_uncond_decide(i, 300.0, True, _cfg(is_guidance_distilled=True)) for i in range(12))
    assert not any(fastercache_uncond_decide(i, 300.0, True, _cfg(unconditional_batch_skip_range=1)) for i in range(12))
    assert R.uncond_pattern([300.0] * 7, c) == [True, False, False, False, False, True, False]


def test_weights_table_and_compounding():
    c = _cfg()                                                  # low (99, 901), high (-1, 301), both 1.1
    a = R.f32(1.1)
    assert fastercache_weights(200.0, 1.0, 1.0, c) == (a, a)
    assert fastercache_weights(99.0, 1.0, 1.0, c) == (1.0, a) and fastercache_weights(99.5, 1.0, 1.0, c) == (a, a)
    assert fastercache_weights(301.0, 1.0, 1.0, c) == (a, 1.0) and fastercache_weights(300.5, 1.0, 1.0, c) == (a, a)
    assert fastercache_weights(901.0, 1.0, 1.0, c) == (1.0, 1.0) and fastercache_weights(900.5, 1.0, 1.0, c) == (a, 1.0)
    assert fastercache_weights(-1.0, 1.0, 1.0, c) == (1.0, 1.0) and fastercache_weights(-0.5, 1.0, 1.0, c) == (1.0, a)
    for t in (-1.0, 50.0, 99.0, 200.0, 301.0, 500.0, 901.0):
        assert fastercache_weights(t, 1.0, a, c) == R.weights(t, 1.0, a, c), t
    # three consecutive skips: every product rounded to fp32
    al = ah = 1.0
    for k in range(3):
        al, ah = fastercache_weights(200.0 - k, al, ah, c)
    a2 = R.f32(torch.tensor(a, dtype=torch.float32) * torch.tensor(a, dtype=torch.float32))
    a3 = R.f32(torch.tensor(a2, dtype=torch.float32) * torch.tensor(a, dtype=torch.float32))
    assert (al, ah) == (a3, a3) and a3 != 1.1 ** 3
    # the callbacks win over the ranges and see the model
    seen = []
    cb = _cfg(low_frequency_weight_callback=lambda m: seen.append(m) or 2.0, high_frequency_weight_callback=lambda m: 0.5)
    assert fastercache_weights(2000.0, 1.5, 3.0, cb, "model") == (3.0, 1.5) and seen == ["model"]
    assert fastercache_weights(200.0, 1.0, 1.0, _cfg(alpha_low_frequency=1.25, alpha_high_frequency=0.5)) == (1.25, 0.5)


def test_attention_decide_table():
    c = _cfg()                                                  # N = 2 inside (-1, 681)
    for t in (-1.0, -0.5, 300.0, 680.5, 681.0):
        for i in range(7):
            for n in (0, 1, 2):
                for ran in (False, True):
                    assert fastercache_attention_decide(i, t, n, ran, c) is R.attention_computes(i, t, n, ran, c), (i, t, n, ran)
    assert [fastercache_attention_decide(i, 300.0, 2, True, c) for i in range(6)] == [True, False] * 3
    assert fastercache_attention_decide(1, 300.0, 0, True, c) is True                    # no plane yet
    assert fastercache_attention_decide(1, 300.0, 2, False, c) is True                   # the stack did not run at i - 1
    assert fastercache_attention_decide(1, 681.0, 2, True, c) is True and fastercache_attention_decide(1, -1.0, 2, True, c) is True
    assert fastercache_attention_decide(1, 680.9, 2, True, c) is False and fastercache_attention_decide(1, -0.9, 2, True, c) is False
    assert all(fastercache_attention_decide(i, 300.0, 2, True, _cfg(spatial_attention_block_skip_range=None)) for i in range(6))


# ------------------------------------------------------------------ refusals, in both orders
def _tiny_model():
    from frameino_amd.transformer_wan import WanTransformer3DModel
    return WanTransformer3DModel(num_attention_heads=2, attention_head_dim=64, in_channels=4, out_channels=4, text_dim=32,
                                 freq_dim=32, ffn_dim=64, num_layers=2)


class _Shard:
    active = True

    def rows(self, L):
        return 0, L // 2, L // 2


def _first_next(m, **kw):
    return next(m.forward_steps(torch.zeros(1, 4, 2, 4, 4), torch.tensor([500.0]), torch.zeros(1, 3, 32), **kw))


@pytest.mark.parametrize("attention", [2, None], ids=["attention_hooked", "uncond_only"])
def test_refusals_in_both_orders(attention):
    from frameino_amd.attention_processor import MI355WanAttnProcessor
    from frameino_amd.window_attention import SparseAttentionConfig, WindowAttentionConfig
    cfg = _cfg(spatial_attention_block_skip_range=attention)
    m = _tiny_model()
    if attention is None:                                        # the unconditional-branch part combines with both
        m.enable_window_attention(WindowAttentionConfig(1))
        m.enable_cache(cfg)
        m.disable_cache()
        m.disable_window_attention()
        m.enable_cache(cfg)
        m.enable_window_attention(WindowAttentionConfig(1))
        m.disable_window_attention()
        m.enable_sparse_attention(SparseAttentionConfig(0.5))
        m.disable_cache()
        m.enable_cache(cfg)
        m.disable_sparse_attention()
        m.disable_cache()
    else:
        m.enable_window_attention(WindowAttentionConfig(1))
        with pytest.raises(NotImplementedError, match="FasterCache.*window attention"):
            m.enable_cache(cfg)
        assert not m.is_cache_enabled
        m.disable_window_attention()
        m.enable_cache(cfg)
        with pytest.raises(NotImplementedError, match="window attention.*FasterCache"):
            m.enable_window_attention(WindowAttentionConfig(1))
        assert not m.is_window_attention_enabled
        with pytest.raises(NotImplementedError, match="sparse attention.*FasterCache"):
            m.enable_sparse_attention(SparseAttentionConfig(0.5))
        assert not m.is_sparse_attention_enabled
        m.disable_cache()
        m.enable_sparse_attention(SparseAttentionConfig(0.5))
        with pytest.raises(NotImplementedError, match="FasterCache.*sparse attention"):
            m.enable_cache(cfg)
        m.disable_sparse_attention()
    # a token-sharded plan: on the model at enable time, or handed to the forward (refused before any launch)
    m.parallel = _Shard()
    with pytest.raises(NotImplementedError, match="token-sharded"):
        m.enable_cache(cfg)
    m.parallel = None
    m.enable_cache(cfg)
    with m.cache_context("c"), pytest.raises(NotImplementedError, match="one GPU"):
        _first_next(m, shard=_Shard())
    assert m.cache_log == () or m.cache_log == []                # refused before the forward counted
    m.disable_cache()

    class Mine(MI355WanAttnProcessor):
        pass

    m.blocks[1].attn1.set_processor(Mine())
    if attention is None:
        m.enable_cache(cfg)                                      # the unconditional-branch part takes any processor
    else:
        with pytest.raises(NotImplementedError, match="attention processor"):
            m.enable_cache(cfg)
        m.blocks[1].attn1.set_processor(MI355WanAttnProcessor())
        m.enable_cache(cfg)
        m.blocks[0].attn2.set_processor(Mine())
        with m.cache_context("c"), pytest.raises(NotImplementedError, match="attention processor"):
            _first_next(m)


# ------------------------------------------------------------------ pipeline limits
def test_pipeline_limits_and_reset():
    pipe = _pipe()
    tr = pipe.transformer
    tr.enable_cache(_cfg())
    assert pipe._step_cache_check(1) is True and pipe._step_cache_check(2) is True        # a batch is allowed
    pipe.use_hip_graph = True
    with pytest.raises(RuntimeError, match="use_hip_graph=True with FasterCache"):
        pipe._step_cache_check(1)
    pipe.use_hip_graph = None
    pipe.parallel = object()
    with pytest.raises(NotImplementedError, match="FasterCache runs on one GPU"):
        pipe._step_cache_check(1)
    pipe.parallel = None
    with tr.cache_context("cond"):
        tr._faster_begin(1, (4, 2, 4, 4), torch.bfloat16, "cpu")
    assert tr._step_cache_states and len(tr.cache_log) == 1
    pipe.maybe_free_model_hooks()
    assert tr._step_cache_states == {} and len(tr.cache_log) == 1


# ------------------------------------------------------------------ the forward's call shapes over a recording stand-in
class _RecordingOps:
    """the three FasterCache entries of frameino_amd.ops on the CPU (tests/fastercache_ref.py), recording their calls"""

    def __init__(self):
        self.calls = []

    def fastercache_supported(self, planes, h, w):
        return h * w <= 16384

    def fastercache_delta(self, u, c, d_low, d_high):
        self.calls.append("delta")
        dl, dh = R.delta_cpu(u, c)
        d_low.copy_(dl)
        d_high.copy_(dh)
        return d_low, d_high

    def fastercache_apply(self, c, d_low, d_high, a_low, a_high, out=None):
        self.calls.append(("apply", a_low, a_high))
        res = R.apply_ref(c, d_low, d_high, a_low, a_high)
        return res if out is None else out.copy_(res)


def _recording_model(config, planes):
    """a Wan DiT whose stack is a stand-in: `planes[context](x)` is the prediction of one element; records every launch of the
    stack as (contexts, batch)"""
    m = _model()
    m.ops = _RecordingOps()
    m.enable_cache(config)
    m.stack_calls = []

    def stack(hidden_states, timestep, text, contexts, *args, faster=None, out_buf=None, text_slot=None):
        names = tuple(contexts) if contexts is not None else (m._ctx_name,)
        m.stack_calls.append((names, hidden_states.shape[0], text.shape[0], text_slot))
        out = torch.stack([planes[n](hidden_states[i]) for i, n in enumerate(names)])
        if out_buf is not None:
            out_buf.copy_(out[0])
            return out_buf[None]
        return out
        yield                                                    # (a generator, like the stack it stands for)

    m._forward_stack = stack
    return m


@pytest.mark.parametrize("batched", [False, True], ids=["sequential", "batched"])
def test_call_shapes_against_the_driver(batched):
    g = torch.Generator().manual_seed(5)
    wc, wu = torch.randn(4, 1, 1, 1, generator=g), torch.randn(4, 1, 1, 1, generator=g)
    planes = {"cond": lambda x: (x[:4] * wc).bfloat16(), "uncond": lambda x: (x[:4] * wu + 0.5).bfloat16()}
    clock = {"t": 0.0}
    cfg = _cfg(unconditional_batch_skip_range=3, spatial_attention_block_skip_range=None, current_timestep_callback=lambda: clock["t"])
    m = _recording_model(cfg, planes)
    ts = [950.0, 700.0, 600.0, 500.0, 400.0, 250.0, 200.0, 50.0]
    xs = [torch.randn(4, 3, 10, 12, generator=g).bfloat16() for _ in ts]
    want, want_log = R.drive(lambda ctx, x: planes[ctx](x), xs, ts, cfg)
    txt = torch.zeros(2, 3, 8)
    for i, (x, t) in enumerate(zip(xs, ts)):
        clock["t"] = t
        if batched:
            with m.cache_context("cfg"):
                both = m(x[None].expand(2, -1, -1, -1, -1), None, txt, return_dict=False, _cache_contexts=("cond", "uncond"))[0]
            c, u = both[0], both[1]
        else:
            with m.cache_context("cond"):
                c = m(x[None], None, txt[:1], return_dict=False)[0][0]
            with m.cache_context("uncond"):
                u = m(x[None], None, txt[1:], return_dict=False)[0][0]
        assert torch.equal(c, want[i][0]) and torch.equal(u, want[i][1]), i
    assert [e[:4] for e in m.cache_log] == want_log and all(e[4] == e[3] for e in m.cache_log)
    ran = [e[3] for e in want_log if e[0] == "uncond"]
    # t = 950 and 700 lie outside (-1, 641); i = 3 and 6 are multiples of 3; the others skip.  The weights: t = 600 and 400
    # move the low one alone, 250 both (a second skip in a row: compounded), 50 the high one alone
    assert ran == [True, True, False, True, False, False, True, False]
    if batched:                                                  # a skipping step launches the stack with batch 1 ...
        assert m.stack_calls == [((("cond", "uncond"), 2, 2, None) if r else (("cond",), 1, 1, "fastercache-cond")) for r in ran]
    else:                                                        # ... and a skipped "uncond" call launches nothing
        assert m.stack_calls == [c_ for r in ran for c_ in ([(("cond",), 1, 1, None)] + ([(("uncond",), 1, 1, None)] if r else []))]
    # one delta per computing step (none while "uncond" never skipped before: still taken, it is what the next skip needs),
    # one apply per skipping step with the compounded weights
    assert [c_ for c_ in m.ops.calls if c_ == "delta"] == ["delta"] * sum(ran)
    a = R.f32(1.1)
    a2 = R.f32(torch.tensor(a) * torch.tensor(a))
    assert [c_ for c_ in m.ops.calls if c_ != "delta"] == [("apply", a, 1.0), ("apply", a, 1.0), ("apply", a2, a), ("apply", 1.0, a)]


def test_other_contexts_guidance_off_and_the_missing_cond_call():
    planes = {k: (lambda x: x[:4].bfloat16()) for k in ("cond", "uncond", "c", "a", "b")}
    cfg = _cfg(unconditional_batch_skip_range=2, unconditional_batch_timestep_skip_range=(-1, 1001),
               spatial_attention_block_skip_range=None)
    m = _recording_model(cfg, planes)
    x, txt = torch.randn(1, 4, 2, 4, 4), torch.zeros(2, 3, 8)
    for _ in range(3):                                           # any other context: inert, the stack always runs
        with m.cache_context("c"):
            m(x, None, txt[:1], return_dict=False)
        with m.cache_context("cfg"):
            m(x.expand(2, -1, -1, -1, -1), None, txt, return_dict=False, _cache_contexts=("a", "b"))
    for _ in range(3):                                           # guidance off: "cond" alone never skips
        with m.cache_context("cond"):
            m(x, None, txt[:1], return_dict=False)
    assert len(m.stack_calls) == 9 and m.ops.calls == [] and all(e[3] for e in m.cache_log)
    with m.cache_context("uncond"):
        m(x, None, txt[1:], return_dict=False)                   # i = 0 of "uncond": runs; "cond" is at i = 2: no pair, no delta
    assert m.ops.calls == []
    m._reset_stateful_cache()
    for ctx in ("cond", "uncond"):
        with m.cache_context(ctx):
            m(x, None, txt[:1], return_dict=False)
    assert m.ops.calls == ["delta"] and m._faster_will_skip()
    with m.cache_context("uncond"), pytest.raises(RuntimeError, match='"cond" context has not run forward 1'):
        m(x, None, txt[1:], return_dict=False)
    with pytest.raises(ValueError, match="No context is set"):
        m(x, None, txt[:1], return_dict=False)
    with m.cache_context("cfg"), pytest.raises(ValueError, match="distinct names"):
        m(x.expand(2, -1, -1, -1, -1), None, txt, return_dict=False, _cache_contexts=("cond", "cond"))


def test_the_attention_plan_has_taylorseers_shape():
    m = _model()
    clock = {"t": 300.0}
    m.enable_cache(_cfg(spatial_attention_block_skip_range=2, unconditional_batch_skip_range=2,
                        unconditional_batch_timestep_skip_range=(-1, 1001), current_timestep_callback=lambda: clock["t"]))
    seen = []
    for i in range(4):
        with m.cache_context("cfg"):
            fc = m._faster_begin(2, (4, 2, 4, 4), torch.bfloat16, "cpu", ("cond", "uncond"))
        plan = m._faster_attention_plan(fc, sum(e.stack for e in fc.entries), 4, 8, torch.bfloat16, "cpu")
        seen.append([(g.name, g.r0, g.r1, g.compute["self"], g.compute["cross"], g.k, g.n_old, g.n_new) for g in plan.segs])
        if i == 0:
            m._step_cache_states["uncond"].has_delta = True      # (what the delta of step 0 leaves)
    assert plan.hooked == {"self": True, "cross": False} and plan.planes == 2 and plan.factor_dtype == torch.bfloat16
    assert seen == [[("cond", 0, 4, True, True, 1, 0, 1), ("uncond", 4, 8, True, True, 1, 0, 1)],
                    [("cond", 0, 4, False, True, 1, 1, 1)],                                  # "uncond" skips its stack
                    [("cond", 0, 4, True, True, 1, 1, 2), ("uncond", 4, 8, True, True, 1, 1, 2)],    # its stack did not run at 1
                    [("cond", 0, 4, False, True, 1, 2, 2)]]
    assert [e[3:] for e in m.cache_log if e[0] == "uncond"] == [(True, True), (False, False), (True, True), (False, False)]
    buf = m._taylor_buffer(plan, plan.segs[0], ("self", 0), 8, "cpu")
    assert buf.shape == (2, 4, 8) and buf.dtype == torch.bfloat16


# ------------------------------------------------------------------ header, SIGNATURES, library; the ABI's error paths
NAMES = ("fino_fastercache_supported", "fino_fastercache_delta", "fino_fastercache_apply")


def test_header_signatures_and_library_agree():
    lib = _lib.lib()
    declared = _lib.declared_symbols()
    header = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    for name in NAMES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
        params = re.search(name + r"\s*\(([^)]*)\)", header).group(1).split(",")
        assert len(params) == len(_lib.SIGNATURES[name]), name
        for p, ct in zip(params, _lib.SIGNATURES[name]):
            want = (_lib.c_void_p if "*" in p else _lib.c_i64 if "int64_t" in p else _lib.c_float if "float" in p else _lib.c_int)
            assert ct is want, (name, p)
    assert lib.fino_version() == 103 == _lib.ABI_VERSION and "#define FINO_VERSION 103" in open(_lib.HEADER_PATH).read()
    assert ops.FASTERCACHE_MAX_PLANE == 16384 and "FINO_FASTERCACHE_MAX_PLANE = 16384" in header


def test_supported_and_the_c_abi_checks_before_any_launch():
    lib = _lib.lib()
    yes = [(1, 1, 1), (720, 44, 80), (1, 128, 128), (3, 1, 16384), (3, 16384, 1), (2, 64, 112)]
    no = [(0, 4, 4), (1, 0, 4), (1, 4, 0), (1, 128, 129), (1, 16385, 1), (-1, 4, 4), (1, 1 << 40, 1 << 40)]
    assert all(lib.fino_fastercache_supported(*s) == 1 for s in yes) and all(lib.fino_fastercache_supported(*s) == 0 for s in no)
    assert all(ops.fastercache_supported(*s) for s in yes) and not any(ops.fastercache_supported(*s) for s in no)
    a = 4096                                                      # any 16-byte aligned address: nothing is dereferenced
    for args, rc, word in (((0, a, a, a, 2, 4, 6, 0, 0), -1, b"null"), ((a, 0, a, a, 2, 4, 6, 0, 0), -1, b"null"),
                           ((a, a, 0, a, 2, 4, 6, 0, 0), -1, b"null"), ((a, a, a, 0, 2, 4, 6, 0, 0), -1, b"null"),
                           ((a + 2, a, a, a, 2, 4, 6, 0, 0), -1, b"alignment"), ((a, a, a, a + 8, 2, 4, 6, 0, 0), -1, b"alignment"),
                           ((a, a, a, a, 2, 4, 6, 2, 0), -1, b"dtype"), ((a, a, a, a, 2, 4, 6, 7, 0), -1, b"dtype"),
                           ((a, a, a, a, 0, 4, 6, 0, 0), -3, b"planes=0"), ((a, a, a, a, 2, 128, 129, 0, 0), -3, b"width=129"),
                           ((a, a, a, a, 2, 0, 6, 1, 0), -3, b"height=0")):
        assert lib.fino_fastercache_delta(*args) == rc and word in lib.fino_last_error(), (args, lib.fino_last_error())
    for args, word in (((0, a, a, 1.0, 1.0, a, 8, 0, 0), b"null"), ((a, a, a, 1.0, 1.0, 0, 8, 0, 0), b"null"),
                       ((a, a + 4, a, 1.0, 1.0, a, 8, 0, 0), b"alignment"), ((a, a, a, 1.0, 1.0, a + 2, 8, 1, 0), b"alignment"),
                       ((a, a, a, 1.0, 1.0, a, 0, 0, 0), b"n=0"), ((a, a, a, 1.0, 1.0, a, -3, 0, 0), b"n=-3"),
                       ((a, a, a, 1.0, 1.0, a, 8, 2, 0), b"dtype")):
        assert lib.fino_fastercache_apply(*args) == -1 and word in lib.fino_last_error(), (args, lib.fino_last_error())


def test_the_ops_check_their_arguments_before_the_library():
    u = torch.zeros(2, 4, 6, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.fastercache_delta(u, u)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.fastercache_apply(u, u.float(), u.float(), 1.0, 1.0)


def test_the_restatement_low_pass():
    """what tests/fastercache_ref.py's low-pass is: the bin counts of the contract, a projection (LP(LP(x)) = LP(x)), the plane
    mean at r = 0, and real to rounding"""
    assert [R.bin_count(h, w) for h, w in ((44, 80), (4, 6), (5, 7), (10, 10))] == [197, 1, 5, 13]
    g = torch.Generator().manual_seed(0)
    for h, w in ((44, 80), (4, 6), (5, 7), (10, 10), (16, 9), (9, 16)):
        x = torch.randn(2, h, w, generator=g, dtype=torch.float64)
        lp = R.lowpass(x)
        assert float((R.lowpass(lp) - lp).abs().max()) < 1e-13
        if min(h, w) < 5:
            assert float((lp - x.mean(dim=(-2, -1), keepdim=True)).abs().max()) < 1e-14
    dl, dh = R.delta_cpu(torch.ones(1, 5, 7).bfloat16(), torch.zeros(1, 5, 7).bfloat16())
    assert float((dl - 1).abs().max()) < 1e-6 and float(dh.abs().max()) < 1e-6
