"""TaylorSeer caching without a GPU: the config and its validation, the duck-typed config, the rule (`taylorseer_decide`) on
its schedule, the prediction's coefficients, every refusal in both orders, the per-context state machine (`_taylor_begin`) with
its log, the restatement's own arithmetic (tests/taylorseer_ref.py), and the pipeline's limits."""
import math

import pytest
import torch

from frameino_amd import ops
from frameino_amd.step_cache import (FirstBlockCacheConfig, PyramidAttentionBroadcastConfig, TaylorSeerCacheConfig,
                                     taylorseer_decide)
from tests import taylorseer_ref as R
from tests.test_step_cache_cpu import _model, _pipe

C, P = True, False


# ------------------------------------------------------------------ config
def test_config_defaults_are_diffusers():
    c = TaylorSeerCacheConfig()
    assert (c.cache_interval, c.disable_cache_before_step, c.disable_cache_after_step, c.max_order) == (5, 3, None, 1)
    assert (c.taylor_factors_dtype, c.skip_predict_identifiers, c.cache_identifiers, c.use_lite_mode) == (None, None, None, False)


@pytest.mark.parametrize("bad", [dict(cache_interval=0), dict(cache_interval=2.5), dict(cache_interval=True),
                                 dict(cache_interval=None), dict(disable_cache_before_step=0),
                                 dict(disable_cache_before_step=-1), dict(disable_cache_after_step=-1),
                                 dict(disable_cache_after_step=1.5), dict(max_order=-1), dict(max_order=4), dict(max_order=1.0),
                                 dict(taylor_factors_dtype=torch.float64), dict(taylor_factors_dtype="bf16")],
                         ids=lambda b: "-".join(f"{k}={v}" for k, v in b.items()))
def test_bad_values_raise(bad):
    m = _model()
    with pytest.raises(ValueError, match=next(iter(bad))):
        m.enable_cache(TaylorSeerCacheConfig(**bad))
    assert not m.is_cache_enabled


def test_accepted_values_and_module_selection():
    for ok in (dict(cache_interval=1), dict(max_order=0), dict(max_order=3), dict(disable_cache_after_step=0),
               dict(taylor_factors_dtype=torch.float32), dict(taylor_factors_dtype=torch.float16),
               dict(taylor_factors_dtype=torch.bfloat16), dict(use_lite_mode=True)):
        m = _model()
        m.enable_cache(TaylorSeerCacheConfig(**ok))
        assert m.is_cache_enabled and m._taylor_on and m._taylor_lite == bool(ok.get("use_lite_mode")) and not m._pab_on
        assert m._step_cache_segments(1, 8) is None           # the first-block code is inert
    for field in ("skip_predict_identifiers", "cache_identifiers"):
        m = _model()
        with pytest.raises(NotImplementedError, match=field):
            m.enable_cache(TaylorSeerCacheConfig(**{field: ("blocks",)}))
        assert not m.is_cache_enabled


def test_a_duck_typed_config_is_accepted_and_a_bare_name_is_not():
    class TaylorSeerCacheConfig:                                # noqa: F811  what diffusers' own class looks like from here
        def __init__(self):
            self.cache_interval, self.disable_cache_before_step, self.max_order = 3, 2, 1

    m = _model()
    cfg = TaylorSeerCacheConfig()
    m.enable_cache(cfg)
    assert m.is_cache_enabled and m._taylor_on and not m._taylor_lite
    assert [taylorseer_decide(s, 1, cfg) for s in range(8)] == [C, C, P, P, C, P, P, C]    # (no disable_cache_after_step: None)
    m.disable_cache()

    class Bare:
        pass
    Bare.__name__ = "TaylorSeerCacheConfig"
    with pytest.raises(NotImplementedError, match="TaylorSeerCacheConfig.*cache_interval"):
        m.enable_cache(Bare())
    assert not m.is_cache_enabled


def test_exclusivity_and_disable_restores_the_model():
    m = _model()
    before = dict(vars(m))
    m.enable_cache(TaylorSeerCacheConfig())
    for other in (FirstBlockCacheConfig(), TaylorSeerCacheConfig(),
                  PyramidAttentionBroadcastConfig(spatial_attention_block_skip_range=2, current_timestep_callback=lambda: 1)):
        with pytest.raises(ValueError, match="already been enabled"):
            m.enable_cache(other)
    with m.cache_context("c"):
        m._taylor_begin(1, 8, 8, torch.bfloat16, "cpu")
    assert m._step_cache_states and m.cache_log == [("c", 0, True)]
    m.disable_cache()
    assert not m.is_cache_enabled and not m._taylor_on and m._step_cache_states == {} and m._step_cache_config is None
    assert m._taylor_begin(1, 8, 8, torch.bfloat16, "cpu") is None
    after = dict(vars(m))
    for k in ("_step_cache_states", "_step_cache_log_fresh", "cache_log", "_step_cache_config"):
        before.pop(k, None), after.pop(k, None)                # (the state dict, now empty, and the log the call left)
    assert after.keys() == before.keys() and all(after[k] is before[k] or after[k] == before[k] for k in before)
    m.enable_cache(FirstBlockCacheConfig())                    # ... and another cache can follow


def test_cogvideox_keeps_refusing_it():
    from frameino_amd.cogvideox_transformer_3d import CogVideoXTransformer3DModel
    m = CogVideoXTransformer3DModel(num_attention_heads=2, attention_head_dim=64, in_channels=4, out_channels=4, num_layers=1,
                                    text_embed_dim=32, time_embed_dim=32, sample_width=8, sample_height=8, sample_frames=5,
                                    use_rotary_positional_embeddings=True)
    with pytest.raises(NotImplementedError, match="TaylorSeerCacheConfig.*PyramidAttentionBroadcastConfig is$"):
        m.enable_cache(TaylorSeerCacheConfig())                # the fully attributed config too
    assert not m.is_cache_enabled


# ------------------------------------------------------------------ the rule
def _table(n_steps, **kw):
    cfg, n, out = TaylorSeerCacheConfig(**kw), 0, []
    for s in range(n_steps):
        out.append(taylorseer_decide(s, n, cfg))
        n += out[-1]
    return out


def test_decide_table():
    assert _table(8, disable_cache_before_step=2, cache_interval=3) == [C, C, P, P, C, P, P, C]
    assert _table(12) == [C, C, C, P, P, P, P, C, P, P, P, P]                      # the defaults: W = 3, N = 5
    assert _table(6, cache_interval=1) == [C] * 6                                  # N = 1: every forward computes
    assert _table(6, disable_cache_before_step=1, cache_interval=2) == [C, P, C, P, C, P]
    assert _table(8, disable_cache_before_step=2, cache_interval=3, disable_cache_after_step=5) == [C, C, P, P, C, C, C, C]
    assert _table(4, disable_cache_before_step=2, cache_interval=3, disable_cache_after_step=0) == [C] * 4
    assert _table(9, disable_cache_before_step=10) == [C] * 9                      # all inside the warm-up
    cfg = TaylorSeerCacheConfig(disable_cache_before_step=1, cache_interval=4)
    assert taylorseer_decide(2, 0, cfg) is True and taylorseer_decide(2, 1, cfg) is False      # no factor yet: compute
    assert all(isinstance(taylorseer_decide(s, 1, cfg), bool) for s in range(6))


def test_coefficients():
    assert ops.taylor_coefficients(3, 4) == [1.0, 3.0, 4.5, 4.5]
    assert ops.taylor_coefficients(1, 4) == [1.0, 1.0, 0.5, float(torch.tensor(1 / 6, dtype=torch.float32))]
    assert ops.taylor_coefficients(5, 4)[3] == float(torch.tensor(125 / 6, dtype=torch.float64).to(torch.float32))
    assert ops.taylor_coefficients(7, 1) == [1.0]
    for k in range(1, 9):
        assert ops.taylor_coefficients(k, 4) == R.coefficients(k, 4)
        assert all(c == float(torch.tensor(c, dtype=torch.float32)) for c in ops.taylor_coefficients(k, 4))     # fp32 values


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


@pytest.mark.parametrize("lite", [False, True], ids=["default", "lite"])
def test_refusals_in_both_orders(lite):
    from frameino_amd.attention_processor import MI355WanAttnProcessor
    from frameino_amd.window_attention import SparseAttentionConfig, WindowAttentionConfig
    cfg = TaylorSeerCacheConfig(use_lite_mode=lite)
    m = _tiny_model()
    # window attention
    m.enable_window_attention(WindowAttentionConfig(1))
    with pytest.raises(NotImplementedError, match="TaylorSeer.*window attention"):
        m.enable_cache(cfg)
    assert not m.is_cache_enabled
    m.disable_window_attention()
    m.enable_cache(cfg)
    with pytest.raises(NotImplementedError, match="window attention.*TaylorSeer"):
        m.enable_window_attention(WindowAttentionConfig(1))
    assert not m.is_window_attention_enabled
    # sparse attention
    with pytest.raises(NotImplementedError, match="sparse attention.*TaylorSeer"):
        m.enable_sparse_attention(SparseAttentionConfig(0.5))
    assert not m.is_sparse_attention_enabled
    m.disable_cache()
    m.enable_sparse_attention(SparseAttentionConfig(0.5))
    with pytest.raises(NotImplementedError, match="TaylorSeer.*sparse attention"):
        m.enable_cache(cfg)
    m.disable_sparse_attention()
    # a token-sharded plan: on the model at enable time, or handed to the forward (refused before any launch)
    m.parallel = _Shard()
    with pytest.raises(NotImplementedError, match="token-sharded"):
        m.enable_cache(cfg)
    m.parallel = None
    m.enable_cache(cfg)
    with pytest.raises(NotImplementedError, match="one GPU"):
        _first_next(m, shard=_Shard())
    m.disable_cache()

    # a user-installed attention processor: default mode refuses it in either order, lite mode does not care
    class Mine(MI355WanAttnProcessor):
        pass

    m.blocks[1].attn1.set_processor(Mine())
    if lite:
        m.enable_cache(cfg)
    else:
        with pytest.raises(NotImplementedError, match="attention processor"):
            m.enable_cache(cfg)
        m.blocks[1].attn1.set_processor(MI355WanAttnProcessor())
        m.enable_cache(cfg)
        m.blocks[0].attn2.set_processor(Mine())
        with m.cache_context("c"), pytest.raises(NotImplementedError, match="attention processor"):
            _first_next(m)
        assert m.cache_log == () or m.cache_log == []            # refused before the forward counted


# ------------------------------------------------------------------ state machine and log
def test_state_machine_log_contexts_and_reset():
    m = _model()
    m.enable_cache(TaylorSeerCacheConfig(cache_interval=3, disable_cache_before_step=2, max_order=2))

    def begin(ctx, b=1, **kw):
        with m.cache_context(ctx):
            return m._taylor_begin(b, 4, 8, torch.bfloat16, "cpu", **kw)

    seen = []
    for s in range(8):
        seg = begin("cond").segs[0]
        seen.append((seg.s, seg.compute["self"], seg.compute["cross"], seg.k, seg.n_old, seg.n_new))
    #                 s  computes     k  n_old n_new
    assert seen == [(0, C, C, 0, 0, 1), (1, C, C, 1, 1, 2), (2, P, P, 1, 2, 2), (3, P, P, 2, 2, 2), (4, C, C, 3, 2, 3),
                    (5, P, P, 1, 3, 3), (6, P, P, 2, 3, 3), (7, C, C, 3, 3, 3)]
    assert m.cache_log == [("cond", s, c) for s, c in enumerate([C, C, P, P, C, P, P, C])]
    # another context has its own counter; a batch with one context per element gets one segment each
    plan = begin("cfg", b=2, contexts=("cond", "uncond"))
    assert [(g.name, g.r0, g.r1, g.s, g.compute["self"]) for g in plan.segs] == [("cond", 0, 4, 8, P), ("uncond", 4, 8, 0, C)]
    assert m.cache_log[-2:] == [("cond", 8, P), ("uncond", 0, C)]
    assert plan.planes == 3 and plan.factor_dtype == torch.bfloat16 and plan.taylor is m._step_cache_config
    # buffers: allocated by a computing forward, missing ones raise
    buf = m._taylor_buffer(plan, plan.segs[1], ("self", 0), 8, "cpu")
    assert buf.shape == (3, 4, 8) and buf.dtype == torch.bfloat16 and m._taylor_buffer(plan, plan.segs[1], ("self", 0)) is buf
    with pytest.raises(KeyError, match="no factors"):
        m._taylor_buffer(plan, plan.segs[0], ("cross", 1))
    # a reset starts over and the next forward starts a new log; without a context a forward raises
    m._reset_stateful_cache()
    assert m._step_cache_states == {} and len(m.cache_log) == 10
    assert begin("cond").segs[0].s == 0 and m.cache_log == [("cond", 0, C)]
    with pytest.raises(ValueError, match="No context is set"):
        m._taylor_begin(1, 4, 8, torch.bfloat16, "cpu")
    # the factor dtype of the config
    m.disable_cache()
    m.enable_cache(TaylorSeerCacheConfig(taylor_factors_dtype=torch.float32))
    assert begin("c").factor_dtype == torch.float32


# ------------------------------------------------------------------ the restatement's own arithmetic
def test_the_restatement_extrapolates_polynomials_exactly():
    """y(s) = a + b s + c s^2 with small dyadic values sampled at s = 0, 1, 2 (every operation exact in fp32): the factors are
    the backward differences (y(2), y(2) - y(1), 2 c), the prediction k steps on is f_0 + k f_1 + k^2 / 2 f_2, and a line
    (c = 0) is extrapolated exactly"""
    a, b = torch.tensor([[1.0, -2.0]]), torch.tensor([[0.5, 0.25]])
    for c in (torch.tensor([[0.125, -0.5]]), torch.zeros(1, 2)):
        y = lambda s: (a + b * s + c * s * s).bfloat16()             # noqa: E731
        f, n = [], 0
        for s in range(3):
            f, n = R.update_ref(y(s), f, n, 1, 2, torch.float32)
        assert n == 3 and torch.equal(f[0], y(2).float()) and torch.equal(f[1], (y(2) - y(1)).float()) and torch.equal(f[2], 2 * c)
        for k in (1, 2, 3):
            assert torch.equal(R.predict_ref(f, 3, k, torch.float32), f[0] + k * f[1] + k * k / 2 * f[2])
            assert torch.equal(R.predict_ref64(f, 3, k).float(), R.predict_ref(f, 3, k, torch.float32))
            if not c.any():
                assert torch.equal(R.predict_ref(f, 3, k, torch.bfloat16), y(2 + k))
    # order 1 after steps 0 and 3 (delta = 3) on a line; planes beyond n_new keep their values
    f, n = R.update_ref(y(0) * 0 + 1, [], 0, 0, 1, torch.bfloat16)
    f, n = R.update_ref(y(0) * 0 + 7, f, n, 3, 1, torch.bfloat16)
    assert n == 2 and torch.equal(f[1], torch.full((1, 2), 2.0).bfloat16())
    planes = torch.full((3, 1, 2), 9.0)
    out, n_new = R.update_planes_ref(torch.ones(1, 2).bfloat16(), planes, 0, 1)
    assert n_new == 1 and torch.equal(out[0], torch.ones(1, 2)) and torch.equal(out[1:], planes[1:])
    assert math.isclose(R.coefficients(2, 3)[2], 2.0)


# ------------------------------------------------------------------ pipeline limits
def test_pipeline_limits_and_reset():
    pipe = _pipe()
    tr = pipe.transformer
    tr.enable_cache(TaylorSeerCacheConfig())
    assert pipe._step_cache_check(1) is True and pipe._step_cache_check(2) is True        # a batch is allowed
    pipe.use_hip_graph = True
    with pytest.raises(RuntimeError, match="use_hip_graph=True with TaylorSeer"):
        pipe._step_cache_check(1)
    pipe.use_hip_graph = None
    pipe.parallel = object()
    with pytest.raises(NotImplementedError, match="TaylorSeer caching runs on one GPU"):
        pipe._step_cache_check(1)
    pipe.parallel = None
    with tr.cache_context("cond"):
        tr._taylor_begin(1, 4, 8, torch.bfloat16, "cpu")
    assert tr._step_cache_states and tr.cache_log == [("cond", 0, True)]
    pipe.maybe_free_model_hooks()
    assert tr._step_cache_states == {} and len(tr.cache_log) == 1


def test_the_ops_check_their_arguments_before_the_library():
    y = torch.zeros(4, 8, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.taylor_update(y, torch.zeros(2, 4, 8, dtype=torch.bfloat16), 0, 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.taylor_predict(torch.zeros(2, 4, 8, dtype=torch.bfloat16), 1, 1, dtype=torch.bfloat16)


def test_the_c_abi_checks_before_any_launch():
    import ctypes
    from frameino_amd import _lib
    lib = _lib.lib()
    coef = (ctypes.c_float * 4)(1, 1, 0.5, 1 / 6)
    a = 4096                                                      # any 16-byte aligned address: nothing is dereferenced
    assert lib.fino_taylor_update(a, 8, a, 64, 8, 0, 8, 0, 1, 0, 0, 0, 0) == 0                  # rows = 0: nothing launched
    for args, word in (((a, 8, a, 64, 8, 4, 8, 0, 1, 0, 2, 0, 0), b"dtype"),                  # T = fp32
                       ((a, 8, a, 64, 8, 4, 8, 0, 1, 0, 0, 3, 0), b"factor dtype"),
                       ((a, 8, a, 64, 8, 4, 12, 0, 1, 0, 0, 0, 0), b"dim"),
                       ((a, 8, a, 64, 8, 4, 8, 0, 2, 1, 0, 0, 0), b"n_new"),                    # n_new > n_old + 1
                       ((a, 8, a, 64, 8, 4, 8, 4, 5, 1, 0, 0, 0), b"n_new"),
                       ((a, 8, a, 64, 8, 4, 8, 1, 2, 0, 0, 0, 0), b"delta"),
                       ((a, 4, a, 64, 8, 4, 8, 1, 2, 1, 0, 0, 0), b"row stride"),
                       ((a, 8, a, 16, 8, 4, 8, 1, 2, 1, 0, 0, 0), b"overlap"),                  # plane stride < rows * ld
                       ((a, 8, a + 2, 64, 8, 4, 8, 1, 2, 1, 0, 0, 0), b"aligned")):
        assert lib.fino_taylor_update(*args) == -1 and word in lib.fino_last_error(), (args, lib.fino_last_error())
    assert lib.fino_taylor_predict(a, 64, 8, 2, coef, 0, 0, a, 8, 0, 8, 0, 0, 0, 0, 0, 0) == 0
    for args, word in (((a, 64, 8, 0, coef, 0, 0, a, 8, 4, 8, 0, 0, 0, 0, 0, 0), b"n=0"),
                       ((a, 64, 8, 5, coef, 0, 0, a, 8, 4, 8, 0, 0, 0, 0, 0, 0), b"n=5"),
                       ((a, 64, 8, 2, None, 0, 0, a, 8, 4, 8, 0, 0, 0, 0, 0, 0), b"coefficients"),
                       ((a, 64, 8, 2, coef, 0, 0, a, 8, 4, 8, a, 0, 0, 0, 0, 0), b"gate needs x"),
                       ((a, 64, 8, 2, coef, a, 4, a, 8, 4, 8, 0, 0, 0, 0, 0, 0), b"row stride"),
                       ((a, 16, 8, 2, coef, 0, 0, a, 8, 4, 8, 0, 0, 0, 0, 0, 0), b"overlap"),
                       ((a, 64, 8, 2, coef, 0, 0, a + 4, 8, 4, 8, 0, 0, 0, 0, 0, 0), b"aligned"),
                       ((a, 64, 8, 2, coef, 0, 0, a, 8, 4, 8, 0, 0, 0, 2, 0, 0), b"dtype")):
        assert lib.fino_taylor_predict(*args) == -1 and word in lib.fino_last_error(), (args, lib.fino_last_error())
