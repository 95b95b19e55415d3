"""Pyramid Attention Broadcast without a GPU: the rule (`pab_decide`) on the schedule diffusers' hook gives, the CacheMixin
surface, the per-context state machine (the mixin's `_pab_begin` / `_pab_buffer` driven with synthetic module outputs on the
stand-in kernel front end tests/test_step_cache_cpu.py uses), reset semantics, the single read of the timestep callback per
forward, and the pipeline's limits."""
import warnings

import pytest
import torch

from frameino_amd.step_cache import FirstBlockCacheConfig, PyramidAttentionBroadcastConfig, pab_decide
from tests.test_step_cache_cpu import _FakeOps, _model

TIMESTEPS = [999, 900, 790, 600, 400, 200, 100, 50]


def _schedule(n, rng=(100, 800), timesteps=TIMESTEPS):
    """the hook's rule applied module-side: the cache fills on the first forward and stays filled"""
    out, has_cache = [], False
    for it, t in enumerate(timesteps):
        out.append(pab_decide(it, t, has_cache, n, rng))
        has_cache = True
    return out


# ------------------------------------------------------------------ the rule
def test_schedule_of_the_rule():
    C, R = True, False
    #   iteration          0  1  2  3  4  5  6  7
    #   timestep         999 900 790 600 400 200 100 50
    assert _schedule(2) == [C, C, C, R, C, R, C, C]     # 0: iteration 0; 1: out of range; 2, 4: % 2 == 0; 6: 100 is not > 100; 7: out
    assert _schedule(3) == [C, C, R, C, R, R, C, C]     # 3: 3 % 3 == 0; 6: 6 % 3 == 0 (and the strict bound)
    # an empty cache computes whatever the counter and the timestep say
    assert pab_decide(3, 600, False, 2, (100, 800)) is True and pab_decide(3, 600, True, 2, (100, 800)) is False
    # both bounds are strict
    assert pab_decide(1, 800, True, 2, (100, 800)) is True and pab_decide(1, 799, True, 2, (100, 800)) is False
    assert pab_decide(1, 100, True, 2, (100, 800)) is True and pab_decide(1, 101, True, 2, (100, 800)) is False


def test_config_defaults_are_diffusers():
    c = PyramidAttentionBroadcastConfig()
    assert (c.spatial_attention_block_skip_range, c.temporal_attention_block_skip_range, c.cross_attention_block_skip_range) \
        == (None, None, None)
    assert c.spatial_attention_timestep_skip_range == c.temporal_attention_timestep_skip_range \
        == c.cross_attention_timestep_skip_range == (100, 800)
    assert c.current_timestep_callback is None
    PyramidAttentionBroadcastConfig(spatial_attention_block_identifiers=("a",), temporal_attention_block_identifiers=("b",),
                                    cross_attention_block_identifiers=("c",))      # accepted (and ignored)


# ------------------------------------------------------------------ surface
def test_enable_disable_and_exclusivity():
    m = _model()
    m.enable_cache(PyramidAttentionBroadcastConfig(spatial_attention_block_skip_range=2, current_timestep_callback=lambda: 500))
    assert m.is_cache_enabled and m._pab_on
    assert m._step_cache_segments(1, 8) is None            # the first-block code is inert
    with pytest.raises(ValueError, match="already been enabled"):
        m.enable_cache(FirstBlockCacheConfig())
    with pytest.raises(ValueError, match="already been enabled"):
        m.enable_cache(PyramidAttentionBroadcastConfig(current_timestep_callback=lambda: 1))
    m.disable_cache()
    assert not m.is_cache_enabled and not m._pab_on
    m.enable_cache(FirstBlockCacheConfig())
    with pytest.raises(ValueError, match="already been enabled"):
        m.enable_cache(PyramidAttentionBroadcastConfig(spatial_attention_block_skip_range=2, current_timestep_callback=lambda: 1))
    assert not m._pab_on and m._pab_begin(1, 8, 8, torch.float32, "cpu") is None


def test_a_missing_callback_raises():
    m = _model()
    with pytest.raises(ValueError, match="current_timestep_callback.*must be provided"):
        m.enable_cache(PyramidAttentionBroadcastConfig(spatial_attention_block_skip_range=2))
    assert not m.is_cache_enabled


def test_all_none_warns_and_defaults_to_spatial_2():
    m = _model()
    cfg = PyramidAttentionBroadcastConfig(current_timestep_callback=lambda: 500)
    with pytest.warns(UserWarning, match="spatial_attention_block_skip_range=2"):
        m.enable_cache(cfg)
    assert cfg.spatial_attention_block_skip_range == 2 and cfg.cross_attention_block_skip_range is None
    m.disable_cache()
    with warnings.catch_warnings():
        warnings.simplefilter("error")                     # a set range: no warning
        m.enable_cache(PyramidAttentionBroadcastConfig(cross_attention_block_skip_range=3, current_timestep_callback=lambda: 5))


def test_a_duck_typed_config_is_accepted_and_a_bare_name_is_not():
    class PyramidAttentionBroadcastConfig:                 # noqa: F811  what diffusers' own class looks like from here
        def __init__(self):
            self.spatial_attention_block_skip_range = 2
            self.temporal_attention_block_skip_range = None
            self.cross_attention_block_skip_range = None
            self.spatial_attention_timestep_skip_range = (100, 800)
            self.temporal_attention_timestep_skip_range = (100, 800)
            self.cross_attention_timestep_skip_range = (100, 800)
            self.current_timestep_callback = lambda: 500

    m = _model()
    m.enable_cache(PyramidAttentionBroadcastConfig())
    assert m.is_cache_enabled and m._pab_on
    m.disable_cache()

    class Bare:
        pass
    Bare.__name__ = "PyramidAttentionBroadcastConfig"
    with pytest.raises(NotImplementedError, match="PyramidAttentionBroadcastConfig"):
        m.enable_cache(Bare())
    assert not m.is_cache_enabled


# ------------------------------------------------------------------ state machine
def _forward(m, ctx, ys, rows=4, d=8, contexts=None, b=1):
    """one forward's cache steps on synthetic module outputs ys[kind][layer] ([b * rows, d]): what every attention module of
    the forward hands on -- its own output on a computing step (kept), the cached one otherwise"""
    with m.cache_context(ctx):
        plan = m._pab_begin(b, rows, d, torch.float32, "cpu", contexts)
    outs = []
    for seg in plan.segs:
        out = {}
        for kind in ("self", "cross"):
            for li, y in enumerate(ys[kind]):
                if not plan.hooked[kind]:
                    out[kind, li] = y[seg.r0:seg.r1]
                elif seg.compute[kind]:
                    out[kind, li] = m._pab_buffer(seg, kind, li, d, torch.float32, "cpu").copy_(y[seg.r0:seg.r1]).clone()
                else:
                    out[kind, li] = m._pab_buffer(seg, kind, li).clone()
        outs.append(out)
    return plan, outs


def _ys(layers=3, rows=4, d=8):
    return {k: [torch.randn(rows, d) for _ in range(layers)] for k in ("self", "cross")}


def test_state_machine_both_kinds_two_contexts():
    torch.manual_seed(0)
    m = _model()
    m.ops = _FakeOps()
    now = {"t": 999}
    calls = []

    def cb():
        calls.append(now["t"])
        return now["t"]

    m.enable_cache(PyramidAttentionBroadcastConfig(spatial_attention_block_skip_range=2, cross_attention_block_skip_range=3,
                                                   current_timestep_callback=cb))
    want_self, want_cross = _schedule(2), _schedule(3)
    last = {"cond": None, "uncond": None}
    for it, t in enumerate(TIMESTEPS):
        now["t"] = t
        for ctx in ("cond", "uncond"):
            ys = _ys()
            plan, (out,) = _forward(m, ctx, ys)
            seg = plan.segs[0]
            assert (seg.compute["self"], seg.compute["cross"]) == (want_self[it], want_cross[it]), (it, ctx)
            for kind, want in (("self", want_self), ("cross", want_cross)):
                for li in range(3):
                    # computed: the module's own output; re-used: what the module handed on at its previous forward
                    exp = ys[kind][li] if want[it] else last[ctx][kind, li]
                    assert torch.equal(out[kind, li], exp), (it, ctx, kind, li)
            last[ctx] = out
    assert calls == [t for t in TIMESTEPS for _ in range(2)]              # the callback: exactly once per forward
    log = m.cache_log
    assert len(log) == 16 and log[0] == ("cond", 0, 999.0, True, True) and log[1] == ("uncond", 0, 999.0, True, True)
    assert [e[3] for e in log if e[0] == "cond"] == want_self and [e[4] for e in log if e[0] == "uncond"] == want_cross
    assert [e[1] for e in log if e[0] == "uncond"] == list(range(8)) and all(isinstance(e[2], float) for e in log)
    st = m._step_cache_states["cond"]
    assert st.iteration == {"self": 8, "cross": 8} and len(st.buffers) == 6       # counters advanced outside the range too


def test_counter_and_cache_advance_outside_the_range():
    """iterations 0 .. 2 outside the range compute (and refresh the cache); the first in-range forward is iteration 3: with N = 3
    it computes (3 % 3 == 0), with N = 2 it re-uses what iteration 2 -- an out-of-range forward -- left"""
    for n, reuse_at_3 in ((3, False), (2, True)):
        m = _model()
        now = {"t": 900}
        m.enable_cache(PyramidAttentionBroadcastConfig(spatial_attention_block_skip_range=n,
                                                       current_timestep_callback=lambda: now["t"]))
        outs = []
        for t in (900, 850, 820, 500):
            now["t"] = t
            ys = _ys()
            plan, (out,) = _forward(m, "c", ys)
            outs.append((ys, out, plan.segs[0].compute["self"]))
        assert [o[2] for o in outs] == [True, True, True, not reuse_at_3]
        want = outs[2][0]["self"][1] if reuse_at_3 else outs[3][0]["self"][1]
        assert torch.equal(outs[3][1]["self", 1], want)


def test_a_none_range_is_never_hooked():
    m = _model()
    m.enable_cache(PyramidAttentionBroadcastConfig(cross_attention_block_skip_range=2, current_timestep_callback=lambda: 500))
    for it in range(4):
        ys = _ys()
        plan, (out,) = _forward(m, "c", ys)
        assert plan.hooked == {"self": False, "cross": True}
        assert plan.segs[0].compute["self"] is True and plan.segs[0].compute["cross"] is (it % 2 == 0)
        assert torch.equal(out["self", 0], ys["self"][0])
    st = m._step_cache_states["c"]
    assert all(k == "cross" for k, _ in st.buffers) and [e[3] for e in m.cache_log] == [True] * 4


def test_a_batch_with_one_context_per_element():
    m = _model()
    m.enable_cache(PyramidAttentionBroadcastConfig(spatial_attention_block_skip_range=2, current_timestep_callback=lambda: 500))
    _forward(m, "uncond", _ys())                           # "uncond" is one forward ahead of "cond"
    ys = _ys(rows=8)
    plan, outs = _forward(m, "cfg", ys, contexts=("cond", "uncond"), b=2)
    assert [(s.name, s.r0, s.r1, s.compute["self"]) for s in plan.segs] == [("cond", 0, 4, True), ("uncond", 4, 8, False)]
    assert torch.equal(outs[0]["self", 2], ys["self"][2][:4]) and not torch.equal(outs[1]["self", 2], ys["self"][2][4:])
    with pytest.raises(ValueError, match="No context is set"):
        m._pab_begin(1, 4, 8, torch.float32, "cpu")


def test_reset_semantics():
    m = _model()
    m.ops = _FakeOps()
    m.enable_cache(PyramidAttentionBroadcastConfig(spatial_attention_block_skip_range=2, current_timestep_callback=lambda: 500))
    for _ in range(2):
        _forward(m, "c", _ys())
    assert [e[3] for e in m.cache_log] == [True, False]
    m._reset_stateful_cache()                              # the end of a pipeline call: state gone, the log stays ...
    assert m._step_cache_states == {} and len(m.cache_log) == 2
    plan, _ = _forward(m, "c", _ys())                      # ... until the next forward, which starts at iteration 0
    assert plan.segs[0].compute["self"] and m.cache_log == [("c", 0, 500.0, True, True)]
    _forward(m, "c", _ys())
    m.reset_caches()                                       # weights / dtype / device changed
    assert m._step_cache_states == {}
    _forward(m, "c", _ys())
    _forward(m, "c", _ys())
    # another shape under the same context starts over (rows, width, dtype, device are the state's key)
    plan, _ = _forward(m, "c", _ys(rows=6), rows=6)
    assert plan.segs[0].compute["self"] and m.cache_log[-1][1] == 0
    with pytest.raises(KeyError, match="no cached output"):
        m._pab_buffer(plan.segs[0], "self", 7)
    m.disable_cache()
    assert m._step_cache_states == {}


# ------------------------------------------------------------------ pipeline limits
def test_pipeline_limits_and_reset():
    from tests.test_step_cache_cpu import _pipe
    pipe = _pipe()
    tr = pipe.transformer
    tr.enable_cache(PyramidAttentionBroadcastConfig(spatial_attention_block_skip_range=2,
                                                    current_timestep_callback=lambda: pipe.current_timestep))
    assert pipe._step_cache_check(1) is True and pipe._step_cache_check(2) is True        # a batch is allowed
    pipe.use_hip_graph = True
    with pytest.raises(RuntimeError, match="use_hip_graph=True"):
        pipe._step_cache_check(1)
    pipe.use_hip_graph = None
    pipe.parallel = object()
    with pytest.raises(NotImplementedError, match="parallel plan"):
        pipe._step_cache_check(1)
    pipe.parallel = None
    pipe._current_timestep = torch.tensor(500.0)           # (the denoise loop sets it before every step)
    _forward(tr, "cond", _ys())
    assert tr._step_cache_states and tr.cache_log == [("cond", 0, 500.0, True, True)]
    pipe.maybe_free_model_hooks()
    assert tr._step_cache_states == {} and len(tr.cache_log) == 1


def test_a_token_sharded_forward_is_refused():
    m = _model()
    m.enable_cache(PyramidAttentionBroadcastConfig(spatial_attention_block_skip_range=2, current_timestep_callback=lambda: 500))

    class _Shard:
        active = True

        def rows(self, L):
            return 0, L // 2, L // 2

    with pytest.raises(NotImplementedError, match="one GPU"):
        next(m.forward_steps(torch.zeros(1, 4, 2, 4, 4), torch.tensor([500.0]), torch.zeros(1, 3, 8), shard=_Shard()))
