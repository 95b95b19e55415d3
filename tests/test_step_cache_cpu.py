"""First-block caching without a GPU: the CacheMixin surface, the per-context state machine (fed synthetic probe sums through a
stand-in for the kernel front end), the host rounding of the decision against torch, and the pipeline's limits."""
import math

import pytest
import torch

from frameino_amd.step_cache import FirstBlockCacheConfig, decide


def _model(layers=3):
    from frameino_amd.transformer_wan import WanTransformer3DModel
    return WanTransformer3DModel(num_attention_heads=2, attention_head_dim=16, in_channels=4, out_channels=4, text_dim=8,
                                 freq_dim=8, ffn_dim=32, num_layers=layers)


class _FakeOps:
    """the two step-cache entries of frameino_amd.ops in plain torch; the probe's sums come from `queue`"""

    def __init__(self):
        self.queue, self.seen_p = [], []

    def step_cache_probe(self, h0, h1, p, r, h1_copy):
        for a, b, rr, c in zip(h0, h1, r, h1_copy):
            rr.copy_(b - a)
            c.copy_(b)
        self.seen_p.append([None if t is None else t.clone() for t in p])
        return torch.tensor(self.queue.pop(0), dtype=torch.float32)

    def step_cache_residual(self, a, b, out=None, subtract=True):
        return out.copy_(a - b if subtract else a + b)


def _drive(m, name, h0, h1, hn, sums):
    """one forward's cache steps on synthetic rows: probe after block 0 (sums -> the decision), finish after the last block"""
    m.ops.queue.append(sums)
    x = h1.clone()
    h1c = torch.empty_like(h1)
    with m.cache_context(name):
        segs = m._step_cache_segments(1, h0.shape[0])
    computes = m._step_cache_probe(segs, h0, x, h1c)
    if any(computes):
        x.copy_(hn)
    m._step_cache_finish(segs, computes, x, h1c)
    return computes[0], x


# ------------------------------------------------------------------ surface
def test_enable_disable_and_is_cache_enabled():
    m = _model()
    assert not m.is_cache_enabled
    m.enable_cache(FirstBlockCacheConfig(threshold=0.1))
    assert m.is_cache_enabled
    with pytest.raises(ValueError, match="already been enabled"):
        m.enable_cache(FirstBlockCacheConfig())
    m.disable_cache()
    assert not m.is_cache_enabled
    with pytest.warns(UserWarning, match="nothing to disable"):
        m.disable_cache()
    assert FirstBlockCacheConfig().threshold == 0.05


def test_unsupported_configs_are_refused():
    m = _model()

    class FasterCacheConfig:
        pass

    class PyramidAttentionBroadcastConfig:
        pass

    for cfg in (FasterCacheConfig(), PyramidAttentionBroadcastConfig()):
        with pytest.raises(NotImplementedError, match=type(cfg).__name__):
            m.enable_cache(cfg)
    with pytest.raises(ValueError, match="is not supported"):
        m.enable_cache(object())
    assert not m.is_cache_enabled


def test_a_duck_typed_config_is_accepted():
    class FirstBlockCacheConfig:          # what diffusers' own class looks like from here
        def __init__(self, threshold):
            self.threshold = threshold

    m = _model()
    m.enable_cache(FirstBlockCacheConfig(0.2))
    assert m.is_cache_enabled


def test_a_single_block_model_is_refused():
    with pytest.raises(ValueError, match="1 block"):
        _model(layers=1).enable_cache(FirstBlockCacheConfig())


def test_a_forward_outside_a_context_raises():
    m = _model()
    m.enable_cache(FirstBlockCacheConfig())
    with pytest.raises(ValueError, match="No context is set"):
        m._step_cache_segments(1, 8)
    with m.cache_context("cond"):
        assert m._step_cache_segments(2, 8) == [("cond", 0, 16)]
    assert m._step_cache_segments(2, 8, ("cond", "uncond")) == [("cond", 0, 8), ("uncond", 8, 16)]
    m.disable_cache()
    assert m._step_cache_segments(1, 8) is None           # no cache: nothing to do, no context needed


# ------------------------------------------------------------------ state machine
def test_state_machine_on_synthetic_diffs():
    torch.manual_seed(0)
    m = _model()
    m.ops = _FakeOps()
    m.enable_cache(FirstBlockCacheConfig(threshold=0.5))
    rows, d = 4, 8
    rnd = lambda: torch.randn(rows, d)           # noqa: E731
    n = rows * d
    # 1. the first call computes, whatever the sums say
    h0, h1, hn = rnd(), rnd(), rnd()
    c, out = _drive(m, "cond", h0, h1, hn, [[0.0, 1.0]])
    st = m._step_cache_states["cond"]
    assert c and torch.equal(out, hn) and torch.equal(st.head, h1 - h0) and torch.equal(st.tail, hn - h1)
    head1, tail1 = st.head.clone(), st.tail.clone()
    # 2. diff 0.25 <= 0.5: skip -- output tail + h1, head residual unchanged, the probe compared against head1
    h0b, h1b = rnd(), rnd()
    c, out = _drive(m, "cond", h0b, h1b, None, [[0.25 * n, 1.0 * n]])
    assert not c and torch.equal(out, tail1 + h1b)
    assert torch.equal(st.head, head1) and torch.equal(st.tail, tail1)
    assert torch.equal(m.ops.seen_p[-1][0], head1)
    # 3. NaN (0/0) skips; the comparison is still against head1
    c, _ = _drive(m, "cond", rnd(), rnd(), None, [[0.0, 0.0]])
    assert not c and torch.equal(st.head, head1) and torch.equal(m.ops.seen_p[-1][0], head1)
    # 4. inf (x/0) computes
    h0c, h1c_, hnc = rnd(), rnd(), rnd()
    c, out = _drive(m, "cond", h0c, h1c_, hnc, [[1.0, 0.0]])
    assert c and torch.equal(out, hnc) and torch.equal(st.head, h1c_ - h0c)
    # 5. contexts are independent: "uncond" starts fresh and computes
    c, _ = _drive(m, "uncond", rnd(), rnd(), rnd(), [[0.0, 1.0]])
    assert c and torch.equal(st.head, h1c_ - h0c)
    log = m.cache_log
    assert [(e[0], e[1], e[3]) for e in log] == [("cond", 0, True), ("cond", 1, False), ("cond", 2, False),
                                                  ("cond", 3, True), ("uncond", 0, True)]
    assert log[0][2] is None and log[1][2] == 0.25 and math.isnan(log[2][2]) and log[3][2] == math.inf
    # 6. a reset drops every context's state; the log survives until the next forward
    m._reset_stateful_cache()
    assert m._step_cache_states == {} and len(m.cache_log) == 5
    c, _ = _drive(m, "cond", rnd(), rnd(), rnd(), [[0.0, 1.0]])
    assert c and m.cache_log == [("cond", 0, None, True)]


def test_reset_caches_and_disable_drop_the_state():
    m = _model()
    m.ops = _FakeOps()
    m.enable_cache(FirstBlockCacheConfig(threshold=0.5))
    _drive(m, "cond", torch.randn(2, 8), torch.randn(2, 8), torch.randn(2, 8), [[0.0, 1.0]])
    assert m._step_cache_states
    m.reset_caches()                              # weights / dtype / device changed
    assert m._step_cache_states == {}
    _drive(m, "cond", torch.randn(2, 8), torch.randn(2, 8), torch.randn(2, 8), [[0.0, 1.0]])
    m.disable_cache()
    assert m._step_cache_states == {}


# ------------------------------------------------------------------ host rounding
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_host_rounding_matches_torch(dtype):
    """decide() from fp32 sums == torch's `((r - p).abs().mean() / p.abs().mean()).item()` on CPU tensors of `dtype` (torch's
    CPU mean of a 16-bit tensor: fp32 sum, fp32 division, one rounding), decisions included"""
    g = torch.Generator().manual_seed(1)
    for trial in range(40):
        n = int(torch.randint(1, 5000, (1,), generator=g))
        p = (torch.randn(n, generator=g) * 10 ** float(torch.randint(-3, 3, (1,), generator=g))).to(dtype)
        r = (p.float() * (1 + 0.3 * torch.randn(n, generator=g))).to(dtype)
        dlt = r - p
        want = float(dlt.abs().mean() / p.abs().mean())
        sa = float(torch.sum(dlt.abs(), dtype=torch.float32))
        sq = float(torch.sum(p.abs(), dtype=torch.float32))
        got, compute = decide(sa, sq, n, dtype, want)
        assert got == want or (math.isnan(got) and math.isnan(want)), (trial, got, want)
        assert compute is False                              # diff > diff is False: the comparison is strict
        assert decide(sa, sq, n, dtype, math.nextafter(want, -math.inf))[1] is True
    assert math.isnan(decide(0.0, 0.0, 8, dtype, 0.1)[0]) and decide(0.0, 0.0, 8, dtype, 0.1)[1] is False
    assert decide(1.0, 0.0, 8, dtype, 0.1) == (math.inf, True)
    assert decide(1.0, 0.0, 8, dtype, math.inf)[1] is False


# ------------------------------------------------------------------ pipeline limits
def _pipe():
    from frameino_amd.pipeline_wan_i2v_motion_frameino import WanImageToVideoPipeline
    from frameino_amd.schedulers import FlowMatchEulerDiscreteScheduler
    m = _model()
    m.ops = _FakeOps()
    return WanImageToVideoPipeline(scheduler=FlowMatchEulerDiscreteScheduler(shift=5.0), transformer=m, expand_timesteps=True)


def test_pipeline_limits_and_reset():
    pipe = _pipe()
    tr = pipe.transformer
    assert pipe._step_cache_check(2) is False                 # no cache: nothing to check
    tr.enable_cache(FirstBlockCacheConfig(0.1))
    with pytest.raises(NotImplementedError, match="batch"):
        pipe.denoise(torch.zeros(2, 4, 2, 4, 4), None, None, None, None, None, None, 5.0, 2)
    pipe.use_hip_graph = True
    with pytest.raises(RuntimeError, match="use_hip_graph=True"):
        pipe._step_cache_check(1)
    pipe.use_hip_graph = None
    assert pipe._step_cache_check(1) is True
    pipe.parallel = object()
    with pytest.raises(NotImplementedError, match="parallel plan"):
        pipe._step_cache_check(1)
    pipe.parallel = None
    # maybe_free_model_hooks() (the end of __call__) drops the state and keeps the log
    _drive(tr, "cond", torch.randn(2, 8), torch.randn(2, 8), torch.randn(2, 8), [[0.0, 1.0]])
    assert tr._step_cache_states and tr.cache_log
    pipe.maybe_free_model_hooks()
    assert tr._step_cache_states == {} and len(tr.cache_log) == 1
