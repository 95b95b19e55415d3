"""Pyramid Attention Broadcast on the CogVideoX DiT, the part that needs no GPU: the CacheMixin surface with every refusal and
warning, the state machine driven through the model's real forward on a stand-in kernel front end that computes nothing (it hands
out zero tensors of the right shapes and counts the calls), contexts, reset semantics, the pipelines' limits, the one-launch
`keep=` route of the MX linears and the new entry points in header and ctypes table."""
import collections
import warnings

import pytest
import torch

from frameino_amd.step_cache import FirstBlockCacheConfig, PyramidAttentionBroadcastConfig, pab_decide
from tests.cog_window_attn_ref import FRAMES, L, LAT_H, LAT_W, TEXT, TINY_CFG

LAYERS = TINY_CFG["num_layers"]
D = TINY_CFG["num_attention_heads"] * TINY_CFG["attention_head_dim"]
TIMESTEPS = [999, 900, 790, 600, 400, 200, 100, 50]


class _StubOps:
    """every kernel the forward launches, as a no-op: results are zeros of the shape the kernel returns, `out=` is handed back"""
    EPI_NONE, EPI_GELU_TANH, EPI_RESIDUAL, EPI_GATED_RESIDUAL, EPI_GATED_RESIDUAL_STAGED = 0, 1, 2, 3, 4

    def __init__(self):
        self.calls = collections.Counter()
        self.kept = []                     # the keep= buffers the out-projections were given
        self.reused = []                   # (y, staged) of the gated_residual calls that read a cached y

    def skinny_linear(self, x, w, b=None, silu_input=False):
        self.calls["skinny_linear"] += 1
        return torch.zeros(x.shape[0], w.shape[0])

    def gemm(self, a, w, bias=None, epilogue=0, residual=None, gate=None, sel=None, out=None, keep=None, **kw):
        self.calls["gemm"] += 1
        if keep is not None:
            assert epilogue == self.EPI_GATED_RESIDUAL_STAGED and keep.shape == out.shape
            self.kept.append(keep)
        return out if out is not None else torch.zeros(a.shape[0], w.shape[0], dtype=a.dtype)

    def patchify(self, x, patch):
        c, f, h, w = x.shape
        return torch.zeros(f * (h // patch[1]) * (w // patch[2]), c * patch[1] * patch[2], dtype=x.dtype)

    def gated_residual(self, x, y, gate=None, sel=None, out=None, staged=False):
        self.calls["gated_residual"] += 1
        if gate is not None:
            self.reused.append((y, staged))
        return out

    def layernorm_zero(self, x, *a, **k):
        self.calls["layernorm_zero"] += 1
        return torch.zeros_like(x)

    def layernorm(self, x, *a, **k):
        return torch.zeros_like(x)

    def headnorm_rope_(self, *a, **k):
        self.calls["headnorm_rope_"] += 1

    def attention(self, q, k, v, heads, **kw):
        self.calls["attention"] += 1
        return torch.zeros(q.shape[0], q.shape[1], q.shape[2], dtype=q.dtype)


def _tiny_model(**over):
    from frameino_amd.cogvideox_transformer_3d import CogVideoXTransformer3DModel
    m = CogVideoXTransformer3DModel(**{**TINY_CFG, **over})
    m.ops = _StubOps()
    return m


def _pab(n=2, cb=lambda: 500, **kw):
    return PyramidAttentionBroadcastConfig(spatial_attention_block_skip_range=n, current_timestep_callback=cb, **kw)


def _forward(m, ctx="cond_uncond", batch=2, **kw):
    x, txt, ts = torch.zeros(batch, FRAMES, 6, LAT_H, LAT_W), torch.zeros(batch, TEXT, 16), torch.zeros(batch)
    with m.cache_context(ctx):
        return m(x, txt, ts, return_dict=False, **kw)[0]


# ------------------------------------------------------------------ surface
def test_the_cache_mixin_surface_and_exclusivity():
    m = _tiny_model()
    assert not m.is_cache_enabled and m.cache_log == ()
    with pytest.warns(UserWarning, match="nothing to disable"):
        m.disable_cache()
    m.enable_cache(_pab())
    assert m.is_cache_enabled and m._pab_on
    with pytest.raises(ValueError, match="already been enabled"):
        m.enable_cache(_pab(3))
    with pytest.raises(ValueError, match="already been enabled"):
        m.enable_cache(FirstBlockCacheConfig())
    m.disable_cache()
    assert not m.is_cache_enabled
    m.enable_cache(_pab(3))                                # ... and again after disable_cache
    assert callable(m._reset_stateful_cache) and callable(m.cache_context)


def test_first_block_caching_and_the_other_configs_are_refused():
    m = _tiny_model()
    with pytest.raises(NotImplementedError, match="CogVideoXTransformer3DModel.*PyramidAttentionBroadcastConfig is"):
        m.enable_cache(FirstBlockCacheConfig())

    class FirstBlockCacheConfig2:                          # what diffusers' own class looks like from here
        threshold = 0.1
    FirstBlockCacheConfig2.__name__ = "FirstBlockCacheConfig"
    with pytest.raises(NotImplementedError, match="FirstBlockCacheConfig is not implemented"):
        m.enable_cache(FirstBlockCacheConfig2())
    for name in ("FasterCacheConfig", "TaylorSeerCacheConfig", "MagCacheConfig", "TeaCacheConfig"):
        with pytest.raises(NotImplementedError, match=f"{name}.*PyramidAttentionBroadcastConfig is$"):
            m.enable_cache(type(name, (), {})())
    with pytest.raises(NotImplementedError, match="PyramidAttentionBroadcastConfig"):       # the name without the attributes
        m.enable_cache(type("PyramidAttentionBroadcastConfig", (), {})())
    for bad in (object(), {"spatial_attention_block_skip_range": 2}, None):
        with pytest.raises(ValueError, match="is not supported"):
            m.enable_cache(bad)
    assert not m.is_cache_enabled


def test_a_missing_callback_raises_and_all_none_defaults_to_spatial_2():
    m = _tiny_model()
    with pytest.raises(ValueError, match="current_timestep_callback.*must be provided"):
        m.enable_cache(PyramidAttentionBroadcastConfig(spatial_attention_block_skip_range=2))
    assert not m.is_cache_enabled
    cfg = PyramidAttentionBroadcastConfig(current_timestep_callback=lambda: 500)
    with pytest.warns(UserWarning, match="spatial_attention_block_skip_range=2"):
        m.enable_cache(cfg)
    assert cfg.spatial_attention_block_skip_range == 2 and cfg.cross_attention_block_skip_range is None
    m.disable_cache()
    with warnings.catch_warnings():
        warnings.simplefilter("error")                     # a set spatial range: no warning
        m.enable_cache(_pab())


def test_a_duck_typed_config_is_accepted():
    class PyramidAttentionBroadcastConfig:                 # noqa: F811  diffusers' own class, seen from here
        def __init__(self):
            self.spatial_attention_block_skip_range = 2
            self.temporal_attention_block_skip_range = None
            self.cross_attention_block_skip_range = None
            self.spatial_attention_timestep_skip_range = (100, 800)
            self.temporal_attention_timestep_skip_range = (100, 800)
            self.cross_attention_timestep_skip_range = (100, 800)
            self.current_timestep_callback = lambda: 500

    m = _tiny_model()
    m.enable_cache(PyramidAttentionBroadcastConfig())
    assert m.is_cache_enabled and m._pab_on


@pytest.mark.parametrize("field", ["temporal_attention_block_skip_range", "cross_attention_block_skip_range"])
def test_temporal_and_cross_ranges_match_no_layer(field):
    """accepted, hooks nothing, warns once (at enable_cache): every forward computes, no buffer is made, the callback is still
    read once per forward and logged"""
    m = _tiny_model()
    reads = []
    cfg = PyramidAttentionBroadcastConfig(current_timestep_callback=lambda: reads.append(1) or 500, **{field: 2})
    with pytest.warns(UserWarning, match="hooks nothing"):
        m.enable_cache(cfg)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                     # once: the forwards are silent
        for _ in range(3):
            _forward(m)
    assert m.ops.calls["attention"] == 3 * LAYERS and m.ops.kept == [] and m.ops.reused == []
    assert m._step_cache_states["cond_uncond"].buffers == {}
    assert m.cache_log == [("cond_uncond", i, 500.0, True, True) for i in range(3)] and len(reads) == 3


# ------------------------------------------------------------------ the state machine, through the forward
def test_state_machine_over_a_schedule():
    """spatial N over (100, 800): the first forward computes, every N-th computes, the bounds are strict, the counter advances
    outside the range; a computing forward hands every out-projection this layer's buffer as keep=, a re-using one launches no
    norm1 / QKV / head norm / attention / out-projection and reads the same buffers through the staged residual"""
    C, R = True, False
    for n, want in ((2, [C, C, C, R, C, R, C, C]), (3, [C, C, R, C, R, R, C, C])):
        m = _tiny_model()
        now = {"t": None, "reads": 0}

        def cb():
            now["reads"] += 1
            return now["t"]

        m.enable_cache(_pab(n, cb))
        # (the rule is `pab_decide`, unchanged: the cache fills on the first forward and stays filled)
        assert want == [pab_decide(i, t, i > 0, n, (100, 800)) for i, t in enumerate(TIMESTEPS)]
        for i, t in enumerate(TIMESTEPS):
            now["t"] = torch.tensor(float(t))              # (the pipeline's current_timestep is a tensor)
            o = m.ops = _StubOps()
            out = _forward(m, live_frames=FRAMES - 1)
            assert tuple(out.shape) == (2, FRAMES, 2, LAT_H, LAT_W) and now["reads"] == i + 1
            bufs = [m._step_cache_states["cond_uncond"].buffers["self", li] for li in range(LAYERS)]
            assert all(tuple(b.shape) == (2 * L, D) and b.dtype == torch.float32 for b in bufs)
            # per block: norm2 always, norm1 when computing; + the final AdaLayerNorm per batch element
            if want[i]:
                assert len(o.kept) == LAYERS and all(k is b for k, b in zip(o.kept, bufs)) and o.reused == []
                assert (o.calls["attention"], o.calls["headnorm_rope_"], o.calls["layernorm_zero"]) == (LAYERS, 2 * LAYERS,
                                                                                                        2 * LAYERS + 2)
            else:
                assert o.kept == [] and [staged for _, staged in o.reused] == [True] * LAYERS
                assert all(y is b for (y, _), b in zip(o.reused, bufs))
                assert (o.calls["attention"], o.calls["headnorm_rope_"], o.calls["layernorm_zero"]) == (0, 0, LAYERS + 2)
                # the GEMMs left: text + patch embedding per element, FFN up / down per block, the output head per element
                assert o.calls["gemm"] == 2 * 2 + 2 * LAYERS + 2
        assert m.cache_log == [("cond_uncond", i, float(t), w, True) for i, (t, w) in enumerate(zip(TIMESTEPS, want))]
        assert all(type(e[2]) is float for e in m.cache_log)
        assert m._step_cache_states["cond_uncond"].iteration["self"] == len(TIMESTEPS)


def test_the_last_block_runs_every_row_under_the_cache():
    """`skip_dead_rows`: without the cache the last block's out-projection and FFN run per batch element on the live rows only;
    with it every block is the same whole-batch launch sequence, and the returned frames are the same"""
    plain, cached = _tiny_model(), _tiny_model()
    cached.enable_cache(_pab())
    a, b = _forward(plain, live_frames=FRAMES - 1), _forward(cached, live_frames=FRAMES - 1)
    assert plain.skip_dead_rows and a.shape == b.shape
    assert plain.ops.calls["gemm"] == 2 * 2 + 4 + 1 + 2 * 3 + 2          # block 0 whole, block 1: QKV + per element 3, heads
    assert cached.ops.calls["gemm"] == 2 * 2 + 4 * LAYERS + 2
    assert len(cached.ops.kept) == LAYERS


def test_a_forward_needs_a_context_and_contexts_are_independent():
    m = _tiny_model()
    m.enable_cache(_pab())
    x, txt, ts = torch.zeros(1, FRAMES, 6, LAT_H, LAT_W), torch.zeros(1, TEXT, 16), torch.zeros(1)
    with pytest.raises(ValueError, match="No context is set"):
        m(x, txt, ts)
    assert m.ops.calls == {} and m.cache_log == ()          # raised before any launch
    for ctx in ("a", "b", "a", "b"):
        _forward(m, ctx)
    assert [(e[0], e[1], e[3]) for e in m.cache_log] == [("a", 0, True), ("b", 0, True), ("a", 1, False), ("b", 1, False)]
    assert m._step_cache_states["a"].buffers["self", 0] is not m._step_cache_states["b"].buffers["self", 0]
    with m.cache_context("outer"):
        with m.cache_context("inner"):
            assert m._ctx_name == "inner"
        assert m._ctx_name == "outer"
    assert m._ctx_name is None
    m.disable_cache()
    m(x, txt, ts)                                           # no cache: no context needed


def test_a_changed_shape_starts_over():
    m = _tiny_model()
    m.enable_cache(_pab())
    _forward(m)
    _forward(m)
    _forward(m, batch=1)                                    # other rows under the same context: iteration 0, computes
    _forward(m, batch=1)
    assert m._step_cache_states["cond_uncond"].buffers["self", 1].shape[0] == L
    _forward(m)                                             # ... and back: over again
    assert [(e[1], e[3]) for e in m.cache_log] == [(0, True), (1, False), (0, True), (1, False), (0, True)]
    assert m._step_cache_states["cond_uncond"].buffers["self", 1].shape[0] == 2 * L
    st = m._step_cache_states["cond_uncond"]
    m.double()                                              # another dtype: the parameters changed, every state is dropped
    assert m._step_cache_states == {} and st.key[2] == torch.float32


def test_reset_semantics_and_the_lifetime_of_cache_log():
    m = _tiny_model()
    m.enable_cache(_pab())
    _forward(m)
    _forward(m)
    assert [e[3] for e in m.cache_log] == [True, False]
    m._reset_stateful_cache()                              # the end of a pipeline call: state gone, the log stays ...
    assert m._step_cache_states == {} and len(m.cache_log) == 2
    _forward(m)                                            # ... until the next forward, which starts at iteration 0
    assert m.cache_log == [("cond_uncond", 0, 500.0, True, True)]
    _forward(m)
    m.reset_caches()                                       # weights / dtype / device changed: the buffers go
    assert m._step_cache_states == {}
    _forward(m)
    assert m.cache_log[-1][1:4] == (0, 500.0, True)
    m.disable_cache()
    assert m._step_cache_states == {}


# ------------------------------------------------------------------ the pipelines
def test_the_pipelines_refuse_a_required_graph_and_reset_the_state():
    from frameino_amd.pipeline_cogvideox_i2v_motion import CogVideoXImageToVideoPipeline as Stage1
    from frameino_amd.pipeline_cogvideox_i2v_motion_frameino import CogVideoXImageToVideoPipeline as Pipe
    for cls in (Pipe, Stage1):
        m = _tiny_model()
        pipe = cls(transformer=m)
        assert pipe.current_timestep is None and pipe._step_cache_check() is False
        m.enable_cache(_pab(cb=lambda: pipe.current_timestep))
        assert pipe._step_cache_check() is True                              # the loop runs eagerly
        pipe.use_hip_graph = True
        with pytest.raises(RuntimeError, match="use_hip_graph=True with Pyramid Attention Broadcast"):
            pipe._step_cache_check()
        with pytest.raises(RuntimeError, match="use_hip_graph=True"):      # denoise: before any work
            pipe.denoise(torch.zeros(1, 2, 2, 4, 6), *([None] * 4 if cls is Pipe else [None] * 3), None)
        m.disable_cache()
        assert pipe._step_cache_check() is False                             # graph mode returns
        pipe.use_hip_graph = None
        m.enable_cache(_pab(cb=lambda: pipe.current_timestep))
        pipe._current_timestep = torch.tensor(500.0)
        _forward(m)
        assert m._step_cache_states and m.cache_log == [("cond_uncond", 0, 500.0, True, True)]
        pipe.maybe_free_model_hooks()
        assert m._step_cache_states == {} and len(m.cache_log) == 1


# ------------------------------------------------------------------ the MX linears' keep= and the library's surface
@pytest.mark.parametrize("fmt", [8, 6])
def test_an_mx_linear_keeps_y_in_one_launch(fmt):
    """`_lin(keep=)` on an MX weight: ONE gemm_mxfp8 / gemm_mxfp6 call with keep= for each residual epilogue (the staged one
    included), no EPI_NONE GEMM and no separate residual pass"""
    from frameino_amd.mx_linears import MXLinearsMixin
    seen = []

    class Ops(_StubOps):
        def quantize_mxfp8(self, x):
            return "xq", "xs"
        quantize_mxfp6 = quantize_mxfp8

        def gemm_mxfp8(self, *a, **kw):
            seen.append((a, kw))
            return kw["out"]
        gemm_mxfp6 = gemm_mxfp8

        def pab_broadcast(self, *a, **k):
            raise AssertionError("a second launch")

    class M(MXLinearsMixin):
        ops = Ops()
    m = M()
    m._fp8, m._mx_fmt = {(0, "out"): ("wq", "ws")}, fmt
    keep, x = object(), object()
    for epi in (Ops.EPI_RESIDUAL, Ops.EPI_GATED_RESIDUAL, Ops.EPI_GATED_RESIDUAL_STAGED):
        seen.clear()
        assert m._lin(0, "out", "x", "w", "b", epi, residual=x, gate="g", sel="s", out=x, keep=keep) is x
        (a, kw), = seen
        assert a == ("xq", "xs", "wq", "ws", "b", epi) and kw["keep"] is keep and kw["residual"] is x
    seen.clear()
    m._lin(0, "out", "x", "w", "b", Ops.EPI_GATED_RESIDUAL_STAGED, residual=x, gate="g", sel="s", out=x)
    assert "keep" not in seen[0][1]


def test_the_new_entry_points_are_in_header_and_ctypes_table():
    import inspect
    from frameino_amd import _lib, ops
    declared = _lib.declared_symbols()
    for fmt in ("mxfp8", "mxfp6"):
        name = f"fino_gemm_{fmt}_keep"
        assert name in declared and name in _lib.SIGNATURES
        plain, keep = _lib.SIGNATURES[f"fino_gemm_{fmt}"], _lib.SIGNATURES[name]
        assert keep[:len(plain) - 1] == plain[:-1] and len(keep) == len(plain) + 2           # + void* keep, int64 ldk
        assert "keep" in inspect.signature(getattr(ops, f"gemm_{fmt}")).parameters
    assert _lib.ABI_VERSION == 103


@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp6"])
def test_argument_validation_of_the_keep_entries(fmt):
    """validation happens before any launch: no GPU needed (as tests/test_lib_abi.py does for the other entry points)"""
    import os
    from frameino_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    entry = getattr(lib, f"fino_gemm_{fmt}_keep")

    def call(epi, keep=16, ldk=8, k=128):
        return entry(16, 16, 16, 16, 0, 16, 8, 8, k, 8, epi, 16, 8, 16, 0, 0, 0, keep, ldk, 0)

    for epi in (0, 1):                                     # FINO_EPI_NONE, FINO_EPI_GELU_TANH: nothing to keep beside
        assert call(epi) == -1 and b"residual epilogues" in lib.fino_last_error() and fmt.encode() in lib.fino_last_error()
    assert call(9) == -1 and b"epilogue" in lib.fino_last_error()
    for epi in (2, 3, 4):
        for bad in (dict(keep=0), dict(keep=24), dict(ldk=4), dict(ldk=12)):     # null, misaligned, ldk < N, ldk % 8
            assert call(epi, **bad) == -1 and b"keep buffer" in lib.fino_last_error(), (epi, bad)
    assert call(2, k=64) == -1 and b"multiple of 128" in lib.fino_last_error()   # the checks of the entry without keep stay
