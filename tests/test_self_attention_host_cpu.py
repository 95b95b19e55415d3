"""The self-attention host path the Wan and CogVideoX DiTs share (SelfAttentionOptionsMixin, frameino_amd/window_attention.py),
without a GPU: which of `ops.attention` / `attention_ranges` / `attention_fp8` / `attention_fp8_ranges` every block calls and
with which fp8 options, the state a fresh model starts with, the `live_rows` gate of the Wan DiT, and the pipelines' rule about a
timestep range.  The forwards run on recording stand-ins for `ops`."""
import pytest
import torch

from frameino_amd.window_attention import WindowAttentionConfig
from tests import cpu_ops
from tests.test_pab_cog_cpu import _StubOps

SELF_ATTENTION = ("attention", "attention_ranges", "attention_fp8", "attention_fp8_ranges")
FP8 = dict(p_mode="exp2", smooth_k=True, smooth_v=True)
# 3 latent frames of 16 x 8 = 128 tokens: 384 rows, two q-blocks; with window_frames = 0 the first sees frames 0 - 1 only
WAN_L = 384


class _WanOps:
    """tests/cpu_ops.py, plus the three other self-attention names answered by its `attention`; notes every call to one of the four
    as (name, query rows, key rows, keyword arguments)"""

    def __init__(self, missing=()):
        self.calls, self._missing = [], set(missing)

    def __getattr__(self, name):
        if name in self._missing or (name not in SELF_ATTENTION and not hasattr(cpu_ops, name)):
            raise AttributeError(name)
        if name not in SELF_ATTENTION:
            return getattr(cpu_ops, name)

        def call(q, k, v, heads, *ranges, out=None, scale=None, **kw):
            assert len(ranges) == (1 if name.endswith("ranges") else 0)
            self.calls.append((name, q.shape[1], k.shape[1], kw))
            return cpu_ops.attention(q, k, v, heads, out=out, scale=scale)
        self.__dict__[name] = call          # one object per name, as a module's functions are
        return call

    def self_attention(self):
        return [c for c in self.calls if c[2] == WAN_L]          # (the text cross-attention has 12 keys)


class _CogOps(_StubOps):
    """the no-op stand-in of tests/test_pab_cog_cpu.py with all four self-attention names, each noted as above"""

    def __init__(self):
        super().__init__()
        self.attn = []

    def _note(self, name, q, k, kw):
        self.attn.append((name, q.shape[1], k.shape[1], {n: v for n, v in kw.items() if n != "scale"}))
        return torch.zeros(q.shape, dtype=q.dtype)

    def attention(self, q, k, v, heads, **kw):
        return self._note("attention", q, k, kw)

    def attention_ranges(self, q, k, v, heads, ranges, **kw):
        return self._note("attention_ranges", q, k, kw)

    def attention_fp8(self, q, k, v, heads, **kw):
        return self._note("attention_fp8", q, k, kw)

    def attention_fp8_ranges(self, q, k, v, heads, ranges, **kw):
        return self._note("attention_fp8_ranges", q, k, kw)


def _wan(ops=None):
    from frameino_amd.transformer_wan import WanTransformer3DModel
    torch.manual_seed(0)
    m = WanTransformer3DModel(num_attention_heads=1, attention_head_dim=128, in_channels=4, out_channels=4, text_dim=32,
                              freq_dim=32, ffn_dim=64, num_layers=2).float().eval()
    m.ops = ops if ops is not None else _WanOps()
    return m


def _wan_forward(m, **kw):
    g = torch.Generator().manual_seed(1)
    x, txt = torch.randn(1, 4, 3, 32, 16, generator=g), torch.randn(1, 12, 32, generator=g)
    return m(x, torch.tensor([500.0]), txt, return_dict=False, **kw)[0]


def _cog():
    from frameino_amd.cogvideox_transformer_3d import CogVideoXTransformer3DModel
    from tests.cog_window_attn_ref import TINY_CFG
    m = CogVideoXTransformer3DModel(**{**TINY_CFG, "sample_frames": 9, "use_FrameIn": False})     # 2 blocks, 2 heads x 64
    m.ops = _CogOps()
    return m


def _cog_forward(m, **kw):
    # 8 text rows + 3 latent frames of 150 tokens = 458 rows, two q-blocks
    return m(torch.zeros(1, 3, 6, 20, 30), torch.zeros(1, 8, 16), torch.zeros(1), return_dict=False, **kw)[0]


# window_frames = 0 without sink frames leaves key tiles out on both geometries; 3 covers the clip
WINDOWS = {"dense": None, "windowed": WindowAttentionConfig(0, sink_frames=()), "skip": WindowAttentionConfig(0, (), skip_layers=(1,)),
           "cover": WindowAttentionConfig(3)}


# ------------------------------------------------------------------ dispatch matrix
@pytest.mark.parametrize("window,fp8,names", [
    ("dense", False, ["attention", "attention"]), ("windowed", False, ["attention_ranges", "attention_ranges"]),
    ("skip", False, ["attention_ranges", "attention"]), ("cover", False, ["attention", "attention"]),
    ("dense", True, ["attention_fp8", "attention_fp8"])])
def test_wan_dispatch(window, fp8, names):
    m = _wan()
    if fp8:
        assert m.enable_fp8_attention(**FP8) is m
    if WINDOWS[window] is not None:
        m.enable_window_attention(WINDOWS[window])
    out = _wan_forward(m)
    assert torch.isfinite(out).all()
    calls = m.ops.self_attention()
    assert [c[0] for c in calls] == names
    for name, lq, lk, kw in calls:
        assert (lq, lk) == (WAN_L, WAN_L)
        assert kw == (FP8 if "fp8" in name else {})              # exactly the model's fp8 options, and only on the fp8 calls


def test_wan_refuses_fp8_with_windows_and_falls_back_without_the_fp8_kernel():
    m = _wan()
    m.enable_fp8_attention(**FP8)
    with pytest.raises(NotImplementedError, match="fp8 attention"):
        m.enable_window_attention(WINDOWS["windowed"])
    m = _wan(_WanOps(missing=("attention_fp8",)))                # a front end without the fp8 kernel: the dense bf16 call, as before
    m.enable_fp8_attention(**FP8)
    _wan_forward(m)
    assert [(c[0], c[3]) for c in m.ops.self_attention()] == [("attention", {}), ("attention", {})]


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("window,kinds", [("dense", [False, False]), ("windowed", [True, True]), ("skip", [True, False]),
                                          ("cover", [False, False])])
def test_cog_dispatch(window, kinds, fp8):
    m = _cog()
    if fp8:
        assert m.enable_fp8_attention(**FP8) is m
    if WINDOWS[window] is not None:
        m.enable_window_attention(WINDOWS[window])
    _cog_forward(m)
    stem = "attention_fp8" if fp8 else "attention"
    assert [c[0] for c in m.ops.attn] == [stem + ("_ranges" if ranged else "") for ranged in kinds]
    for name, lq, lk, kw in m.ops.attn:
        assert lk == 458 and kw == (FP8 if fp8 else {})
    # bf16: the last block's queries are the video rows; fp8 attention runs every row of every block
    assert [c[1] for c in m.ops.attn] == ([458, 458] if fp8 else [458, 450])


# ------------------------------------------------------------------ defaults
@pytest.mark.parametrize("make", [_wan, _cog])
def test_a_fresh_model_has_every_option_off(make):
    m = make()
    assert m.fp8_attention is False and m.fp8_p_mode is None and m.fp8_smooth_k is False and m.fp8_smooth_v is False
    assert m.window_attention_log == [] and not m.is_window_attention_enabled and not m.window_attention_is_timestep_gated
    assert m.enable_fp8_attention() is m and m.fp8_attention is True and m.fp8_p_mode is None
    assert m.enable_fp8_attention(False) is m and m.fp8_attention is False


# ------------------------------------------------------------------ live rows (Wan): windows alone keep the gate open, fp8 closes it
def test_wan_live_rows_are_honoured_with_windows_but_not_with_fp8():
    live = (128, 384)
    m = _wan()
    m.enable_window_attention(WINDOWS["windowed"])
    out = _wan_forward(m, live_rows=live)
    assert [(c[0], c[1]) for c in m.ops.self_attention()] == [("attention_ranges", WAN_L), ("attention_ranges", 256)]
    assert not out[:, :, 0].any() and out[:, :, 1:].any()        # the dead rows (frame 0) come back zero
    m = _wan()
    m.enable_fp8_attention()
    out = _wan_forward(m, live_rows=live)
    assert [(c[0], c[1]) for c in m.ops.self_attention()] == [("attention_fp8", WAN_L), ("attention_fp8", WAN_L)]
    assert out[:, :, 0].any()


# ------------------------------------------------------------------ the pipelines' rule
def _pipes():
    from frameino_amd.pipeline_cogvideox_i2v_motion_frameino import CogVideoXImageToVideoPipeline as CogPipe
    from frameino_amd.pipeline_wan_i2v_motion_frameino import WanImageToVideoPipeline as WanPipe
    wan = WanPipe.__new__(WanPipe)
    wan.transformer = _wan()
    return [wan, CogPipe(transformer=_cog())]


@pytest.mark.parametrize("which", [0, 1])
def test_the_pipelines_read_the_public_property(which):
    pipe = _pipes()[which]
    m = pipe.transformer
    pipe.use_hip_graph = True
    assert m.window_attention_is_timestep_gated is False and pipe._window_attention_check() is False      # off
    m.enable_window_attention(WindowAttentionConfig(1))
    assert m.window_attention_is_timestep_gated is False and pipe._window_attention_check() is False      # a static table
    m.enable_window_attention(WindowAttentionConfig(1, timestep_range=(100, 800), current_timestep_callback=lambda: 500))
    assert m.window_attention_is_timestep_gated is True
    with pytest.raises(RuntimeError, match="use_hip_graph=True with window attention"):
        pipe._window_attention_check()
    pipe.use_hip_graph = None
    assert pipe._window_attention_check() is True                                                        # the loop runs eagerly
    m.disable_window_attention()
    assert m.window_attention_is_timestep_gated is False and pipe._window_attention_check() is False


def test_the_wan_pipeline_refuses_a_parallel_plan():
    pipe = _pipes()[0]
    pipe.use_hip_graph, pipe.parallel = None, object()
    assert pipe._window_attention_check() is False               # window attention off: the plan is no concern of this check
    pipe.transformer.enable_window_attention(WindowAttentionConfig(1))
    with pytest.raises(NotImplementedError, match="one GPU"):
        pipe._window_attention_check()
