"""The routing of the MX linears (frameino_amd/mx_linears.py), recorded on the CPU: which front-end calls a model's public
switches and its `_lin` / `_ln_q` make, seen by a recording stand-in assigned to `m.ops`.  No kernel runs; the numbers are
tests/test_mxfp8_gpu.py's and tests/test_mxfp6_gpu.py's business."""
import pytest
import torch

from tests.test_host_cpu import _tiny


class _Recorder:
    """stands in for frameino_amd.ops: every call is noted as (name, args, kwargs) and answered with a tagged placeholder"""

    def __init__(self):
        self.calls = []

    def _note(self, name, *args, **kw):
        self.calls.append((name, args, kw))
        return len(self.calls)

    def names(self):
        return [c[0] for c in self.calls]

    def gemm(self, *args, **kw):
        return ("gemm", self._note("gemm", *args, **kw))

    def quantize_mxfp8(self, x):
        i = self._note("quantize_mxfp8", x)
        return ("q8", i), ("s8", i)

    def quantize_mxfp6(self, x):
        i = self._note("quantize_mxfp6", x)
        return ("q6", i), ("s6", i)

    def gemm_mxfp8(self, *args, **kw):
        return ("gemm_mxfp8", self._note("gemm_mxfp8", *args, **kw))

    def gemm_mxfp6(self, *args, **kw):
        return ("gemm_mxfp6", self._note("gemm_mxfp6", *args, **kw))

    def gemm_mxfp8_q(self, *args, **kw):
        i = self._note("gemm_mxfp8_q", *args, **kw)
        return ("q8", i), ("s8", i)

    def ln_mxfp8(self, mode, x, **kw):
        i = self._note("ln_mxfp8", mode, x, **kw)
        return ("q8", i), ("s8", i)


def _tiny_cog():
    from frameino_amd.cogvideox_transformer_3d import CogVideoXTransformer3DModel
    return CogVideoXTransformer3DModel(num_attention_heads=2, attention_head_dim=16, in_channels=6, out_channels=2,
                                       time_embed_dim=16, text_embed_dim=8, num_layers=1, sample_width=8, sample_height=8,
                                       sample_frames=9, max_text_seq_length=5, use_rotary_positional_embeddings=True,
                                       use_learned_positional_embeddings=True)


# (model, MX linears per block x blocks, the LayerNorm mode its _ln_q calls use)
MODELS = {"wan": (_tiny, 6 * 2, 0), "cog": (_tiny_cog, 4 * 1, 2)}


@pytest.fixture(params=sorted(MODELS))
def case(request):
    make, n_weights, ln_mode = MODELS[request.param]
    m = make()
    m.ops = rec = _Recorder()
    x, w, b = torch.zeros(3, 8), torch.zeros(5, 8), torch.zeros(5)
    return m, rec, n_weights, ln_mode, x, w, b


def test_off_goes_to_the_model_dtype_gemm_with_its_tile_height(case):
    m, rec, _, _, x, w, b = case
    out = m._lin(0, "qkv", x, w, b, 1, tile_m=4)
    assert out == ("gemm", 1) and rec.names() == ["gemm"]
    _, args, kw = rec.calls[0]
    assert args[0] is x and args[1] is w and args[2] is b and args[3] == 1 and kw == {"tile_m": 4}


def test_mxfp8_quantises_every_weight_once_and_the_activations_unless_given(case):
    m, rec, n_weights, _, x, w, b = case
    assert m.enable_mxfp8_linears() is m
    assert rec.names() == ["quantize_mxfp8"] * n_weights and len(m._fp8) == n_weights and m._mx_fmt == 8
    wq = m._fp8[(0, "qkv")]
    rec.calls.clear()
    pre = (object(), object())
    m._lin(0, "qkv", x, w, b, 3, xq=pre, tile_m=4, residual=x)
    assert rec.names() == ["gemm_mxfp8"]                              # no quantiser: the activations came quantised
    _, args, kw = rec.calls[0]
    assert args[0] is pre[0] and args[1] is pre[1] and args[2] is wq[0] and args[3] is wq[1] and args[4] is b and args[5] == 3
    assert "tile_m" not in kw and kw["residual"] is x
    rec.calls.clear()
    m._lin(0, "qkv", x, w, b)
    assert rec.names() == ["quantize_mxfp8", "gemm_mxfp8"] and rec.calls[0][1][0] is x
    assert rec.calls[1][1][:2] == (("q8", 1), ("s8", 1))


def test_one_reduced_precision_at_a_time(case):
    m, rec, n_weights, _, *_ = case
    m.enable_mxfp8_linears()
    before = dict(m._fp8)
    with pytest.raises(ValueError, match="enable_mxfp6_linears"):
        m.enable_mxfp6_linears()
    assert m.enable_mxfp6_linears(False) is m                         # the other precision's off-switch: nothing to drop
    assert m._fp8 == before and m._mx_fmt == 8 and len(rec.calls) == n_weights


def test_moving_the_parameters_defers_the_requantisation(case):
    m, rec, *_ = case
    m.enable_mxfp8_linears()
    rec.calls.clear()
    m.to(torch.float64)
    assert not m._fp8 and m._fp8_pending and m._mx_fmt == 8 and rec.calls == []


def test_mxfp6_quantises_the_activations_itself_and_has_no_fused_layernorm(case):
    m, rec, n_weights, ln_mode, x, w, b = case
    m.enable_mxfp8_linears()
    m.to(torch.float64)
    m.enable_mxfp8_linears(False)
    assert not m._fp8 and not m._fp8_pending
    rec.calls.clear()
    m.enable_mxfp6_linears()
    assert m._mx_fmt == 6 and rec.names() == ["quantize_mxfp6"] * n_weights and len(m._fp8) == n_weights
    wq = m._fp8[(0, "qkv")]
    rec.calls.clear()
    m._lin(0, "qkv", x, w, b, xq=(object(), object()))
    assert rec.names() == ["quantize_mxfp6", "gemm_mxfp6"] and rec.calls[0][1][0] is x
    assert rec.calls[1][1][:4] == (("q6", 1), ("s6", 1), wq[0], wq[1])
    rec.calls.clear()
    assert m._ln_q(0, "qkv", ln_mode, x, eps=1e-6) is None and rec.calls == []


def test_layernorm_emits_mxfp8_unless_the_environment_says_two_passes(case, monkeypatch):
    m, rec, _, ln_mode, x, *_ = case
    monkeypatch.delenv("FINO_NO_LN_MXFP8", raising=False)
    assert m._ln_q(0, "qkv", ln_mode, x, eps=1e-6) is None and rec.calls == []          # off: not on the MXFP8 path
    m.enable_mxfp8_linears()
    rec.calls.clear()
    assert m._ln_q(0, "qkv", ln_mode, x, eps=1e-6) == (("q8", 1), ("s8", 1))
    name, args, kw = rec.calls[0]
    assert name == "ln_mxfp8" and args[0] == ln_mode and args[1] is x and kw == {"eps": 1e-6}
    assert m._ln_q(0, "no such linear", ln_mode, x, eps=1e-6) is None
    rec.calls.clear()
    monkeypatch.setenv("FINO_NO_LN_MXFP8", "1")
    assert m._ln_q(0, "qkv", ln_mode, x, eps=1e-6) is None and rec.calls == []


@pytest.mark.parametrize("fmt", [8, 6])
def test_wan_token_shard_blocks_are_quantised_on_first_use(fmt):
    m = _tiny()
    m.ops = rec = _Recorder()
    x, w, b = torch.zeros(3, 8), torch.zeros(5, 8), torch.zeros(5)
    m._lin(0, "kv", x, w, b)
    assert rec.names() == ["gemm"] and not m._fp8                     # MX off: the model-dtype GEMM, nothing stored
    (m.enable_mxfp6_linears if fmt == 6 else m.enable_mxfp8_linears)()
    rec.calls.clear()
    m._lin(0, "kv", x, w, b)
    assert rec.names() == [f"quantize_mxfp{fmt}"] * 2 + [f"gemm_mxfp{fmt}"]             # the weight block, then x
    assert rec.calls[0][1][0].shape == w.shape and (0, "kv") in m._fp8
    stored = m._fp8[(0, "kv")]
    rec.calls.clear()
    m._lin(0, "kv", x, w, b)
    assert rec.names() == [f"quantize_mxfp{fmt}", f"gemm_mxfp{fmt}"] and rec.calls[0][1][0] is x
    assert m._fp8[(0, "kv")] is stored and rec.calls[1][1][2] is stored[0]
