"""Pyramid Attention Broadcast on the CogVideoX DiT (CogVideoXTransformer3DModel.enable_cache) against the cache-disabled forward,
against itself (a re-using forward on an unchanged input must give the computing forward's bits) and against the restatement in
tests/cog_pab_ref.py (oracle.cog_dit's pieces in bf16, the attention branch output carried over between forwards).  The tiny DiT of
tests/cog_window_attn_ref.py: 2 layers, 2 heads x 64, 8 text rows, 9 latent frames of 150 tokens, L = 1358 (a ragged last q-block
and key tile), batch 2 under one cache context as the pipelines' CFG batch runs.  Tolerances: the dense tiny forward's bound
against the bf16 oracle (tests/test_cog_model_gpu.py: 3e-2); with fp8 attention the bound the tiny-model fp8 attention test holds
the dense model to (6e-2); with MX linears the bounds tests/test_mxfp8_gpu.py and tests/test_mxfp6_gpu.py hold the dense tiny model
to against its own model-dtype forward (MXFP8 0.12, MXFP6 1.5 x the MXFP8 error)."""
import pytest
import torch

from frameino_amd.step_cache import PyramidAttentionBroadcastConfig
from frameino_amd.window_attention import WindowAttentionConfig
from tests import cog_window_attn_ref as R
from tests.cog_pab_ref import CogPyramidAttentionBroadcastRef
from tests.parity import record, rel_rms

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOUND = 3e-2
FP8_BOUND = 6e-2
MXFP8_BOUND = 0.12
CFG, FRAMES, TPF, TEXT, L, SINKS = R.TINY_CFG, R.FRAMES, R.TPF, R.TEXT, R.L, R.SINKS
LAYERS, D = CFG["num_layers"], CFG["num_attention_heads"] * CFG["attention_head_dim"]
CTX = "cond_uncond"
T0, T1 = 500.0, 450.0                      # both strictly inside (100, 800)


def _ref(sdb, clock, **kw):
    return CogPyramidAttentionBroadcastRef(sdb, CFG, lambda: clock["t"], **kw)


def _ref_fwd(ref, inp, ctx=CTX):
    x, txt, ts, rot = inp
    return ref(ctx, x.bfloat16(), txt.bfloat16(), ts, rot).float()


@pytest.fixture(scope="module")
def setup():
    """two inputs (other latents, another timestep) on which the restatement's RE-USING output on the second -- attention
    branches of the first -- and its recomputed output there differ by at least 5 x BOUND (on the CPU, the restatement alone):
    otherwise no assertion below could tell re-use from recomputation.  The weights are scaled until they do."""
    x, txt, ts, rot = R.tiny_inputs(batch=2)
    x2 = R.tiny_inputs(seed=13, batch=2)[0]
    a, b = (x, txt, torch.full((2,), T0), rot), (x2, txt, torch.full((2,), T1), rot)
    for v_scale, gate in ((4.0, 0.5), (8.0, 1.0), (16.0, 1.0)):
        sd = R.tiny_state_dict(11, 0.05, v_scale, gate)
        sdb = {k: v.bfloat16() for k, v in sd.items()}
        clock = {"t": T0}
        ref = _ref(sdb, clock)
        first = _ref_fwd(ref, a)
        clock["t"] = T1
        reused = _ref_fwd(ref, b)
        fresh = _ref_fwd(_ref(sdb, clock), b)
        assert [e[3] for e in ref.log] == [True, False]
        gap = rel_rms(reused, fresh)
        print(f"restatement: re-using vs recomputing rel-RMS {gap:.3e} at value scale {v_scale}, gate {gate} (needs >= {5 * BOUND:.3e})")
        if gap >= 5 * BOUND:
            return sd, sdb, a, b, first, reused, fresh, gap
    raise AssertionError(f"no scale separates re-use from recomputation: last gap {gap}")


def _model(sd, clock=None, spatial=2, dtype=torch.bfloat16, **ranges):
    from frameino_amd.cogvideox_transformer_3d import CogVideoXTransformer3DModel
    m = CogVideoXTransformer3DModel(**CFG).to(DEV)
    m.load_reference_state_dict(sd, dtype=dtype)
    m = m.eval()
    if clock is not None:
        m.enable_cache(PyramidAttentionBroadcastConfig(spatial_attention_block_skip_range=spatial,
                                                       current_timestep_callback=lambda: clock["t"], **ranges))
    return m


def _fwd(m, inp, ctx=CTX, dtype=torch.bfloat16, **kw):
    x, txt, ts, rot = inp
    with m.cache_context(ctx):
        return m(hidden_states=x.to(DEV, dtype), encoder_hidden_states=txt.to(DEV, dtype), timestep=ts.to(DEV),
                 image_rotary_emb=(rot[0].to(DEV), rot[1].to(DEV)), return_dict=False, **kw)[0]


# ------------------------------------------------------------------ (i) outside the range: the uncached model
def test_outside_the_timestep_range_equals_the_uncached_forward(setup):
    sd, a, b = setup[0], setup[2], setup[3]
    clock = {"t": 999.0}
    default, plain, cached = _model(sd), _model(sd), _model(sd, clock)
    plain.skip_dead_rows = False                                            # every block runs all L rows, as under the cache
    assert default.skip_dead_rows
    times = (999.0, 900.0, 800.0, 100.0, 50.0)                              # (800 and 100: the bounds are strict)
    for i, t in enumerate(times):
        clock["t"] = t
        x, txt, _, rot = b if i % 2 else a
        inp = (x, txt, torch.full((2,), t), rot)
        live = {"live_frames": FRAMES - 1} if i >= 3 else {}
        out = _fwd(cached, inp, **live)
        k = FRAMES - 1 if live else FRAMES                                  # (under live_frames the other frames come back zero)
        assert torch.equal(out[:, :k], _fwd(plain, inp, **live)[:, :k]), t
        want = _fwd(default, inp, **live)
        err = rel_rms(out, want)
        print(f"t = {t}: cached vs the default uncached model (skip_dead_rows on) rel-RMS {err:.3e}")
        assert err < BOUND, t
        if live:                                                            # the returned rows and the zeros stay as they are
            assert float(out[:, FRAMES - 1].abs().max()) == 0.0 and float(want[:, FRAMES - 1].abs().max()) == 0.0
    assert cached.cache_log == [(CTX, i, t, True, True) for i, t in enumerate(times)]


# ------------------------------------------------------------------ (ii) an unchanged input: a re-use gives the same bits
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_a_reuse_forward_on_the_same_input_is_bit_identical(setup, dtype):
    sd, a, b = setup[0], setup[2], setup[3]
    clock = {"t": T0}
    m = _model(sd, clock, dtype=dtype)
    first = _fwd(m, a, dtype=dtype).clone()                                  # iteration 0: computes
    again = _fwd(m, a, dtype=dtype)                                          # iteration 1, in range, 1 % 2 != 0: re-uses
    assert torch.isfinite(first.float()).all() and torch.equal(again, first)
    assert [e[3] for e in m.cache_log] == [True, False]
    buf = m._step_cache_states[CTX].buffers
    assert sorted(buf) == [("self", li) for li in range(LAYERS)]
    assert all(tuple(v.shape) == (2 * L, D) and v.dtype == dtype for v in buf.values())
    # ... and with N = 3 at iterations 1 and 2, behind a forward on another input: iteration 1 is out of range and computes on
    # `a`, iteration 2 (2 % 3 != 0, in range) re-uses what iteration 1 left
    clock = {"t": T0}
    m = _model(sd, clock, spatial=3, dtype=dtype)
    _fwd(m, b, dtype=dtype)
    clock["t"] = 900.0
    first = _fwd(m, a, dtype=dtype).clone()
    clock["t"] = T0
    assert torch.equal(_fwd(m, a, dtype=dtype), first)
    assert [e[3] for e in m.cache_log] == [True, True, False]


# ------------------------------------------------------------------ (iii) a changed input: the restatement
def test_a_reuse_forward_on_a_changed_input_matches_the_restatement(setup):
    sd, sdb, a, b, first, reused, fresh, gap = setup
    assert gap >= 5 * BOUND                                                  # (on the restatement alone)
    clock = {"t": T0}
    m, ref = _model(sd, clock), _ref(sdb, clock)
    for i, (inp, t) in enumerate(((a, T0), (b, T1), (b, T1))):               # compute, re-use, compute (2 % 2 == 0)
        clock["t"] = t
        out, want = _fwd(m, inp), _ref_fwd(ref, inp)
        err = rel_rms(out, want)
        print(f"forward {i}: rel-RMS {err:.3e} against the restatement (re-use / recompute gap {gap:.3e})")
        record(f"cog_pab[tiny, bf16, forward {i}]", "rel_rms vs the restatement", err, BOUND)
        assert err < BOUND, i
        if i == 1:
            assert torch.equal(want, reused) and rel_rms(out, fresh) > 3 * BOUND      # (and so it did not recompute)
    assert m.cache_log == ref.log and [e[3] for e in m.cache_log] == [True, False, True]


# ------------------------------------------------------------------ (iv) what a re-use forward launches
def _spy(monkeypatch, names):
    from frameino_amd import ops
    counts = {}

    def wrap(name):
        real = getattr(ops, name)

        def f(*a_, **k_):
            counts[name] = counts.get(name, 0) + 1
            return real(*a_, **k_)
        monkeypatch.setattr(ops, name, f)
    for name in names:
        wrap(name)
    return counts


def test_a_reuse_forward_launches_no_norm1_qkv_head_norm_or_attention(setup, monkeypatch):
    """(the log is written before any launch, so it cannot show this)"""
    sd, a, b = setup[0], setup[2], setup[3]
    counts = _spy(monkeypatch, ("layernorm_zero", "gemm", "headnorm_rope_", "attention", "attention_ranges", "attention_fp8",
                                "gated_residual", "pab_broadcast"))
    clock = {"t": T0}
    m = _model(sd, clock)
    _fwd(m, a)
    # a computing forward: per block norm1 + norm2, QKV + out + FFN up + down, 2 head norms, 1 attention; per element the text and
    # patch embeddings, the positional add, the final AdaLayerNorm and the output head
    assert (counts["layernorm_zero"], counts["gemm"], counts["headnorm_rope_"], counts["attention"], counts["gated_residual"]) \
        == (2 * LAYERS + 2, 2 * 2 + 4 * LAYERS + 2, 2 * LAYERS, LAYERS, 2)
    counts.clear()
    _fwd(m, b)                                                               # iteration 1: re-uses
    assert counts.get("attention", 0) + counts.get("attention_ranges", 0) + counts.get("attention_fp8", 0) == 0
    assert counts.get("headnorm_rope_", 0) == 0 and counts.get("pab_broadcast", 0) == 0
    assert counts["layernorm_zero"] == LAYERS + 2                            # norm2 of every block; no norm1
    assert counts["gemm"] == 2 * 2 + 2 * LAYERS + 2                          # FFN up + down; no QKV, no out-projection
    assert counts["gated_residual"] == 2 + LAYERS                            # the cached y, once per block
    counts.clear()
    _fwd(m, b)                                                               # iteration 2: computes again
    assert (counts["attention"], counts["headnorm_rope_"], counts["gemm"]) == (LAYERS, 2 * LAYERS, 2 * 2 + 4 * LAYERS + 2)


@pytest.mark.parametrize("fmt", [8, 6])
def test_an_mx_out_projection_keeps_y_in_one_launch(setup, monkeypatch, fmt):
    sd, a, b = setup[0], setup[2], setup[3]
    gemm = f"gemm_mxfp{fmt}"
    counts = _spy(monkeypatch, (gemm, "gemm_mxfp8_q", "pab_broadcast", "gated_residual", "ln_mxfp8", "layernorm_zero",
                                f"quantize_mxfp{fmt}", "attention"))
    clock = {"t": T0}
    m = _model(sd, clock)
    getattr(m, f"enable_mxfp{fmt}_linears")()
    counts.clear()
    _fwd(m, a)
    # computing: QKV, out (with keep=) and FFN down per block (+ FFN up on MXFP6; MXFP8 runs it as gemm_mxfp8_q) -- and no
    # separate residual pass behind the out-projection
    assert counts[gemm] == (3 if fmt == 8 else 4) * LAYERS and counts.get("pab_broadcast", 0) == 0
    assert counts["gated_residual"] == 2 and counts["attention"] == LAYERS
    counts.clear()
    _fwd(m, b)                                                               # re-using: the FFN alone
    assert counts[gemm] == (1 if fmt == 8 else 2) * LAYERS and counts.get("attention", 0) == 0
    assert counts["gated_residual"] == 2 + LAYERS
    if fmt == 8:
        assert counts["ln_mxfp8"] == LAYERS and counts["gemm_mxfp8_q"] == LAYERS and counts["layernorm_zero"] == 2
    else:
        assert counts["quantize_mxfp6"] == 2 * LAYERS and counts["layernorm_zero"] == LAYERS + 2


# ------------------------------------------------------------------ (v) contexts
def test_contexts_are_independent_and_a_context_is_required(setup):
    sd, a, b = setup[0], setup[2], setup[3]
    clock = {"t": T0}
    m = _model(sd, clock)
    oa = _fwd(m, a, "one").clone()
    ob = _fwd(m, b, "two").clone()                                           # its own state: iteration 0, computes
    assert torch.equal(_fwd(m, a, "one"), oa)                                # re-uses its own cache, not the other's
    assert torch.equal(_fwd(m, b, "two"), ob)
    assert [(e[0], e[1], e[3]) for e in m.cache_log] == [("one", 0, True), ("two", 0, True), ("one", 1, False), ("two", 1, False)]
    x, txt, ts, rot = a
    args = dict(hidden_states=x.to(DEV, torch.bfloat16), encoder_hidden_states=txt.to(DEV, torch.bfloat16), timestep=ts.to(DEV),
                image_rotary_emb=(rot[0].to(DEV), rot[1].to(DEV)), return_dict=False)
    with pytest.raises(ValueError, match="No context is set"):
        m(**args)
    m.disable_cache()
    m(**args)                                                                # no cache: no context needed


# ------------------------------------------------------------------ (vi) combinations
def test_mx_linears_compose(setup):
    """computing and re-using forwards with MXFP8 / MXFP6 linears against the same forwards of the model-dtype cached model, at
    the bounds the dense tiny model is held to; a re-use on an unchanged input repeats the computing forward's bits"""
    sd, a, b = setup[0], setup[2], setup[3]
    clock = {"t": T0}
    outs = {}
    for fmt in (0, 8, 6):
        m = _model(sd, clock)
        if fmt:
            getattr(m, f"enable_mxfp{fmt}_linears")()
        outs[fmt] = [_fwd(m, a).clone(), _fwd(m, b).clone()]                 # compute, re-use on a changed input
        assert [e[3] for e in m.cache_log] == [True, False]
        if fmt:
            m._reset_stateful_cache()
            first = _fwd(m, a).clone()
            assert torch.equal(first, outs[fmt][0]) and torch.equal(_fwd(m, a), first), fmt
    for i, what in enumerate(("computing", "re-using")):
        e8, e6 = rel_rms(outs[8][i], outs[0][i].float()), rel_rms(outs[6][i], outs[0][i].float())
        print(f"{what} forward: mxfp8-linears vs the model-dtype cached model rel-RMS {e8:.4f}, mxfp6-linears {e6:.4f}")
        record(f"cog_pab[tiny, mxfp8, {what}]", "rel_rms vs own bf16", e8, MXFP8_BOUND)
        record(f"cog_pab[tiny, mxfp6, {what}]", "rel_rms vs own bf16", e6, 1.5 * e8)
        assert 1e-4 < e8 < MXFP8_BOUND and 1e-4 < e6 <= 1.5 * e8, what
        assert not torch.equal(outs[8][i], outs[6][i])


@pytest.mark.parametrize("fp8", [dict(), dict(smooth_k=True), dict(p_mode="exp2")], ids=["ramp", "ramp-smooth-k", "exp2"])
def test_fp8_attention_composes(setup, fp8):
    sd, sdb, a, b = setup[:4]
    clock = {"t": T0}
    m, ref = _model(sd, clock), _ref(sdb, clock)
    m.enable_fp8_attention(**fp8)
    for i, (inp, t) in enumerate(((a, T0), (b, T1))):                        # compute, re-use
        clock["t"] = t
        out = _fwd(m, inp)
        err = rel_rms(out, _ref_fwd(ref, inp))
        print(f"fp8 attention {fp8}, forward {i}: rel-RMS {err:.3e} against the restatement")
        record(f"cog_pab[tiny, fp8 attention {fp8}, forward {i}]", "rel_rms vs the restatement", err, FP8_BOUND)
        assert torch.isfinite(out.float()).all() and err < FP8_BOUND, i
    assert m.cache_log == ref.log and [e[3] for e in m.cache_log] == [True, False]


def test_window_attention_composes(setup):
    """a re-using forward under an enabled window: the restatement with the WINDOWED branch carried over (under the cache every
    block runs all L rows: one table, q-blocks from row 0); nothing of the table is read, the window's log still grows"""
    sd, sdb, a, b = setup[:4]
    masks = R.layer_masks(LAYERS, FRAMES, TPF, TEXT, 1, SINKS)
    clock = {"t": T0}
    m, ref, dense = _model(sd, clock), _ref(sdb, clock, masks=masks), _ref(sdb, clock)
    m.enable_window_attention(WindowAttentionConfig(window_frames=1, sink_frames=(0,)))
    for i, (inp, t) in enumerate(((a, T0), (b, T1))):
        clock["t"] = t
        out, want, far = _fwd(m, inp, id_frames=1), _ref_fwd(ref, inp), _ref_fwd(dense, inp)
        err = rel_rms(out, want)
        print(f"window + cache, forward {i}: rel-RMS {err:.3e} against the windowed restatement, {rel_rms(out, far):.3e} against "
              f"the dense one (the two restatements: {rel_rms(want, far):.3e})")
        assert err < BOUND and err < rel_rms(out, far), i
        if i == 0:
            tables = {k: v for k, v in m._pos_cache.items() if k[0] == "window"}
            assert len(tables) == 1
    assert {k: v for k, v in m._pos_cache.items() if k[0] == "window"}.keys() == tables.keys()
    assert m.window_attention_log == [(0, None, True), (1, None, True)] and [e[3] for e in m.cache_log] == [True, False]


# ------------------------------------------------------------------ (vii) a custom processor
def test_a_custom_processor_is_cached_by_its_return_value(setup):
    """a user-installed processor (a subclass of the built-in one: the model then goes through the plugin protocol) computes the
    oracle's attention, so the bound of a forward against the restatement applies; `torch.cat([text, video], 1)` of its return
    value is what is cached, and a re-using forward calls no processor"""
    from frameino_amd.attention_processor import MI355CogVideoXAttnProcessor
    sd, sdb, a, b = setup[:4]
    returned = []

    class Spy(MI355CogVideoXAttnProcessor):
        def __call__(self, attn, hidden_states, encoder_hidden_states, attention_mask=None, image_rotary_emb=None):
            out = super().__call__(attn, hidden_states, encoder_hidden_states, attention_mask, image_rotary_emb)
            returned.append(out)
            return out

    clock = {"t": T0}
    m, ref = _model(sd, clock), _ref(sdb, clock)
    for blk in m.transformer_blocks:
        blk.attn1.set_processor(Spy())
    seen = []
    for i, (inp, t) in enumerate(((a, T0), (b, T1), (b, T1))):
        clock["t"] = t
        out = _fwd(m, inp)
        seen.append(len(returned))
        err = rel_rms(out, _ref_fwd(ref, inp))
        print(f"custom processor: forward {i}: rel-RMS {err:.3e} against the restatement")
        assert err < BOUND, i
        if i == 0:
            for li, (ah, ae) in enumerate(returned):
                assert torch.equal(m._step_cache_states[CTX].buffers["self", li], torch.cat([ae, ah], dim=1).reshape(2 * L, D))
    assert seen == [LAYERS, LAYERS, 2 * LAYERS]                              # the re-using forward called no processor
    assert m.cache_log == ref.log and [e[3] for e in m.cache_log] == [True, False, True]
