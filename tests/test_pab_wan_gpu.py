"""Pyramid Attention Broadcast on the Wan DiT (tiny random model, 3 blocks: the model and inputs of
tests/test_step_cache_wan_gpu.py) against the cache-disabled forward, against itself (a re-use step on an unchanged input must
give the computing step's bits) and against the restatement in tests/pab_ref.py (the oracle's pieces in bf16).  Tolerance of a
forward against the bf16 oracle: the one tests/test_wan_model_gpu.py states, rel-RMS <= 1.5e-2.  The decisions are a function
of the step counter and the timestep the callback returns, so the logs of model and restatement must be equal entry by entry."""
import pytest
import torch

from frameino_amd.attention_processor import MI355WanAttnProcessor
from frameino_amd.step_cache import PyramidAttentionBroadcastConfig
from tests.parity import bf16_state_dict, hip_wan_model, rel_rms
from tests.pab_ref import PyramidAttentionBroadcastRef
from tests.test_step_cache_wan_gpu import CFG, DEV, TS

pytestmark = pytest.mark.gpu
BOUND = 1.5e-2
KINDS = {"self": dict(spatial=2), "cross": dict(cross=2), "both": dict(spatial=2, cross=2)}


@pytest.fixture(scope="module")
def setup():
    from oracle import wan_dit as W
    sd = W.wan_random_state_dict(CFG, seed=11, dtype=torch.float32, std=0.04)
    g = torch.Generator().manual_seed(12)
    x = torch.randn(1, 16, 5, 16, 20, generator=g)
    dx = torch.randn(1, 16, 5, 16, 20, generator=g)
    txt = torch.randn(1, 77, 256, generator=g)
    return sd, bf16_state_dict(sd), x, dx, txt


def _model(sd, clock=None, spatial=None, cross=None, dtype=torch.bfloat16, **ranges):
    m = hip_wan_model(CFG, sd, DEV, dtype=dtype)
    if clock is not None:
        m.enable_cache(PyramidAttentionBroadcastConfig(spatial_attention_block_skip_range=spatial,
                                                       cross_attention_block_skip_range=cross,
                                                       current_timestep_callback=lambda: clock["t"], **ranges))
    return m


def _fwd(m, ctx, x, txt, ts=TS, dtype=torch.bfloat16, **kw):
    with m.cache_context(ctx):
        return m(x.to(DEV, dtype), ts.to(DEV), txt.to(DEV, dtype), return_dict=False, **kw)[0]


def _padded(txt, total=256, real=40):
    """a prompt zero-padded as the pipeline pads it: the model folds the padding into one key and runs the text branch's
    out-projection as P.(V W_o^T), the other closing GEMM that keeps y"""
    out = torch.zeros(txt.shape[0], total, txt.shape[2])
    out[:, :real] = txt[:, :real]
    return out


# ------------------------------------------------------------------ 1. outside the range: the uncached model, bit for bit
@pytest.mark.parametrize("padded", [False, True], ids=["prompt", "padded_prompt"])
def test_outside_the_timestep_range_equals_the_uncached_forward(setup, padded):
    sd, _, x, dx, txt = setup
    txt = _padded(txt) if padded else txt
    clock = {"t": 999}
    plain, cached = _model(sd), _model(sd, clock, spatial=2, cross=2)
    for i, t in enumerate((999.0, 900.0, 800.0, 100.0, 50.0)):          # (800 and 100: the bounds are strict)
        clock["t"] = t
        xi, ts = x + 0.1 * i * dx, torch.tensor([t])
        assert torch.equal(_fwd(cached, "c", xi, txt, ts), _fwd(plain, "c", xi, txt, ts)), t
    assert [e[1:] for e in cached.cache_log] == [(i, t, True, True) for i, t in enumerate((999.0, 900.0, 800.0, 100.0, 50.0))]
    if padded:
        assert cached._text_cache["c"][2].w2 is not None                # (the re-associated text out-projection did run)


# ------------------------------------------------------------------ 2. an unchanged input: a re-use step gives the same bits
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("kinds", list(KINDS), ids=list(KINDS))
def test_a_reuse_step_on_the_same_input_is_bit_identical(setup, kinds, dtype):
    sd, _, x, dx, txt = setup
    want = (kinds != "cross", kinds != "self")                          # which kinds are hooked, so re-use
    for text in (txt, _padded(txt)):
        clock = {"t": 500}
        m = _model(sd, clock, dtype=dtype, **KINDS[kinds])
        first = _fwd(m, "c", x, text, dtype=dtype).clone()                # iteration 0: computes
        again = _fwd(m, "c", x, text, dtype=dtype)                        # iteration 1, in range, 1 % 2 != 0: re-uses
        assert torch.equal(again, first)
        assert [(e[3], e[4]) for e in m.cache_log] == [(True, True), (not want[0], not want[1])]
    # ... and with N = 3 at iterations 1 and 2, behind a forward on another input: iteration 1 is out of range and computes on
    # x, iteration 2 (2 % 3 != 0, in range) re-uses what iteration 1 left
    n3 = {k: 3 for k in KINDS[kinds]}
    clock = {"t": 500}
    m = _model(sd, clock, dtype=dtype, **n3)
    _fwd(m, "c", x + dx, txt, dtype=dtype)
    clock["t"] = 900
    first = _fwd(m, "c", x, txt, dtype=dtype).clone()
    clock["t"] = 500
    assert torch.equal(_fwd(m, "c", x, txt, dtype=dtype), first)
    assert [(e[3], e[4]) for e in m.cache_log][1:] == [(True, True), (not want[0], not want[1])]


# ------------------------------------------------------------------ 3. a changed input: the restatement
def _stale_inputs(sdb, x, dx, txt, make_ref, **kw):
    """s such that the restatement's re-use output on x + s dx (attention outputs of x) and its own fresh output there differ by
    at least 5 x the bound: a model that silently recomputes cannot be within the bound of the re-use output"""
    for s in (1.0, 2.0, 0.5, 4.0):
        x2 = x + s * dx
        ref = make_ref()
        ref("c", x.bfloat16(), TS, txt.bfloat16())
        reused = ref("c", x2.bfloat16(), TS, txt.bfloat16())
        fresh = make_ref()("c", x2.bfloat16(), TS, txt.bfloat16())
        gap = rel_rms(reused, fresh)
        if gap >= 5 * BOUND:
            return x2, gap
    raise AssertionError(f"no s separates re-use from recomputation: last gap {gap}")


@pytest.mark.parametrize("kinds", ["cross", "both"])
def test_a_reuse_step_on_a_changed_input_matches_the_restatement(setup, kinds):
    """(the restatement's gap between re-use and recomputation at s = 1: 0.107 with the text branch re-used, 0.114 with both;
    with the self-attention alone it stays below 0.05 for every s, so that case cannot carry the condition and is left to the
    tests above and to the processor count below)"""
    sd, sdb, x, dx, txt = setup
    clock = {"t": 500}
    make_ref = lambda: PyramidAttentionBroadcastRef(sdb, CFG, lambda: clock["t"], **KINDS[kinds])       # noqa: E731
    x2, gap = _stale_inputs(sdb, x, dx, txt, make_ref)
    assert gap >= 5 * BOUND                                              # (on the restatement alone)
    m, ref = _model(sd, clock, **KINDS[kinds]), make_ref()
    for i, v in enumerate((x, x2, x2)):                                  # compute, re-use, compute (2 % 2 == 0)
        out, want = _fwd(m, "c", v, txt), ref("c", v.bfloat16(), TS, txt.bfloat16())
        err = rel_rms(out, want)
        print(f"{kinds}: forward {i}: rel-RMS {err:.3e} against the restatement (re-use / recompute gap {gap:.3e})")
        assert err < BOUND
    assert m.cache_log == ref.log and [e[4] for e in m.cache_log] == [True, False, True]


# ------------------------------------------------------------------ 4. contexts
def test_contexts_are_independent_and_a_context_is_required(setup):
    sd, _, x, dx, txt = setup
    clock = {"t": 500}
    m = _model(sd, clock, spatial=2)
    a = _fwd(m, "cond", x, txt).clone()
    b = _fwd(m, "uncond", x + dx, txt).clone()                          # its own state: iteration 0, computes
    assert torch.equal(_fwd(m, "cond", x, txt), a)                       # re-uses cond's own cache, not uncond's
    assert torch.equal(_fwd(m, "uncond", x + dx, txt), b)
    assert [(e[0], e[1], e[3]) for e in m.cache_log] == [("cond", 0, True), ("uncond", 0, True), ("cond", 1, False),
                                                          ("uncond", 1, False)]
    with pytest.raises(ValueError, match="No context is set"):
        m(x.to(DEV).bfloat16(), TS.to(DEV), txt.to(DEV).bfloat16(), return_dict=False)
    m.disable_cache()
    m(x.to(DEV).bfloat16(), TS.to(DEV), txt.to(DEV).bfloat16(), return_dict=False)     # no cache: no context needed


# ------------------------------------------------------------------ 5. a CFG batch with one context per element
@pytest.mark.parametrize("padded", [True, False], ids=["padded_prompt", "prompt"])
@pytest.mark.parametrize("ahead", [0, 1], ids=["lockstep", "uncond_one_ahead"])
def test_a_batch_with_contexts_equals_sequential_calls(setup, ahead, padded):
    """batch 2 with _cache_contexts=("cond", "uncond") == the two calls one after the other, bit for bit, logs included; with
    "uncond" one forward ahead the two elements of a batched call decide differently"""
    sd, _, x, dx, txt = setup
    # (a padded prompt takes the folded, re-associated text branch; a plain one the ordinary attention + out-projection)
    t2 = torch.cat([_padded(txt), _padded(txt.flip(1))]) if padded else torch.cat([txt, txt.flip(1)])
    clock = {"t": 500}
    seq, bat = _model(sd, clock, spatial=2, cross=3), _model(sd, clock, spatial=2, cross=3)
    for m in (seq, bat):
        for _ in range(ahead):
            _fwd(m, "uncond", x - dx, t2[1:])
    for i in range(4):
        xi = x + 0.3 * i * dx
        want = torch.cat([_fwd(seq, "cond", xi, t2[:1]), _fwd(seq, "uncond", xi, t2[1:])])
        got = _fwd(bat, "cfg", xi.expand(2, -1, -1, -1, -1), t2, _cache_contexts=("cond", "uncond"))
        assert torch.equal(got, want), i
    assert bat.cache_log == seq.cache_log
    decided = [(e[3], e[4]) for e in bat.cache_log[ahead:]]
    assert (decided[0::2] != decided[1::2]) == bool(ahead)


def test_a_batch_under_one_context_decides_jointly(setup):
    """batch 2 under one `cache_context`, no `_cache_contexts`: one counter and one decision for the whole batch, as diffusers'
    hook makes it, and every element gets its branches -- each element's output is bit for bit what it gives alone"""
    sd, _, x, dx, txt = setup
    clock = {"t": 500}
    t2 = torch.cat([txt, txt.flip(1)])
    joint, alone = _model(sd, clock, spatial=2, cross=3), _model(sd, clock, spatial=2, cross=3)
    for i in range(4):
        xs = torch.cat([x + 0.3 * i * dx, x - 0.2 * i * dx])
        got = _fwd(joint, "c", xs, t2)
        want = torch.cat([_fwd(alone, f"e{k}", xs[k:k + 1], t2[k:k + 1]) for k in range(2)])
        assert torch.equal(got, want), i
    assert [(e[0], e[1], e[3], e[4]) for e in joint.cache_log] == [("c", 0, True, True), ("c", 1, False, False),
                                                                    ("c", 2, True, False), ("c", 3, False, True)]
    assert joint._step_cache_states["c"].buffers["self", 0].shape[0] == 2 * 400


def test_a_reuse_step_launches_no_attention_on_the_default_path(setup, monkeypatch):
    """the built-in processors: across a re-use step of both kinds no attention, GEMM of the branches or norm + RoPE launch is
    made (the log is written before any launch, so it cannot show this), and a self-only re-use keeps the text branch"""
    from frameino_amd import ops
    sd, _, x, dx, txt = setup
    counts = {}

    def spy(name):
        real = getattr(ops, name)

        def f(*a, **k):
            counts[name] = counts.get(name, 0) + 1
            return real(*a, **k)
        monkeypatch.setattr(ops, name, f)
    for name in ("attention", "attention_tail", "attention_probs", "gemm", "qkv_rmsnorm_rope_", "pab_broadcast"):
        spy(name)
    layers = CFG["num_layers"]
    for kinds, attn_launches in (("both", 0), ("self", layers)):
        clock = {"t": 500}
        m = _model(sd, clock, **KINDS[kinds])
        _fwd(m, "c", x, txt)
        counts.clear()
        _fwd(m, "c", x + dx, txt)                                        # iteration 1: re-uses
        assert counts.get("attention", 0) + counts.get("attention_tail", 0) + counts.get("attention_probs", 0) == attn_launches
        assert counts.get("qkv_rmsnorm_rope_", 0) == 0
        assert counts["pab_broadcast"] == layers * len(KINDS[kinds])
        gemms_reuse = counts["gemm"]
        counts.clear()
        _fwd(m, "c", x - dx, txt)                                        # iteration 2: computes again
        assert counts.get("attention", 0) == 2 * layers and counts.get("pab_broadcast", 0) == 0
        assert counts["qkv_rmsnorm_rope_"] == layers
        # the GEMMs the re-use step left out: QKV + out-projection (and to_q + out-projection of the text branch) per block
        assert counts["gemm"] - gemms_reuse == 2 * layers * len(KINDS[kinds])


# ------------------------------------------------------------------ 6. live rows, a custom processor
def test_live_rows_read_as_the_restatement(setup):
    sd, sdb, x, dx, txt = setup
    clock = {"t": 500}
    m = _model(sd, clock, spatial=2, cross=2)
    ref = PyramidAttentionBroadcastRef(sdb, CFG, lambda: clock["t"], spatial=2, cross=2)
    rows_per_frame = (16 // 2) * (20 // 2)
    for i, v in enumerate((x, x + dx, x - dx)):
        out = _fwd(m, "c", v, txt, live_rows=(rows_per_frame, 5 * rows_per_frame))       # the caller drops frame 0
        want = ref("c", v.bfloat16(), TS, txt.bfloat16())
        assert rel_rms(out[:, :, 1:], want[:, :, 1:]) < BOUND, i
    assert m.cache_log == ref.log and [e[3] for e in m.cache_log] == [True, False, True]


def test_a_custom_processor_is_cached_by_its_return_value(setup):
    """a user-installed processor (a subclass of the built-in one: the model then goes through the plugin protocol) computes the
    oracle's attention, so the bound of a forward against the bf16 oracle applies; its return value is what is cached, and a
    re-use step calls no processor"""
    sd, sdb, x, dx, txt = setup
    calls = []

    class Spy(MI355WanAttnProcessor):
        def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, rotary_emb=None):
            calls.append(encoder_hidden_states is None)
            return super().__call__(attn, hidden_states, encoder_hidden_states, attention_mask, rotary_emb)

    clock = {"t": 500}
    m = _model(sd, clock, spatial=2, cross=2)
    for b in m.blocks:
        b.attn1.set_processor(Spy())
        b.attn2.set_processor(Spy())
    ref = PyramidAttentionBroadcastRef(sdb, CFG, lambda: clock["t"], spatial=2, cross=2)
    seen = []
    for i, v in enumerate((x, x + dx, x - dx)):
        out = _fwd(m, "c", v, txt)
        seen.append(len(calls))
        err = rel_rms(out, ref("c", v.bfloat16(), TS, txt.bfloat16()))
        print(f"custom processor: forward {i}: rel-RMS {err:.3e} against the restatement")
        assert err < BOUND, i
    assert seen == [6, 6, 12]                                            # the re-use step called no processor
    assert m.cache_log == ref.log and [(e[3], e[4]) for e in m.cache_log] == [(True, True), (False, False), (True, True)]


def test_mx_linears_and_fp8_attention_compose(setup):
    """the cache holds whatever the enabled path produced: a re-use step on the same input repeats the computing step's bits"""
    sd, _, x, _, txt = setup
    for switch in ("enable_mxfp8_linears", "enable_mxfp6_linears", "enable_fp8_attention"):
        clock = {"t": 500}
        m = _model(sd, clock, spatial=2, cross=2)
        getattr(m, switch)()
        first = _fwd(m, "c", x, txt).clone()
        assert torch.equal(_fwd(m, "c", x, txt), first), switch
        assert [(e[3], e[4]) for e in m.cache_log] == [(True, True), (False, False)]
