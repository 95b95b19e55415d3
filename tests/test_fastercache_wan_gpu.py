"""FasterCache on the Wan DiT (the tiny 3-block model and inputs of tests/test_taylorseer_wan_gpu.py): against the cache-disabled
forward (a schedule that never skips must give its bits, and so must the "cond" row of a skipping step), against the two ops
(the "uncond" row of a skipping step is ops.fastercache_apply of the "cond" row with ops.fastercache_delta of the last computing
step's two predictions, bit for bit), against itself (on an unchanged input y_1 - y_0 = 0, so an attention-skipping forward
gives the computing one's bits) and against the restatement in tests/fastercache_ref.py within the bound of a forward against
the bf16 oracle, rel-RMS <= 1.5e-2."""
import pytest
import torch

from frameino_amd import ops
from frameino_amd.step_cache import FasterCacheConfig, fastercache_weights
from tests import fastercache_ref as R
from tests.parity import bf16_state_dict, hip_wan_model, rel_rms
from tests.test_step_cache_wan_gpu import CFG, DEV, TS

pytestmark = pytest.mark.gpu
BOUND = 1.5e-2
ALL = (-1, 1001)
SHAPES = pytest.mark.parametrize("batched", [False, True], ids=["sequential", "batched"])


@pytest.fixture(scope="module")
def setup():
    from oracle import wan_dit as W
    sd = W.wan_random_state_dict(CFG, seed=11, dtype=torch.float32, std=0.04)
    g = torch.Generator().manual_seed(12)
    x = torch.randn(1, 16, 5, 16, 20, generator=g)
    dx = torch.randn(1, 16, 5, 16, 20, generator=g)
    txt = torch.randn(2, 77, 256, generator=g)
    return sd, bf16_state_dict(sd), x, dx, txt


def _config(clock, uncond=2, attention=None, **kw):
    kw.setdefault("unconditional_batch_timestep_skip_range", ALL)
    kw.setdefault("spatial_attention_timestep_skip_range", ALL)
    return FasterCacheConfig(unconditional_batch_skip_range=uncond, spatial_attention_block_skip_range=attention,
                             attention_weight_callback=lambda m: 0.5, current_timestep_callback=lambda: clock["t"], **kw)


def _model(sd, config=None, dtype=torch.bfloat16):
    m = hip_wan_model(CFG, sd, DEV, dtype=dtype)
    if config is not None:
        m.enable_cache(config)
    return m


def _fwd(m, ctx, x, txt, ts=TS, dtype=torch.bfloat16, **kw):
    with m.cache_context(ctx):
        return m(x.to(DEV, dtype), ts.to(DEV), txt.to(DEV, dtype), return_dict=False, **kw)[0]


def _pair(m, x, txt, batched, dtype=torch.bfloat16, cached=True, **kw):
    """(cond, uncond) predictions of one step in either call shape"""
    if batched:
        ctxs = {"_cache_contexts": ("cond", "uncond")} if cached else {}
        both = _fwd(m, "cfg", x.expand(2, -1, -1, -1, -1), txt, dtype=dtype, **ctxs, **kw)
        return both[0], both[1]
    return _fwd(m, "cond", x, txt[:1], dtype=dtype, **kw)[0], _fwd(m, "uncond", x, txt[1:], dtype=dtype, **kw)[0]


# ------------------------------------------------------------------ a schedule that never skips
@SHAPES
def test_a_schedule_that_never_skips_equals_the_uncached_forward(setup, batched):
    sd, _, x, dx, txt = setup
    clock = {"t": 811.0}                                             # outside (-1, 641) and (-1, 681): diffusers' defaults
    cfg = FasterCacheConfig(attention_weight_callback=lambda m: 0.5, current_timestep_callback=lambda: clock["t"])
    plain, cached = _model(sd), _model(sd, cfg)
    for i in range(3):
        xi = x + 0.1 * i * dx
        got, want = _pair(cached, xi, txt, batched), _pair(plain, xi, txt, batched, cached=False)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), i
    assert cached.cache_log == [(c, i, 811.0, True, True) for i in range(3) for c in ("cond", "uncond")]


# ------------------------------------------------------------------ the unconditional branch alone
@SHAPES
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_a_skipping_step_is_the_cond_forward_plus_the_two_ops(setup, batched, dtype):
    sd, _, x, dx, txt = setup
    clock = {"t": 200.0}                                             # inside both weight-update ranges: both weights compound
    cfg = _config(clock, uncond=3)
    plain, m = _model(sd, dtype=dtype), _model(sd, cfg, dtype=dtype)
    c0, u0 = (t.clone() for t in _pair(m, x, txt, batched, dtype))   # i = 0: both run
    p0 = _pair(plain, x, txt, batched, dtype, cached=False)
    assert torch.equal(c0, p0[0]) and torch.equal(u0, p0[1])
    dl, dh = ops.fastercache_delta(u0, c0)
    al = ah = 1.0
    for i in (1, 2):                                                 # 1 % 3, 2 % 3 != 0: "uncond" is rebuilt
        xi = x + 0.2 * i * dx
        c, u = _pair(m, xi, txt, batched, dtype)
        assert torch.equal(c, _fwd(plain, "cond", xi, txt[:1], dtype=dtype)[0]), i
        al, ah = fastercache_weights(200.0, al, ah, cfg, m)
        assert torch.equal(u, ops.fastercache_apply(c, dl, dh, al, ah)), i
    assert (al, ah) == (R.f32(R.f32(1.1) * R.f32(1.1)),) * 2
    c3, u3 = _pair(m, x - dx, txt, batched, dtype)                   # i = 3: both run again, a new delta, weights back to 1
    p3 = _pair(plain, x - dx, txt, batched, dtype, cached=False)
    assert torch.equal(c3, p3[0]) and torch.equal(u3, p3[1])
    st = m._step_cache_states["uncond"]
    assert (st.a_low, st.a_high) == (1.0, 1.0)
    want = ops.fastercache_delta(u3, c3)
    assert torch.equal(st.d_low, want[0]) and torch.equal(st.d_high, want[1])
    assert [e[3] for e in m.cache_log if e[0] == "uncond"] == [True, False, False, True]
    assert all(e[3] for e in m.cache_log if e[0] == "cond")
    assert m._step_cache_states["cond"].out.data_ptr() == c3.data_ptr()          # kept by reference, not copied


def test_the_uncond_call_needs_the_cond_call_of_the_same_step(setup):
    sd, _, x, dx, txt = setup
    clock = {"t": 200.0}
    m = _model(sd, _config(clock))
    _pair(m, x, txt, False)
    with pytest.raises(RuntimeError, match='"cond" context has not run forward 1'):
        _fwd(m, "uncond", x, txt[1:])


def test_launch_counts_and_live_rows(setup, monkeypatch):
    sd, _, x, dx, txt = setup
    counts = {}

    def spy(name):
        real = getattr(ops, name)

        def f(*a, **k):
            counts[name] = counts.get(name, 0) + 1
            return real(*a, **k)
        monkeypatch.setattr(ops, name, f)
    for name in ("attention", "gemm", "qkv_rmsnorm_rope_", "taylor_update", "taylor_predict", "adaln_modulate", "unpatchify",
                 "patchify", "fastercache_delta", "fastercache_apply"):
        spy(name)
    layers = CFG["num_layers"]
    clock = {"t": 200.0}
    plain = _model(sd)
    _fwd(plain, "cond", x, txt[:1])
    counts.clear()
    _fwd(plain, "cond", x, txt[:1])
    one = dict(counts)                                               # the launches of one uncached batch-1 forward
    # the unconditional branch: a skipped "uncond" launches no stack, in either call shape
    m = _model(sd, _config(clock))
    _pair(m, x, txt, False)
    counts.clear()
    _fwd(m, "cond", x + dx, txt[:1])
    assert counts == one
    counts.clear()
    _fwd(m, "uncond", x + dx, txt[1:])
    assert counts == {"fastercache_apply": 1}
    m = _model(sd, _config(clock))
    _pair(m, x, txt, True)
    assert counts["fastercache_delta"] == 1
    counts.clear()
    _pair(m, x + dx, txt, True)                                      # batch 1 through the stack, one apply
    assert counts == dict(one, fastercache_apply=1)
    # the self-attention part: an attention-skipping forward launches no attn1 branch
    m = _model(sd, _config(clock, uncond=None, attention=2))
    _fwd(m, "cond", x, txt[:1])
    counts.clear()
    _fwd(m, "cond", x + dx, txt[:1])                                 # i = 1: skips (one plane: re-use)
    assert counts["attention"] == layers and counts.get("qkv_rmsnorm_rope_", 0) == 0 and counts["taylor_predict"] == layers
    assert counts.get("taylor_update", 0) == 0 and one["gemm"] - counts["gemm"] == 2 * layers
    counts.clear()
    _fwd(m, "cond", x - dx, txt[:1])                                 # i = 2: computes
    assert counts["taylor_update"] == layers and counts.get("taylor_predict", 0) == 0
    assert {k: v for k, v in counts.items() if k != "taylor_update"} == one
    # live_rows is honoured under the unconditional-branch part: dead planes are zero in both rows, live ones unchanged
    rows = (16 // 2) * (20 // 2)
    full, live = _model(sd, _config(clock)), _model(sd, _config(clock))
    for i in range(2):
        xi = x + 0.3 * i * dx
        a, b = _pair(full, xi, txt, True), _pair(live, xi, txt, True, live_rows=(rows, 4 * rows))
        for k in range(2):
            assert torch.equal(a[k][:, 1:4], b[k][:, 1:4]) and not b[k][:, :1].any() and not b[k][:, 4:].any(), (i, k)
    assert [e[3] for e in live.cache_log] == [True, True, True, False]


# ------------------------------------------------------------------ the self-attention part
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_an_attention_skipping_forward_on_the_same_input_is_bit_identical(setup, dtype):
    sd, _, x, _, txt = setup
    clock = {"t": 500.0}
    m = _model(sd, _config(clock, uncond=None, attention=3), dtype=dtype)
    first = _fwd(m, "c", x, txt[:1], dtype=dtype).clone()
    for i in range(1, 5):                                            # i = 3 computes: f_1 = y - y = 0; 4 extrapolates with it
        assert torch.equal(_fwd(m, "c", x, txt[:1], dtype=dtype), first), i
    assert [e[4] for e in m.cache_log] == [True, False, False, True, False]
    bufs = m._step_cache_states["c"].buffers
    assert len(bufs) == CFG["num_layers"] and all(f.shape[0] == 2 and f.dtype == dtype and not f[1].any() for f in bufs.values())


def test_changed_inputs_match_the_restatement(setup):
    sd, sdb, x, dx, txt = setup
    clock = {"t": 500.0}
    cfg = _config(clock, uncond=None, attention=3)
    m, ref = _model(sd, cfg), R.attention_ref(sdb, CFG, cfg)
    # compute, compute, skip (two planes: extrapolates), compute, skip
    for i, s in enumerate((0.0, 1.0, 2.0, 3.0, 4.0)):
        if i == 1:
            clock["t"] = 2000.0                                      # out of range: i = 1 computes, so i = 2 has two planes
        else:
            clock["t"] = 500.0
        v = x + s * dx
        out, want = _fwd(m, "c", v, txt[:1]), ref("c", v.bfloat16(), TS, txt[:1].bfloat16())
        err = rel_rms(out, want)
        print(f"forward {i}: rel-RMS {err:.3e} against the restatement")
        assert err < BOUND, i
    assert m.cache_log == ref.log
    assert [e[4] for e in m.cache_log] == [True, True, False, True, False]


def test_a_stack_that_did_not_run_last_time_computes_its_attention(setup):
    sd, _, x, dx, txt = setup
    clock = {"t": 500.0}
    m = _model(sd, _config(clock, uncond=2, attention=3))
    for i in range(5):
        _pair(m, x + 0.1 * i * dx, txt, True)
    log = {c: [e[3:] for e in m.cache_log if e[0] == c] for c in ("cond", "uncond")}
    assert log["cond"] == [(True, True), (True, False), (True, False), (True, True), (True, False)]
    # "uncond" runs at 0, 2, 4: its stack never ran at i - 1, so every one of them computes its attention
    assert log["uncond"] == [(True, True), (False, False), (True, True), (False, False), (True, True)]


# ------------------------------------------------------------------ call shapes, contexts, reset, MX linears
@pytest.mark.parametrize("attention", [None, 2], ids=["uncond_only", "with_attention"])
def test_the_batched_call_equals_the_sequential_calls(setup, attention):
    sd, _, x, dx, txt = setup
    clock = {"t": 200.0}
    seq, bat = _model(sd, _config(clock, 2, attention)), _model(sd, _config(clock, 2, attention))
    for i in range(5):
        xi = x + 0.3 * i * dx
        a, b = _pair(seq, xi, txt, False), _pair(bat, xi, txt, True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), i
    assert bat.cache_log == seq.cache_log and [e[3] for e in bat.cache_log if e[0] == "uncond"] == [True, False, True, False, True]


def test_contexts_keep_separate_state_and_a_reset_starts_over(setup):
    sd, _, x, dx, txt = setup
    clock = {"t": 200.0}
    m = _model(sd, _config(clock, 2, 2))
    _fwd(m, "other", x, txt[:1])                                     # any other context: the unconditional-branch rule is inert
    _fwd(m, "other", x + dx, txt[:1])
    assert [e[3:] for e in m.cache_log] == [(True, True), (True, False)]
    _pair(m, x, txt, True)
    _pair(m, x + dx, txt, True)
    assert [e[1] for e in m.cache_log] == [0, 1, 0, 0, 1, 1] and m.cache_log[-1][3] is False
    with pytest.raises(ValueError, match="No context is set"):
        m(x.to(DEV).bfloat16(), TS.to(DEV), txt[:1].to(DEV).bfloat16(), return_dict=False)
    m._reset_stateful_cache()
    assert m._step_cache_states == {}
    fresh = _pair(_model(sd), x - dx, txt, True, cached=False)
    got = _pair(m, x - dx, txt, True)
    assert torch.equal(got[0], fresh[0]) and torch.equal(got[1], fresh[1])
    assert m.cache_log == [("cond", 0, 200.0, True, True), ("uncond", 0, 200.0, True, True)]
    m.disable_cache()
    assert m._step_cache_states == {}


def test_mxfp8_linears_compose(setup):
    sd, _, x, dx, txt = setup
    clock = {"t": 200.0}
    plain, m = _model(sd), _model(sd, _config(clock, 2, None))
    plain.enable_mxfp8_linears()
    m.enable_mxfp8_linears()
    c0, u0 = (t.clone() for t in _pair(m, x, txt, True))
    p0 = _pair(plain, x, txt, True, cached=False)
    assert torch.equal(c0, p0[0]) and torch.equal(u0, p0[1])
    c1, u1 = _pair(m, x + dx, txt, True)
    assert torch.equal(c1, _fwd(plain, "cond", x + dx, txt[:1])[0])
    dl, dh = ops.fastercache_delta(u0, c0)
    assert torch.equal(u1, ops.fastercache_apply(c1, dl, dh, *fastercache_weights(200.0, 1.0, 1.0, m._step_cache_config, m)))
