"""TaylorSeer caching on the Wan DiT (the tiny 3-block model and inputs of tests/test_pab_wan_gpu.py), in default and in lite
mode: against the cache-disabled forward (a schedule on which every forward computes must give its bits), against itself (on
an unchanged input the first-order factor is exactly zero, so a predicted forward gives the computing one's bits) and against
the restatement in tests/taylorseer_ref.py (the oracle's pieces in bf16) within the bound of a forward against the bf16
oracle, rel-RMS <= 1.5e-2.  The decisions are a function of the step counter alone, so the logs of model and restatement must
be equal entry by entry."""
import copy

import pytest
import torch

from frameino_amd.step_cache import TaylorSeerCacheConfig
from tests.parity import bf16_state_dict, hip_wan_model, rel_rms
from tests.taylorseer_ref import TaylorSeerRef
from tests.test_step_cache_wan_gpu import CFG, DEV, TS

pytestmark = pytest.mark.gpu
BOUND = 1.5e-2
MODES = pytest.mark.parametrize("lite", [False, True], ids=["default", "lite"])
C, P = True, False


@pytest.fixture(scope="module")
def setup():
    from oracle import wan_dit as W
    sd = W.wan_random_state_dict(CFG, seed=11, dtype=torch.float32, std=0.04)
    g = torch.Generator().manual_seed(12)
    x = torch.randn(1, 16, 5, 16, 20, generator=g)
    dx = torch.randn(1, 16, 5, 16, 20, generator=g)
    txt = torch.randn(1, 77, 256, generator=g)
    return sd, bf16_state_dict(sd), x, dx, txt


def _config(lite, interval=3, warmup=2, **kw):
    return TaylorSeerCacheConfig(cache_interval=interval, disable_cache_before_step=warmup, use_lite_mode=lite, **kw)


def _model(sd, config=None, dtype=torch.bfloat16):
    m = hip_wan_model(CFG, sd, DEV, dtype=dtype)
    if config is not None:
        m.enable_cache(config)
    return m


def _fwd(m, ctx, x, txt, ts=TS, dtype=torch.bfloat16, **kw):
    with m.cache_context(ctx):
        return m(x.to(DEV, dtype), ts.to(DEV), txt.to(DEV, dtype), return_dict=False, **kw)[0]


# ------------------------------------------------------------------ (a) schedules on which every forward computes
@MODES
@pytest.mark.parametrize("kw", [dict(interval=1), dict(warmup=9), dict(disable_cache_after_step=2)],
                         ids=["interval_1", "inside_the_warm_up", "after_step"])
def test_a_schedule_that_always_computes_equals_the_uncached_forward(setup, lite, kw):
    sd, _, x, dx, txt = setup
    plain, cached = _model(sd), _model(sd, _config(lite, **kw))
    for i in range(4):
        xi = x + 0.1 * i * dx
        assert torch.equal(_fwd(cached, "c", xi, txt), _fwd(plain, "c", xi, txt)), i
    assert cached.cache_log == [("c", i, True) for i in range(4)]


# ------------------------------------------------------------------ (b) an unchanged input: prediction gives the same bits
@MODES
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_a_predicted_forward_on_the_same_input_is_bit_identical(setup, lite, dtype):
    sd, _, x, _, txt = setup
    m = _model(sd, _config(lite, max_order=1), dtype=dtype)
    first = _fwd(m, "c", x, txt, dtype=dtype).clone()
    assert torch.equal(_fwd(m, "c", x, txt, dtype=dtype), first)                     # s = 1: computes, f_1 = (y - y) / 1
    for f in m._step_cache_states["c"].buffers.values():
        assert f.shape[0] == 2 and f.dtype == dtype and not f[1].any()               # the first-order factor: exactly zero
    assert len(m._step_cache_states["c"].buffers) == (1 if lite else 2 * CFG["num_layers"])
    for s in (2, 3):
        assert torch.equal(_fwd(m, "c", x, txt, dtype=dtype), first), s              # predicted, k = 1 and 2
    assert m.cache_log == [("c", 0, C), ("c", 1, C), ("c", 2, P), ("c", 3, P)]


@MODES
def test_mxfp8_linears_compose(setup, lite):
    sd, _, x, _, txt = setup
    m = _model(sd, _config(lite))
    m.enable_mxfp8_linears()
    first = _fwd(m, "c", x, txt).clone()
    for s in range(1, 4):
        assert torch.equal(_fwd(m, "c", x, txt), first), s
    assert [e[2] for e in m.cache_log] == [C, C, P, P]


def test_fp32_factors_on_the_same_input(setup):
    sd, _, x, _, txt = setup
    m = _model(sd, _config(False, max_order=2, taylor_factors_dtype=torch.float32))
    first = _fwd(m, "c", x, txt).clone()
    for s in range(1, 4):
        assert torch.equal(_fwd(m, "c", x, txt), first), s
    f = m._step_cache_states["c"].buffers["self", 0]
    assert f.dtype == torch.float32 and f.shape[0] == 3 and m._step_cache_states["c"].n == 2


# ------------------------------------------------------------------ (c), (d) changed inputs: the restatement
_SEPARATED = {}


def _separating_inputs(sdb, x, dx, txt, lite):
    """inputs x + s * scale * dx for s = 0 .. last, with the scale -- and the predicted forward `last` that carries the
    condition, s = 2 (k = 1) or s = 3 (k = 2) -- chosen on the CPU from the restatement alone: its order-1 prediction at `last`
    must differ by at least 5 x the bound both from its order-0 prediction (the re-use of forward 1's outputs, what Pyramid
    Attention Broadcast does) and from a fresh forward there -- else a model that re-uses, or one that silently recomputes,
    would pass.  (Default mode: at k = 1 no scale reaches 5 x the bound on both sides -- at scale 1 the gaps are 0.079 to
    re-use and 0.061 to recomputation --, at k = 2 they are 0.114 and 0.095; lite mode: 0.66 and 0.44 at k = 1.)"""
    if lite in _SEPARATED:
        return _SEPARATED[lite]
    b16 = lambda t: t.bfloat16()                                                      # noqa: E731
    for last in (2, 3):
        for scale in (1.0, 2.0, 0.5, 4.0):
            xs = [x + s * scale * dx for s in range(last + 1)]
            ref = TaylorSeerRef(sdb, CFG, _config(lite))
            for v in xs[:-1]:
                ref("c", b16(v), TS, b16(txt))
            reuse = copy.deepcopy(ref)
            reuse.order = 0
            order1, order0 = ref("c", b16(xs[-1]), TS, b16(txt)), reuse("c", b16(xs[-1]), TS, b16(txt))
            fresh = TaylorSeerRef(sdb, CFG, _config(lite, interval=1))("c", b16(xs[-1]), TS, b16(txt))
            assert ref.log[-1] == reuse.log[-1] == ("c", last, False)
            gaps = (rel_rms(order1, order0), rel_rms(order1, fresh))
            if min(gaps) >= 5 * BOUND:
                _SEPARATED[lite] = (xs, gaps)
                return _SEPARATED[lite]
    raise AssertionError(f"no scale separates extrapolation from re-use and from recomputation: last gaps {gaps}")


@MODES
def test_changed_inputs_match_the_restatement(setup, lite):
    sd, sdb, x, dx, txt = setup
    xs, gaps = _separating_inputs(sdb, x, dx, txt, lite)
    assert min(gaps) >= 5 * BOUND                                                     # (on the restatement alone)
    m, ref = _model(sd, _config(lite)), TaylorSeerRef(sdb, CFG, _config(lite))
    for s, v in enumerate(xs):                                                        # compute, compute, predict (k = 1, 2)
        out, want = _fwd(m, "c", v, txt), ref("c", v.bfloat16(), TS, txt.bfloat16())
        err = rel_rms(out, want)
        print(f"lite={lite}: forward {s}: rel-RMS {err:.3e} against the restatement (gaps of forward {len(xs) - 1} to re-use / "
              f"recomputation {gaps[0]:.3e} / {gaps[1]:.3e})")
        assert err < BOUND, s
    assert m.cache_log == ref.log == [("c", s, s < 2) for s in range(len(xs))]


@MODES
def test_logs_of_model_and_restatement_are_equal(setup, lite):
    """(d) a longer schedule in two contexts, one of them a forward ahead, with `disable_cache_after_step` and order 2: the
    decisions entry by entry (the outputs are test (c)'s business)"""
    sd, sdb, x, dx, txt = setup
    kw = dict(disable_cache_after_step=6, max_order=2)
    m, ref = _model(sd, _config(lite, **kw)), TaylorSeerRef(sdb, CFG, _config(lite, **kw))
    calls = [("uncond", 0)] + [(ctx, s) for s in range(8) for ctx in ("cond", "uncond")]
    for ctx, s in calls:
        v = x + 0.05 * s * dx
        assert bool(torch.isfinite(_fwd(m, ctx, v, txt)).all())
        ref(ctx, v.bfloat16(), TS, txt.bfloat16())
    assert m.cache_log == ref.log and len(ref.log) == 17
    assert [e[2] for e in m.cache_log if e[0] == "cond"] == [C, C, P, P, C, P, C, C]
    assert [e[1:] for e in m.cache_log if e[0] == "uncond"] == [(s, c) for s, c in enumerate([C, C, P, P, C, P, C, C, C])]
    assert m._step_cache_states["cond"].n == 3


# ------------------------------------------------------------------ (e) launch counts
def test_launch_counts(setup, monkeypatch):
    from frameino_amd import ops
    sd, _, x, dx, txt = setup
    counts = {}

    def spy(name):
        real = getattr(ops, name)

        def f(*a, **k):
            counts[name] = counts.get(name, 0) + 1
            return real(*a, **k)
        monkeypatch.setattr(ops, name, f)
    for name in ("attention", "attention_tail", "attention_probs", "gemm", "qkv_rmsnorm_rope_", "pab_broadcast", "taylor_update",
                 "taylor_predict", "adaln_modulate", "unpatchify"):
        spy(name)
    layers = CFG["num_layers"]
    attn = lambda: sum(counts.get(k, 0) for k in ("attention", "attention_tail", "attention_probs"))      # noqa: E731
    plain = _model(sd)
    _fwd(plain, "c", x, txt)
    counts.clear()
    _fwd(plain, "c", x, txt)
    uncached = dict(counts)
    assert "taylor_update" not in uncached and "taylor_predict" not in uncached
    # default mode
    m = _model(sd, _config(False))
    _fwd(m, "c", x, txt)
    counts.clear()
    _fwd(m, "c", x + dx, txt)                                            # s = 1: computes
    assert counts["taylor_update"] == 2 * layers and counts.get("taylor_predict", 0) == 0
    assert {k: v for k, v in counts.items() if k != "taylor_update"} == uncached      # ... and is the uncached forward otherwise
    counts.clear()
    _fwd(m, "c", x - dx, txt)                                            # s = 2: predicts
    assert attn() == 0 and counts.get("qkv_rmsnorm_rope_", 0) == 0 and counts.get("taylor_update", 0) == 0
    assert counts["taylor_predict"] == 2 * layers and counts.get("pab_broadcast", 0) == 0
    # the GEMMs the predicting forward left out: QKV + out-projection, to_q + out-projection of the text branch, per block
    assert uncached["gemm"] - counts["gemm"] == 4 * layers
    # lite mode
    m = _model(sd, _config(True))
    _fwd(m, "c", x, txt)
    counts.clear()
    _fwd(m, "c", x + dx, txt)                                            # computes: the uncached forward + one update
    assert counts["taylor_update"] == 1 and {k: v for k, v in counts.items() if k != "taylor_update"} == uncached
    counts.clear()
    _fwd(m, "c", x - dx, txt)                                            # predicts: one launch and the unpatchify
    assert counts == {"taylor_predict": 1, "unpatchify": 1}


# ------------------------------------------------------------------ (f), (g) contexts, reset, batches
@MODES
def test_contexts_keep_separate_state_and_a_reset_starts_over(setup, lite):
    sd, _, x, dx, txt = setup
    m = _model(sd, _config(lite))
    a = _fwd(m, "cond", x, txt).clone()
    b = _fwd(m, "uncond", x + dx, txt).clone()                          # its own state: s = 0, computes
    assert not torch.equal(a, b)
    for s in range(1, 4):
        assert torch.equal(_fwd(m, "cond", x, txt), a), s                # s = 2, 3: predicted from cond's own factors
        assert torch.equal(_fwd(m, "uncond", x + dx, txt), b), s
    assert m.cache_log == [(c, s, s < 2) for s in range(4) for c in ("cond", "uncond")]
    with pytest.raises(ValueError, match="No context is set"):
        m(x.to(DEV).bfloat16(), TS.to(DEV), txt.to(DEV).bfloat16(), return_dict=False)
    # (g) a reset: the counter starts at 0 again, the next forward computes on its input and a new log begins
    m._reset_stateful_cache()
    assert m._step_cache_states == {}
    fresh = _fwd(_model(sd), "c", x - dx, txt)
    assert torch.equal(_fwd(m, "cond", x - dx, txt), fresh) and m.cache_log == [("cond", 0, C)]
    m.disable_cache()
    assert m._step_cache_states == {} and all(getattr(ws, "taylor_y", None) is None for ws in m._ws.values())
    assert torch.equal(m(x.to(DEV).bfloat16(), TS.to(DEV), txt.to(DEV).bfloat16(), return_dict=False)[0], a)     # no context needed


@MODES
@pytest.mark.parametrize("ahead", [0, 1], ids=["lockstep", "uncond_one_ahead"])
def test_a_batch_with_contexts_equals_sequential_calls(setup, lite, ahead):
    """batch 2 with _cache_contexts=("cond", "uncond") == the two calls one after the other, bit for bit, logs included; with
    "uncond" one forward ahead the two elements of a batched call decide differently"""
    sd, _, x, dx, txt = setup
    t2 = torch.cat([txt, txt.flip(1)])
    seq, bat = _model(sd, _config(lite)), _model(sd, _config(lite))
    for m in (seq, bat):
        for _ in range(ahead):
            _fwd(m, "uncond", x - dx, t2[1:])
    for i in range(5):
        xi = x + 0.3 * i * dx
        want = torch.cat([_fwd(seq, "cond", xi, t2[:1]), _fwd(seq, "uncond", xi, t2[1:])])
        got = _fwd(bat, "cfg", xi.expand(2, -1, -1, -1, -1), t2, _cache_contexts=("cond", "uncond"))
        assert torch.equal(got, want), i
    assert bat.cache_log == seq.cache_log
    decided = [e[2] for e in bat.cache_log[ahead:]]
    assert (decided[0::2] != decided[1::2]) == bool(ahead)


@MODES
def test_a_batch_under_one_context_and_live_rows(setup, lite):
    """batch 2 under one context: one counter, one buffer per hooked tensor for all rows, each element as it gives alone;
    `live_rows` is not honoured under the cache (the factors cover every row): the kept rows read as the restatement"""
    sd, sdb, x, dx, txt = setup
    t2 = torch.cat([txt, txt.flip(1)])
    joint, alone = _model(sd, _config(lite)), _model(sd, _config(lite))
    for i in range(4):
        xs = torch.cat([x + 0.3 * i * dx, x - 0.2 * i * dx])
        got = _fwd(joint, "c", xs, t2)
        want = torch.cat([_fwd(alone, f"e{k}", xs[k:k + 1], t2[k:k + 1]) for k in range(2)])
        assert torch.equal(got, want), i
    assert joint.cache_log == [("c", 0, C), ("c", 1, C), ("c", 2, P), ("c", 3, P)]
    assert next(iter(joint._step_cache_states["c"].buffers.values())).shape[1] == 2 * 400
    m, ref = _model(sd, _config(lite)), TaylorSeerRef(sdb, CFG, _config(lite))
    rows_per_frame = (16 // 2) * (20 // 2)
    for i, v in enumerate((x, x + 0.1 * dx, x + 0.2 * dx)):
        out = _fwd(m, "c", v, txt, live_rows=(rows_per_frame, 5 * rows_per_frame))
        want = ref("c", v.bfloat16(), TS, txt.bfloat16())
        assert rel_rms(out[:, :, 1:], want[:, :, 1:]) < BOUND, i
    assert m.cache_log == ref.log
