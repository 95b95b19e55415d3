"""MagCache without a GPU: the rule (`magcache_decide`) against its restatement in exact arithmetic (tests/magcache_ref.py), the
config with its validation, resampling, per-context curves and persistence, the model's surface and per-context state machine
(`_magcache_begin` / `_magcache_finish` over stand-in ops), the C ABI's new symbols and their argument checks."""
import ctypes
import json
import math
from fractions import Fraction

import pytest
import torch

from frameino_amd import _lib
from frameino_amd import step_cache as S
from frameino_amd.step_cache import (FirstBlockCacheConfig, MagCacheConfig, load_mag_ratios, magcache_decide, save_mag_ratios)
from tests import magcache_ref as R
from tests.test_step_cache_cpu import _model, _pipe

C, K = True, False              # computes / skips


def _trace(forwards, cfg, ratios):
    """the model-independent fold of `magcache_decide` over consecutive forwards of one context, wrapping at N"""
    out, s, st = [], 0, S.MAG_FRESH
    for _ in range(forwards):
        compute, st = magcache_decide(s, st, cfg, ratios)
        out.append((s, compute, st[2], st[1]))
        s += 1
        if s == cfg.num_inference_steps:
            s, st = 0, S.MAG_FRESH
    return out


# ------------------------------------------------------------------ the rule
def test_the_worked_example():
    cfg = MagCacheConfig(num_inference_steps=10, mag_ratios=[0.98] * 10)
    got = _trace(10, cfg, cfg.mag_ratios)
    assert [c for _, c, _, _ in got] == [C, C, K, K, C, K, K, C, K, K]
    assert S.magcache_retention(cfg) == 2
    assert math.isclose(got[2][2], 0.02, rel_tol=1e-12) and math.isclose(got[3][2], 0.0596, rel_tol=1e-12)
    margins = R.decision_margins(10, [0.98] * 10, 10)
    # the fifth forward saw 0.02 + 0.0396 + 0.058808 = 0.118408, above the threshold
    assert abs(margins[2] - (Fraction(118408, 10 ** 6) - Fraction(6, 100))) < Fraction(1, 10 ** 12)


CURVES = {
    "worked": dict(n=10, ratios=[0.98] * 10),
    "max_skip_binds": dict(n=12, ratios=[1.0] * 12, max_skip_steps=2),
    "retention_0": dict(n=8, ratios=[0.99] * 8, retention_ratio=0.0),
    "retention_1": dict(n=8, ratios=[0.5] * 8, retention_ratio=1.0),
    "threshold_0": dict(n=8, ratios=[1.0, 1.0, 1.0, 0.97, 1.0, 1.0, 0.99, 1.0], threshold=0.0),
    "short_curve": dict(n=12, ratios=[0.97, 0.97, 0.97, 0.97, 0.97], max_skip_steps=4, threshold=0.1),
    "decaying": dict(n=16, ratios=[1.0, 1.0, 0.99, 0.995, 0.99, 0.98, 0.985, 0.97, 0.96, 0.97, 0.95, 0.93, 0.9, 0.85, 0.8, 0.7],
                     threshold=0.08, max_skip_steps=3, retention_ratio=0.125),
    "rising": dict(n=9, ratios=[1.02] * 9, threshold=0.05, retention_ratio=0.1),
}


@pytest.mark.parametrize("name", list(CURVES))
def test_the_rule_against_exact_arithmetic(name):
    kw = dict(CURVES[name])
    n, ratios = kw.pop("n"), kw.pop("ratios")
    forwards = 2 * n + 3                                         # past the wrap at N, twice
    # a condition on the inputs: no decision sits within 1e-6 of the threshold, so float and exact arithmetic cannot disagree
    # (threshold 0 with ratios of exactly 1.0 compares 0 <= 0 in both arithmetics: exact on either side)
    margins = R.decision_margins(forwards, ratios, n, **kw)
    assert all(m >= Fraction(1, 10 ** 6) or (m == 0 and kw.get("threshold") == 0.0) for m in margins), min(margins)
    cfg = MagCacheConfig(num_inference_steps=n, mag_ratios=ratios, **kw)
    got, want = _trace(forwards, cfg, ratios), R.rule_trace(forwards, ratios, n, **kw)
    assert [(s, c, k) for s, c, _, k in got] == [(s, c, k) for s, c, _, k in want]
    assert all(abs(Fraction(a[2]) - b[2]) < Fraction(1, 10 ** 9) for a, b in zip(got, want))
    assert [s for s, _, _, _ in got] == [i % n for i in range(forwards)]      # the wrap at N


def test_the_edges_of_the_rule():
    dec = lambda name: [c for _, c, _, _ in _trace(CURVES[name]["n"], MagCacheConfig(              # noqa: E731
        num_inference_steps=CURVES[name]["n"], mag_ratios=CURVES[name]["ratios"],
        **{k: v for k, v in CURVES[name].items() if k not in ("n", "ratios")}), CURVES[name]["ratios"])]
    assert dec("max_skip_binds") == [C, C, K, K, C, K, K, C, K, K, C, K]         # R = 2; the error stays 0: the count binds
    assert dec("retention_0") == [C, K, K, K, C, K, K, K]                        # forward 0: no residual yet
    assert dec("retention_1") == [C] * 8
    assert dec("threshold_0") == [C, C, K, C, K, K, C, K]                        # R = 2; any error at all computes
    # a curve shorter than the counter scales by 1.0 beyond it: the error keeps growing by the same |1 - acc_ratio|
    cfg = MagCacheConfig(num_inference_steps=12, max_skip_steps=4, threshold=0.1)
    cfg.mag_ratios = [0.97] * 5
    compute, (ratio, steps, err, has) = magcache_decide(7, (0.97, 1, 0.03, True), cfg, cfg.mag_ratios)
    assert (compute, ratio, steps, has) == (False, 0.97, 2, True) and math.isclose(err, 0.06, rel_tol=1e-12)
    assert magcache_decide(4, (0.97, 1, 0.03, True), cfg, cfg.mag_ratios)[1][0] == 0.97 * 0.97
    # no residual: compute and reset, whatever the error; calibrate: compute, accumulators untouched
    assert magcache_decide(5, (1.0, 0, 0.0, False), cfg, [1.0] * 12) == (True, (1.0, 0, 0.0, True))
    cal = MagCacheConfig(calibrate=True)
    assert magcache_decide(20, (0.9, 2, 0.05, True), cal, None) == (True, (0.9, 2, 0.05, True))
    assert all(isinstance(magcache_decide(s, S.MAG_FRESH, cfg, [1.0] * 12)[0], bool) for s in range(12))


# ------------------------------------------------------------------ config
def test_config_defaults_are_diffusers():
    c = MagCacheConfig(calibrate=True)
    assert (c.threshold, c.max_skip_steps, c.retention_ratio, c.num_inference_steps, c.mag_ratios) == (0.06, 3, 0.2, 28, None)
    assert MagCacheConfig().calibrate is False


@pytest.mark.parametrize("bad", [dict(threshold=-0.1), dict(threshold=float("nan")), dict(threshold="x"),
                                 dict(max_skip_steps=-1), dict(max_skip_steps=1.5), dict(max_skip_steps=True),
                                 dict(retention_ratio=-0.01), dict(retention_ratio=1.01), dict(retention_ratio=None),
                                 dict(num_inference_steps=0), dict(num_inference_steps=2.0),
                                 dict(mag_ratios=[1.0, 0.0]), dict(mag_ratios=[1.0, -0.5]), dict(mag_ratios=[float("inf")]),
                                 dict(mag_ratios=[float("nan")]), dict(mag_ratios=[]), dict(mag_ratios=["a"]),
                                 dict(mag_ratios=3.0), dict(mag_ratios={"cond": [1.0, 0.0]}), dict(mag_ratios={})],
                         ids=lambda b: "-".join(f"{k}={v}" for k, v in b.items()))
def test_bad_values_raise_and_name_the_field(bad):
    m = _model()
    kw = dict(mag_ratios=[1.0] * 4, num_inference_steps=4)
    kw.update(bad)
    with pytest.raises(ValueError, match=next(iter(bad))):
        m.enable_cache(MagCacheConfig(**kw))
    assert not m.is_cache_enabled


def test_no_curve_and_no_calibration_says_how_to_calibrate():
    m = _model()
    with pytest.raises(ValueError, match="calibrate=True"):
        m.enable_cache(MagCacheConfig())
    assert not m.is_cache_enabled
    m.enable_cache(MagCacheConfig(calibrate=True))            # a calibrating run needs no curve
    assert m.is_cache_enabled and m._mag_on


def test_resampling_by_nearest_index():
    five, nine = [1.0, 0.9, 0.8, 0.7, 0.6], [1.0, 0.95, 0.9, 0.85, 0.8, 0.75, 0.7, 0.65, 0.6]
    # src[round(i * 4 / 8)], Python's round (half to even): indices 0 0 1 2 2 2 3 4 4
    assert S.magcache_resample(five, 9) == [1.0, 1.0, 0.9, 0.8, 0.8, 0.8, 0.7, 0.6, 0.6]
    assert S.magcache_resample(nine, 5) == [1.0, 0.9, 0.8, 0.7, 0.6]                  # src[2 i]
    assert S.magcache_resample(nine, 1) == [0.6] and S.magcache_resample([0.5], 3) == [0.5] * 3
    assert S.magcache_resample(torch.tensor(five, dtype=torch.float64), 5) == five
    assert S.magcache_curve(MagCacheConfig(mag_ratios=five, num_inference_steps=9), "any") == S.magcache_resample(five, 9)
    assert S.magcache_curve(MagCacheConfig(mag_ratios=torch.tensor(nine), num_inference_steps=1), None) == [
        float(torch.tensor(0.6, dtype=torch.float32))]
    assert S.magcache_curve(MagCacheConfig(calibrate=True), "cond") is None


def test_a_mapping_gives_every_context_its_curve():
    a, b = [1.0, 0.9, 0.8], [1.0, 0.99, 0.98]
    cfg = MagCacheConfig(mag_ratios={"cond": a, "uncond": b}, num_inference_steps=3)
    assert S.magcache_curve(cfg, "cond") == a and S.magcache_curve(cfg, "uncond") == b
    assert S.magcache_curve(cfg, "cfg") == a and S.magcache_curve(cfg, None) == a          # unnamed: the "cond" entry
    with pytest.raises(ValueError, match="no \"cond\" entry"):
        S.magcache_curve(MagCacheConfig(mag_ratios={"uncond": b}, num_inference_steps=3), "cfg")
    m = _model()
    m.enable_cache(MagCacheConfig(mag_ratios={"uncond": b}, num_inference_steps=3))
    with m.cache_context("c"), pytest.raises(ValueError, match="no curve for context 'c'"):
        m._magcache_begin(1, 4, 8, torch.bfloat16, "cpu")
    assert m.cache_log == () or m.cache_log == []                # refused before the forward counted


def test_a_duck_typed_config_is_accepted_and_a_bare_name_is_not():
    class MagCacheConfig:                                        # noqa: F811  what diffusers' own class looks like from here
        def __init__(self):
            self.threshold, self.max_skip_steps, self.retention_ratio, self.num_inference_steps = 0.06, 3, 0.2, 10
            self.mag_ratios, self.calibrate = torch.full((10,), 0.98, dtype=torch.float64), False

    m = _model()
    cfg = MagCacheConfig()
    m.enable_cache(cfg)
    assert m.is_cache_enabled and m._mag_on and not m._taylor_on and not m._pab_on
    assert [c for _, c, _, _ in _trace(10, cfg, S.magcache_curve(cfg, "cond"))] == [C, C, K, K, C, K, K, C, K, K]
    m.disable_cache()

    class Bare:
        pass
    Bare.__name__ = "MagCacheConfig"
    with pytest.raises(NotImplementedError, match="MagCacheConfig.*`threshold`.*`mag_ratios`"):
        m.enable_cache(Bare())
    assert not m.is_cache_enabled


def test_mag_ratios_round_trip(tmp_path):
    cal = {"cond": {"mag_ratios": [1.0, 0.987654321, 0.5], "cos_dist": [0.0, 0.01, 0.2]},
           "uncond": {"mag_ratios": [1.0, 0.9, 0.8], "cos_dist": [0.0, 0.02, 0.3]}}
    path = tmp_path / "curves.json"
    save_mag_ratios(path, cal)
    assert load_mag_ratios(path) == {"cond": [1.0, 0.987654321, 0.5], "uncond": [1.0, 0.9, 0.8]}
    d = json.loads(path.read_text())
    assert d["format"] == "frameino_amd.mag_ratios" and d["version"] == 1 and d["contexts"]["cond"]["cos_dist"] == [0.0, 0.01, 0.2]
    save_mag_ratios(path, {"cond": [1.0, 0.5]})                  # bare curves too
    assert load_mag_ratios(path) == {"cond": [1.0, 0.5]}
    _model().enable_cache(MagCacheConfig(mag_ratios=load_mag_ratios(path), num_inference_steps=2))
    for text in ('{"format": "frameino_amd.sparse_thresholds", "version": 1}', '{"contexts": {}}', "[1.0, 0.9]"):
        path.write_text(text)
        with pytest.raises(ValueError, match="not a file of save_mag_ratios"):
            load_mag_ratios(path)


# ------------------------------------------------------------------ surface
def _config(**kw):
    kw.setdefault("mag_ratios", [0.98] * 10)
    kw.setdefault("num_inference_steps", 10)
    return MagCacheConfig(**kw)


def test_exclusivity_and_disable_restores_the_model():
    m = _model()
    before = dict(vars(m))
    m.enable_cache(_config())
    assert m._step_cache_segments(1, 8) is None and m._taylor_begin(1, 4, 8, torch.bfloat16, "cpu") is None
    for other in (FirstBlockCacheConfig(), _config()):
        with pytest.raises(ValueError, match="already been enabled"):
            m.enable_cache(other)
    with m.cache_context("c"):
        m._magcache_begin(1, 8, 8, torch.bfloat16, "cpu")
    assert m._step_cache_states and m.cache_log == [("c", 0, True, 0.0, 0)]
    m.disable_cache()
    assert not m.is_cache_enabled and not m._mag_on and m._step_cache_states == {} and m._step_cache_config is None
    assert m._magcache_begin(1, 8, 8, torch.bfloat16, "cpu") is None
    after = dict(vars(m))
    for k in ("_step_cache_states", "_step_cache_log_fresh", "cache_log", "_step_cache_config"):
        before.pop(k, None), after.pop(k, None)                # (the state dict, now empty, and the log the call left)
    assert after.keys() == before.keys() and all(after[k] is before[k] or after[k] == before[k] for k in before)
    m.enable_cache(FirstBlockCacheConfig())                    # ... and another cache can follow


def test_the_policy_and_its_refusals():
    from tests.test_taylorseer_cpu import _Shard, _first_next, _tiny_model
    from frameino_amd.attention_processor import MI355WanAttnProcessor
    from frameino_amd.window_attention import SparseAttentionConfig, WindowAttentionConfig
    policy = S._POLICIES["MagCacheConfig"]
    assert policy is S._MagCachePolicy and policy in S.StepCacheMixin._cache_policies
    assert policy not in S.PyramidAttentionBroadcastMixin._cache_policies and "MagCacheConfig" not in S._OTHER_DIFFUSERS_CONFIGS
    assert policy.batched and not policy.hooks_attention(_config()) and policy.takes_windows(_config())
    assert "use_hip_graph=True with MagCache" in str(policy.capture_refusal()) and policy.why_eager in str(policy.capture_refusal())
    m = _tiny_model()
    # it leaves the attention branches alone: window attention, sparse attention and a user's processor are none of its business

    class Mine(MI355WanAttnProcessor):
        pass

    m.enable_window_attention(WindowAttentionConfig(1))
    m.enable_cache(_config())
    m.disable_cache()
    m.disable_window_attention()
    m.enable_cache(_config())
    m.enable_sparse_attention(SparseAttentionConfig(0.5))
    m.disable_sparse_attention()
    m.disable_cache()
    m.blocks[1].attn1.set_processor(Mine())
    m.enable_cache(_config())
    m.disable_cache()
    # a token-sharded plan: on the model at enable time, or handed to the forward (refused before any launch)
    m.parallel = _Shard()
    with pytest.raises(NotImplementedError, match="MagCache with a token-sharded plan.*one GPU"):
        m.enable_cache(_config())
    m.parallel = None
    m.enable_cache(_config())
    with m.cache_context("c"), pytest.raises(NotImplementedError, match="one GPU"):
        _first_next(m, shard=_Shard())
    assert m.cache_log == () or m.cache_log == []                # refused before the forward counted


def test_cogvideox_keeps_refusing_it():
    from frameino_amd.cogvideox_transformer_3d import CogVideoXTransformer3DModel
    m = CogVideoXTransformer3DModel(num_attention_heads=2, attention_head_dim=64, in_channels=4, out_channels=4, num_layers=1,
                                    text_embed_dim=32, time_embed_dim=32, sample_width=8, sample_height=8, sample_frames=5,
                                    use_rotary_positional_embeddings=True)
    with pytest.raises(NotImplementedError, match="MagCacheConfig.*PyramidAttentionBroadcastConfig is$"):
        m.enable_cache(_config())                                # the fully attributed config too
    assert not m.is_cache_enabled


# ------------------------------------------------------------------ state machine over stand-in ops
class _FakeOps:
    """the two entries MagCache calls, in plain torch (the calibration quantity from the restatement)"""

    def __init__(self):
        self.calls = []

    def step_cache_residual(self, a, b, out=None, subtract=True):
        self.calls.append("sub" if subtract else "add")
        return out.copy_(a - b if subtract else a + b)

    def magcache_calibrate(self, x_out, x_in, r_prev, r_new, stats):
        self.calls.append("calibrate")
        new = x_out - x_in
        stats.copy_(torch.tensor(R.calibration(new, r_prev), dtype=torch.float64))
        return r_new.copy_(new)


def _forward(m, ctxs, x_in, x_out, b=1):
    """one forward's cache steps on synthetic rows: decisions, then the finish stage on a copy of the stack's output"""
    n = x_in.shape[0] // b
    with m.cache_context("cfg" if isinstance(ctxs, tuple) else ctxs):
        plan = m._magcache_begin(b, n, x_in.shape[1], x_in.dtype, "cpu", ctxs if isinstance(ctxs, tuple) else None)
    x = x_out.clone() if any(s.compute for s in plan.segs) else torch.full_like(x_out, float("nan"))
    m._magcache_finish(plan, x, x_in)
    return plan, x


def test_state_machine_log_contexts_wrap_and_reset():
    m = _model()
    m.ops = _FakeOps()
    m.enable_cache(_config(mag_ratios={"cond": [1.0] * 6, "uncond": [0.5] * 6}, num_inference_steps=6, retention_ratio=0.0,
                           max_skip_steps=2))
    g = torch.Generator().manual_seed(5)
    ins = [torch.randn(8, 8, generator=g) for _ in range(8)]
    outs = [torch.randn(8, 8, generator=g) for _ in range(8)]
    kept = None
    for i in range(6):
        plan, x = _forward(m, ("cond", "uncond"), ins[i], outs[i], b=2)
        cond, uncond = plan.segs
        assert (cond.name, cond.r0, cond.r1, uncond.name, uncond.r0, uncond.r1) == ("cond", 0, 4, "uncond", 4, 8)
        assert uncond.compute and torch.equal(x[4:], outs[i][4:])            # 0.5 per step: always above the threshold
        if cond.compute:
            kept = outs[i][:4] - ins[i][:4]
            assert torch.equal(x[:4], outs[i][:4])
        else:
            assert torch.equal(x[:4], ins[i][:4] + kept)                     # the rows of the skipping segment alone
    assert [e[2] for e in m.cache_log if e[0] == "cond"] == [C, K, K, C, K, K]
    assert [e[:3] for e in m.cache_log if e[0] == "uncond"] == [("uncond", s, C) for s in range(6)]
    assert m._step_cache_states == {}                            # both counters reached N = 6: both contexts started over
    plan, x = _forward(m, "cond", ins[6][:4], outs[6][:4])
    assert m.cache_log[-1] == ("cond", 0, C, 0.0, 0) and m.ops.calls[-1] == "sub"       # residual dropped: computes again
    # every segment skips: the stack's output is not read at all
    calls = len(m.ops.calls)
    plan, x = _forward(m, "cond", ins[7][:4], outs[7][:4])
    assert not plan.segs[0].compute and torch.equal(x, ins[7][:4] + (outs[6][:4] - ins[6][:4])) and m.ops.calls[calls:] == ["add"]
    # a reset starts over and the next forward starts a new log; without a context a forward raises
    m._reset_stateful_cache()
    assert m._step_cache_states == {} and len(m.cache_log) == 14
    _forward(m, "cond", ins[0][:4], outs[0][:4])
    assert m.cache_log == [("cond", 0, C, 0.0, 0)]
    with pytest.raises(ValueError, match="No context is set"):
        m._magcache_begin(1, 4, 8, torch.float32, "cpu")
    # other rows: the context starts over
    _forward(m, "cond", ins[0], outs[0])
    assert m.cache_log[-1][:3] == ("cond", 0, C)


def test_calibrate_mode_records_one_row_per_step_and_files_it_once():
    m = _model()
    m.ops = _FakeOps()
    m.enable_cache(MagCacheConfig(calibrate=True, num_inference_steps=4))
    g = torch.Generator().manual_seed(6)
    ins = [torch.randn(6, 8, generator=g) for _ in range(6)]
    outs = [torch.randn(6, 8, generator=g) for _ in range(6)]
    for i in range(3):
        plan, x = _forward(m, "cond", ins[i], outs[i])
        assert plan.calibrate and plan.segs[0].compute and torch.equal(x, outs[i])
    assert m.magcache_calibration is None                       # nothing is read before the context starts over
    _forward(m, "cond", ins[3], outs[3])
    cal = m.magcache_calibration["cond"]
    res = [o - i for i, o in zip(ins, outs)]
    want = [(1.0, 0.0)] + [R.calibration(res[i], res[i - 1]) for i in range(1, 4)]
    assert cal["mag_ratios"] == [w[0] for w in want] and cal["cos_dist"] == [w[1] for w in want]
    assert m.ops.calls == ["sub", "calibrate", "calibrate", "calibrate"]
    assert m.cache_log == [("cond", s, True, None, None) for s in range(4)] and m._step_cache_states == {}
    # a reset files what an unfinished context has recorded
    _forward(m, "uncond", ins[4], outs[4])
    _forward(m, "uncond", ins[5], outs[5])
    m._reset_stateful_cache()
    assert m.magcache_calibration["uncond"]["mag_ratios"] == [1.0, R.calibration(res[5], res[4])[0]]
    assert m.magcache_calibration["cond"] is cal


def test_pipeline_limits_warning_and_reset():
    pipe = _pipe()
    tr = pipe.transformer
    tr.enable_cache(_config())
    assert pipe._step_cache_check(1) is True and pipe._step_cache_check(2) is True        # a batch is allowed
    pipe.use_hip_graph = True
    with pytest.raises(RuntimeError, match="use_hip_graph=True with MagCache"):
        pipe._step_cache_check(1)
    pipe.use_hip_graph = None
    pipe.parallel = object()
    with pytest.raises(NotImplementedError, match="MagCache runs on one GPU"):
        pipe._step_cache_check(1)
    pipe.parallel = None
    with tr.cache_context("cond"):
        tr._magcache_begin(1, 4, 8, torch.bfloat16, "cpu")
    assert tr._step_cache_states and tr.cache_log == [("cond", 0, True, 0.0, 0)]
    pipe.maybe_free_model_hooks()
    assert tr._step_cache_states == {} and len(tr.cache_log) == 1


# ------------------------------------------------------------------ the C ABI
def test_the_new_symbols_are_declared_exported_and_bound():
    lib = _lib.lib()
    for name in ("fino_magcache_calibrate", "fino_magcache_workspace_bytes"):
        assert name in _lib.declared_symbols() and name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.fino_version() == 103 == _lib.ABI_VERSION
    assert len(_lib.SIGNATURES["fino_magcache_calibrate"]) == 15
    # one fp64 pair per wave; the wave count depends on the rows alone and is capped
    sizes = [lib.fino_magcache_workspace_bytes(r) for r in (0, 1, 4, 5, 1188, 24640, 2 ** 31 - 1)]
    assert sizes[0] == 0 and sizes[1] == sizes[2] == 4 * 16 and sizes[3] == 8 * 16 and sizes[4] == 1188 * 16
    assert sizes[5] == sizes[6] and sizes[5] % 16 == 0 and 24640 * 16 >= sizes[5] >= 4096 * 16


def test_the_c_abi_checks_before_any_launch():
    lib = _lib.lib()
    a = 4096                                                      # any 16-byte aligned address: nothing is dereferenced
    ws = lib.fino_magcache_workspace_bytes(4)
    good = [a, 8, a, 8, a, 8, a, 8, 4, 8, 0, a, a, ws, 0]       # bf16 [4, 8]
    X_OUT, LD_OUT, X_IN, LD_IN, R_PREV, LD_PREV, R_NEW, LD_NEW, ROWS, DIM, DTYPE, STATS, WS, WS_BYTES = range(14)
    cases = [({p: 0}, b"null pointer") for p in (X_OUT, X_IN, R_PREV, R_NEW, STATS, WS)]
    cases += [({DIM: 12, LD_OUT: 16, LD_IN: 16, LD_PREV: 16, LD_NEW: 16}, b"dim=12"), ({DIM: 0}, b"dim=0"),
              ({DTYPE: 2, DIM: 6}, b"dim=6"),                     # fp32: a vector is 4 elements
              ({DTYPE: 3}, b"dtype"), ({ROWS: 0}, b"rows=0"), ({ROWS: 2 ** 31}, b"rows=2147483648")]
    cases += [({p: 0}, b"row stride is below dim") for p in (LD_OUT, LD_IN, LD_PREV, LD_NEW)]
    cases += [({p: a + 2}, b"alignment") for p in (X_OUT, X_IN, R_PREV, R_NEW, WS)] + [({STATS: a + 8}, b"alignment")]
    cases += [({LD_IN: 12}, b"alignment"),                       # rows that do not start on 16 bytes
              ({LD_NEW: 16}, b"aliases r_prev"),                 # r_new == r_prev with another stride
              ({WS_BYTES: ws - 1}, b"workspace"), ({WS_BYTES: 0}, b"workspace"),
              ({ROWS: 5, WS_BYTES: ws}, b"workspace")]           # five rows: a second workgroup's partials
    for change, word in cases:
        args = list(good)
        for k, v in change.items():
            args[k] = v
        assert lib.fino_magcache_calibrate(*args) == -1, (change, word)
        err = lib.fino_last_error()
        assert word in err and err.startswith(b"fino_magcache_calibrate"), (change, err)


def test_the_op_checks_its_arguments_before_the_library():
    from frameino_amd import ops
    x = torch.zeros(4, 8, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.magcache_calibrate(x, x, x, x, torch.zeros(2, dtype=torch.float64))
