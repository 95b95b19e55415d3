"""TeaCache without a GPU: the rule (`teacache_decide`) against its restatement in exact arithmetic (tests/teacache_ref.py), the
config with its validation, per-context polynomials, fitting and persistence, the model's surface, a whole forward over a
stand-in for `ops` (tests/cpu_ops.py plus the two entries TeaCache calls, in plain torch) with its log and its host reads, the
pipeline's limits, and the C ABI's new symbols with their argument checks."""
import json
import math
import random
import warnings
from fractions import Fraction

import pytest
import torch

from frameino_amd import _lib
from frameino_amd import step_cache as S
from frameino_amd.step_cache import (FirstBlockCacheConfig, MagCacheConfig, TeaCacheConfig, fit_teacache_coefficients,
                                     load_teacache, save_teacache, teacache_decide)
from oracle import wan_dit as W
from tests import cpu_ops
from tests import teacache_ref as R
from tests.test_step_cache_cpu import _model, _pipe

C, K = True, False              # computes / skips
NAN, INF = float("nan"), float("inf")


def _trace(ds, cfg, context="cond"):
    """the model-independent fold of `teacache_decide` over consecutive forwards of one context, wrapping at N"""
    out, s, st = [], 0, S.TEA_FRESH
    for d in ds:
        compute, st = teacache_decide(s, st, cfg, d, context)
        out.append((s, compute, st[0]))
        s += 1
        if s == cfg.num_inference_steps:
            s, st = 0, S.TEA_FRESH
    return out


# ------------------------------------------------------------------ the rule
def test_the_worked_example():
    cfg = TeaCacheConfig(coefficients=[1.0, 0.0], num_inference_steps=6, rel_l1_thresh=0.2)
    got = _trace([None, 0.0625, 0.0625, 0.0625, 0.125, 0.5], cfg)
    # 1/16, 2/16, 3/16 stay under 0.2; 3/16 + 1/8 does not; the last step always computes
    assert got == [(0, C, 0.0), (1, K, 0.0625), (2, K, 0.125), (3, K, 0.1875), (4, C, 0.0), (5, C, 0.0)]
    assert S.teacache_cutoff(cfg) == 5 and S.teacache_poly([2.0, -1.0, 0.5], 0.5) == 0.5


def _draw(rng, n_forwards, degree):
    ds = [rng.randrange(0, 513) / 1024 for _ in range(n_forwards)]
    coef = [rng.randrange(-128, 129) / 64 for _ in range(degree + 1)]
    return ds, coef


RULES = [dict(), dict(ret_steps=0), dict(ret_steps=3), dict(cutoff_steps=5), dict(cutoff_steps=0), dict(max_skip_steps=1),
         dict(max_skip_steps=2, rel_l1_thresh=1.0), dict(max_skip_steps=0), dict(rel_l1_thresh=0.0), dict(rel_l1_thresh=0.75),
         dict(ret_steps=2, cutoff_steps=9, max_skip_steps=3, rel_l1_thresh=0.5), dict(calibrate=True)]


@pytest.mark.parametrize("rule", RULES, ids=lambda r: "-".join(f"{k}={v}" for k, v in r.items()) or "defaults")
def test_the_rule_against_exact_arithmetic(rule):
    """every d a multiple of 2^-10 in [0, 0.5], every coefficient a multiple of 2^-6 in [-2, 2], degree <= 4: every Horner
    value is a multiple of 2^-46 below 2^4 and every accumulated sum one below 2^6, so the fp64 arithmetic is exact and
    EVERY decision and EVERY acc must equal the Fractions'"""
    rng = random.Random(100 + RULES.index(rule))
    skipped = computed_by_acc = 0
    for case in range(40):
        n, degree = rng.choice([6, 11, 12]), case % 5
        forwards = 2 * n + 3                                        # past the start-over at N, twice
        ds, coef = _draw(rng, forwards, degree)
        if case % 4 == 0:                                           # small non-negative polynomials: runs of skips
            coef = [abs(c) / 8 for c in coef]
        if case % 7 == 3:
            ds[rng.randrange(forwards)] = NAN
            ds[rng.randrange(forwards)] = INF
        cfg = TeaCacheConfig(coefficients=coef, num_inference_steps=n, **rule)
        got = _trace(ds, cfg)
        want = R.rule_trace(ds, n, coef, **rule)
        assert [(s, c) for s, c, _ in got] == [(s, c) for s, c, _, _ in want], (case, coef, ds)
        assert all(Fraction(a[2]) == b[2] for a, b in zip(got, want)), (case, coef, ds)
        assert [s for s, _, _ in got] == [i % n for i in range(forwards)]       # the start-over at N
        skipped += sum(not c for _, c, _ in got)
        computed_by_acc += sum(c and m for (_, c, _), (_, _, _, m) in zip(got, want))
    if rule.get("calibrate") or rule.get("max_skip_steps") == 0 or rule.get("cutoff_steps") == 0:
        assert skipped == 0
    else:                                                           # (a threshold of 0 still skips under a negative acc)
        assert skipped > 20 and computed_by_acc > 20                # both branches of the comparison were exercised


def test_the_edges_of_the_rule():
    cfg = TeaCacheConfig(coefficients=[1.0, 0.0], num_inference_steps=10, rel_l1_thresh=0.25, max_skip_steps=2)
    # the cap binds: two skips in a row, then a compute although acc is small
    assert [c for _, c, _ in _trace([None] + [0.03125] * 8 + [None], cfg)] == [C, K, K, C, K, K, C, K, K, C]
    # a NaN or inf distance computes and resets; so does a negative polynomial's acc never reach the threshold
    assert teacache_decide(3, (0.1, 1, True), cfg, NAN) == (True, (0.0, 0, True))
    assert teacache_decide(3, (0.1, 1, True), cfg, INF) == (True, (0.0, 0, True))
    assert teacache_decide(3, (0.1, 1, True), cfg, 0.125) == (False, (0.225, 2, True))
    assert teacache_decide(3, (0.1, 2, True), cfg, 0.125) == (True, (0.0, 0, True))         # the cap
    assert teacache_decide(3, (0.125, 0, True), cfg, 0.125) == (True, (0.0, 0, True))       # acc == thresh is no skip
    # no plane or residual yet, the first `ret_steps`, from the cutoff on, calibrate: compute whatever d says
    assert teacache_decide(3, (0.0, 0, False), cfg, 0.0) == (True, (0.0, 0, True))
    assert teacache_decide(0, (0.0, 0, True), cfg, 0.0) == (True, (0.0, 0, True))
    assert teacache_decide(9, (0.0, 0, True), cfg, 0.0) == (True, (0.0, 0, True))
    assert teacache_decide(8, (0.0, 0, True), cfg, 0.0) == (False, (0.0, 1, True))
    cal = TeaCacheConfig(calibrate=True)
    assert teacache_decide(20, (0.1, 1, True), cal, 0.0) == (True, (0.0, 0, True))
    assert S.teacache_unconditional(20, (0.1, 1, True), cal) and not S.teacache_unconditional(8, (0.0, 0, True), cfg)
    assert S.teacache_unconditional(9, (0.0, 0, True), cfg) and S.teacache_unconditional(5, (0.0, 0, False), cfg)


# ------------------------------------------------------------------ config
def test_config_defaults():
    c = TeaCacheConfig(calibrate=True)
    assert (c.rel_l1_thresh, c.coefficients, c.num_inference_steps, c.ret_steps, c.cutoff_steps, c.max_skip_steps) == (
        0.2, None, 50, 1, None, None)
    assert TeaCacheConfig().calibrate is False


@pytest.mark.parametrize("bad", [dict(rel_l1_thresh=-0.1), dict(rel_l1_thresh=NAN), dict(rel_l1_thresh=INF), dict(rel_l1_thresh="x"),
                                 dict(rel_l1_thresh=True), dict(num_inference_steps=0), dict(num_inference_steps=2.0),
                                 dict(ret_steps=-1), dict(ret_steps=None), dict(ret_steps=1.5), dict(cutoff_steps=-1),
                                 dict(cutoff_steps=2.5), dict(max_skip_steps=-1), dict(max_skip_steps=True),
                                 dict(coefficients=[]), dict(coefficients=[1.0] * 9), dict(coefficients=[NAN]),
                                 dict(coefficients=[1.0, INF]), dict(coefficients=["a"]), dict(coefficients=3.0),
                                 dict(coefficients={"cond": []}), dict(coefficients={})],
                         ids=lambda b: "-".join(f"{k}={v}" for k, v in b.items()))
def test_bad_values_raise_and_name_the_field(bad):
    m = _model()
    kw = dict(coefficients=[1.0, 0.0], num_inference_steps=4)
    kw.update(bad)
    with pytest.raises(ValueError, match=next(iter(bad))):
        m.enable_cache(TeaCacheConfig(**kw))
    assert not m.is_cache_enabled


def test_no_coefficients_and_no_calibration_says_how_to_calibrate():
    m = _model()
    with pytest.raises(ValueError, match="calibrate=True.*fit_teacache_coefficients"):
        m.enable_cache(TeaCacheConfig())
    assert not m.is_cache_enabled
    m.enable_cache(TeaCacheConfig(calibrate=True))            # a calibrating run needs no polynomial
    assert m.is_cache_enabled and m._tea_on and not m._mag_on


def test_a_mapping_gives_every_context_its_polynomial():
    a, b = [1.0, 0.0], [0.5, 0.25, 0.0]
    cfg = TeaCacheConfig(coefficients={"cond": a, "uncond": b}, num_inference_steps=3)
    assert S.teacache_coefficients(cfg, "cond") == a and S.teacache_coefficients(cfg, "uncond") == b
    assert S.teacache_coefficients(cfg, "cfg") == a and S.teacache_coefficients(cfg, None) == a       # unnamed: the "cond" entry
    assert S.teacache_coefficients(TeaCacheConfig(coefficients=torch.tensor(b, dtype=torch.float64)), "x") == b
    assert S.teacache_coefficients(TeaCacheConfig(calibrate=True), "cond") is None
    assert teacache_decide(1, (0.0, 0, True), cfg, 0.25, "uncond")[1][0] == 0.5 * 0.0625 + 0.25 * 0.25
    assert teacache_decide(1, (0.0, 0, True), cfg, 0.125, "other")[1][0] == 0.125
    with pytest.raises(ValueError, match="no \"cond\" entry"):
        S.teacache_coefficients(TeaCacheConfig(coefficients={"uncond": b}), "cfg")
    m = _model()
    m.enable_cache(TeaCacheConfig(coefficients={"uncond": b}, num_inference_steps=3))
    with m.cache_context("c"), pytest.raises(ValueError, match="no polynomial for context 'c'"):
        m._teacache_begin(1, 4, 8, torch.bfloat16, "cpu")
    assert m.cache_log == () or m.cache_log == []                # refused before the forward counted


def test_a_duck_typed_config_is_accepted_and_a_bare_name_is_not():
    class TeaCacheConfig:                                        # noqa: F811  another library's class of that name
        def __init__(self):
            self.rel_l1_thresh, self.coefficients, self.num_inference_steps = 0.3, [1.0, 0.0], 10

    m = _model()
    m.enable_cache(TeaCacheConfig())                             # the other fields take this project's defaults
    assert m.is_cache_enabled and m._tea_on
    m.disable_cache()

    class Bare:
        pass
    Bare.__name__ = "TeaCacheConfig"
    with pytest.raises(NotImplementedError, match="TeaCacheConfig.*`rel_l1_thresh`.*`coefficients`"):
        m.enable_cache(Bare())
    assert not m.is_cache_enabled


def test_fit_recovers_a_known_quartic():
    want = [3.0, -2.5, 1.25, 0.5, 0.01]
    xs = [0.02 + 0.013 * i for i in range(23)]
    ys = [S.teacache_poly(want, x) for x in xs]
    # entry 0 of a run compares nothing
    run = {"cond": {"rel_l1_in": [None] + xs[:12], "rel_l1_out": [None] + ys[:12]}}
    more = {"cond": {"rel_l1_in": [None] + xs[12:], "rel_l1_out": [None] + ys[12:]},
            "uncond": {"rel_l1_in": [None] + xs, "rel_l1_out": [None] + [2 * y for y in ys]}}
    got = fit_teacache_coefficients([run, more], degree=4)       # two runs pooled per context
    assert set(got) == {"cond", "uncond"}
    assert all(abs(g - w) <= 1e-8 * abs(w) for g, w in zip(got["cond"], want)), got["cond"]
    assert all(abs(g - 2 * w) <= 1e-8 * abs(2 * w) for g, w in zip(got["uncond"], want)), got["uncond"]
    assert len(fit_teacache_coefficients(run, degree=1)["cond"]) == 2
    with pytest.raises(ValueError, match="needs more than 4"):
        fit_teacache_coefficients({"cond": {"rel_l1_in": [None, 0.1, 0.2], "rel_l1_out": [None, 0.1, 0.2]}})
    with pytest.raises(ValueError, match="degree"):
        fit_teacache_coefficients(run, degree=8)
    _model().enable_cache(TeaCacheConfig(coefficients=got, num_inference_steps=4))


def test_save_load_round_trip(tmp_path):
    coef = {"cond": [1.5, -0.25, 0.0078125], "uncond": [0.987654321, 0.0]}
    cal = {"cond": {"rel_l1_in": [None, 0.1, 0.2], "rel_l1_out": [None, 0.05, 0.3]}}
    path = tmp_path / "tea.json"
    save_teacache(path, coef, cal)
    assert load_teacache(path) == coef
    d = json.loads(path.read_text())
    assert d["format"] == "frameino_amd.teacache" and d["version"] == 1
    assert d["contexts"]["cond"]["rel_l1_in"] == [None, 0.1, 0.2] and d["contexts"]["cond"]["coefficients"] == coef["cond"]
    save_teacache(path, [2.0, 0.5])                              # one polynomial: the "cond" entry
    assert load_teacache(path) == {"cond": [2.0, 0.5]}
    _model().enable_cache(TeaCacheConfig(coefficients=load_teacache(path), num_inference_steps=2))
    xs = [0.05 * i for i in range(1, 9)]
    save_teacache(path, calibration={"cond": {"rel_l1_in": [None] + xs, "rel_l1_out": [None] + [2 * x for x in xs]}})
    fitted = load_teacache(path)["cond"]                         # measurements alone: fitted on loading
    assert len(fitted) == 5 and abs(fitted[3] - 2.0) < 1e-6 and abs(fitted[4]) < 1e-6
    for text in ('{"format": "frameino_amd.mag_ratios", "version": 1, "contexts": {}}', '{"contexts": {}}', "[1.0, 0.9]"):
        path.write_text(text)
        with pytest.raises(ValueError, match="not a file of save_teacache"):
            load_teacache(path)


# ------------------------------------------------------------------ surface
def _config(**kw):
    kw.setdefault("coefficients", [1.0, 0.0])
    kw.setdefault("num_inference_steps", 10)
    return TeaCacheConfig(**kw)


def test_exclusivity_and_disable_restores_the_model():
    m = _model()
    before = dict(vars(m))
    m.enable_cache(_config())
    assert m._step_cache_segments(1, 8) is None and m._magcache_begin(1, 4, 8, torch.bfloat16, "cpu") is None
    for other in (FirstBlockCacheConfig(), MagCacheConfig(calibrate=True), _config()):
        with pytest.raises(ValueError, match="already been enabled"):
            m.enable_cache(other)
    with m.cache_context("c"):
        plan = m._teacache_begin(1, 8, 8, torch.bfloat16, "cpu")
    assert m._step_cache_states and plan.segs[0].unconditional and plan.segs[0].compute is None and plan.segs[0].s == 0
    m.disable_cache()
    assert not m.is_cache_enabled and not m._tea_on and m._step_cache_states == {} and m._step_cache_config is None
    assert m._teacache_begin(1, 8, 8, torch.bfloat16, "cpu") is None
    after = dict(vars(m))
    for k in ("_step_cache_states", "_step_cache_log_fresh", "cache_log", "_step_cache_config"):
        before.pop(k, None), after.pop(k, None)
    assert after.keys() == before.keys() and all(after[k] is before[k] or after[k] == before[k] for k in before)
    m.enable_cache(FirstBlockCacheConfig())                    # ... and another cache can follow


def test_the_policy_and_its_refusals():
    from tests.test_taylorseer_cpu import _Shard, _first_next, _tiny_model
    from frameino_amd.attention_processor import MI355WanAttnProcessor
    from frameino_amd.window_attention import SparseAttentionConfig, WindowAttentionConfig
    policy = S._POLICIES["TeaCacheConfig"]
    assert policy is S._TeaCachePolicy and policy in S.StepCacheMixin._cache_policies
    assert policy not in S.PyramidAttentionBroadcastMixin._cache_policies and S._OTHER_DIFFUSERS_CONFIGS == ()
    assert policy.batched and not policy.reads_timestep_on_host
    assert not policy.hooks_attention(_config()) and policy.takes_windows(_config()) and policy.takes_fp8_attention(_config())
    assert "use_hip_graph=True with TeaCache" in str(policy.capture_refusal()) and policy.why_eager in str(policy.capture_refusal())
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
    m.parallel = _Shard()
    with pytest.raises(NotImplementedError, match="TeaCache with a token-sharded plan.*one GPU"):
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
    with pytest.raises(NotImplementedError, match="TeaCacheConfig.*PyramidAttentionBroadcastConfig is$"):
        m.enable_cache(_config())                                # the fully attributed config too
    assert not m.is_cache_enabled


# ------------------------------------------------------------------ a whole forward over stand-in ops
class _TeaOps:
    """tests/cpu_ops.py plus the two entries TeaCache calls, in plain torch; notes every call by name"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(cpu_ops, name)
        if not callable(fn):
            return fn

        def call(*a, **kw):
            self.calls.append(name)
            return fn(*a, **kw)
        return call

    def step_cache_residual(self, a, b, out=None, subtract=True):
        self.calls.append("residual_sub" if subtract else "residual_add")
        return out.copy_(a - b if subtract else a + b)

    def teacache_probe(self, x, plane, stats, shift=None, scale=None, sel=None, eps=1e-6, compare=True):
        self.calls.append(("probe" if shift is not None else "probe_plain") + ("" if compare else "_store"))
        m = x if shift is None else cpu_ops.adaln_modulate(x, shift, scale, sel, eps)
        stats.copy_(torch.tensor(R.sums(m, plane) if compare else (0.0, 0.0), dtype=torch.float64))
        return plane.copy_(m)


CFG = dict(W.WAN22_5B_CFG, num_attention_heads=2, attention_head_dim=64, in_channels=4, out_channels=4, text_dim=32, freq_dim=32,
           ffn_dim=64, num_layers=2)


def _setup(b=2, **cfg):
    from tests.parity import model_cfg
    from frameino_amd.transformer_wan import WanTransformer3DModel
    sd = W.wan_random_state_dict(CFG, seed=21, dtype=torch.float32, std=0.2)
    m = WanTransformer3DModel(**model_cfg(CFG))
    m.load_reference_state_dict(sd, dtype=torch.float32)
    m.eval()
    m.ops = _TeaOps()
    if cfg:
        m.enable_cache(TeaCacheConfig(**cfg))
    g = torch.Generator().manual_seed(22)
    base = torch.randn(b, 4, 3, 8, 10, generator=g)
    steps = [0.0, 0.02, 0.02, 0.02, 0.5, 0.02, 0.02, 0.02]        # how far every forward's latent moves from the previous one
    xs, x = [], base
    for step in steps:
        x = x + step * torch.randn(b, 4, 3, 8, 10, generator=g)
        xs.append(x)
    txt = torch.randn(b, 6, 32, generator=g)
    ts = torch.tensor([811.0, 650.0][:b])
    return sd, m, xs, txt, ts


class _Reads:
    """counts the device-to-host reads a forward makes through Tensor.tolist (the one way step_cache.py reads)"""

    def __enter__(self):
        self.n, self._orig = 0, torch.Tensor.tolist
        outer = self

        def tolist(t):
            outer.n += 1
            return outer._orig(t)
        torch.Tensor.tolist = tolist
        return self

    def __exit__(self, *exc):
        torch.Tensor.tolist = self._orig


def _fwd(m, x, ts, txt, ctxs=("cond", "uncond")):
    with m.cache_context("cfg"):
        return m(x, ts, txt, return_dict=False, _cache_contexts=ctxs[:x.shape[0]])[0]


def test_a_forward_logs_the_rule_reads_once_and_skips_the_stack():
    kw = dict(coefficients=[1.0, 0.0], num_inference_steps=8, rel_l1_thresh=0.12, max_skip_steps=2)
    sd, m, xs, txt, ts = _setup(**kw)
    plain = _setup()[1]
    outs, reads, calls = [], [], []
    for x in xs:
        m.ops.calls.clear()
        with _Reads() as r:
            outs.append(_fwd(m, x, ts, txt))
        reads.append(r.n)
        calls.append(list(m.ops.calls))
    log = {c: [e for e in m.cache_log if e[0] == c] for c in ("cond", "uncond")}
    for c in ("cond", "uncond"):
        assert [e[1] for e in log[c]] == list(range(8))
        assert log[c][0][3] is None and log[c][7][3] is None and all(e[3] is not None for e in log[c][1:7])
        # the log follows the rule: the restatement, fed the distances the model measured, decides and accumulates alike
        want = R.rule_trace([e[3] for e in log[c]], 8, kw["coefficients"], rel_l1_thresh=0.12, max_skip_steps=2)
        assert [(e[1], e[2]) for e in log[c]] == [(s, comp) for s, comp, _, _ in want]
        assert all(abs(Fraction(e[4]) - w[2]) < Fraction(1, 10 ** 12) for e, w in zip(log[c], want))
        # skips, a compute forced by the cap, one forced by the accumulated distance (the 0.5 move), the last step
        assert [e[2] for e in log[c]] == [C, K, K, C, C, K, K, C], log[c]
        assert log[c][3][4] == 0.0 and log[c][3][3] < 0.12 and log[c][4][3] > 0.12
    # one host read per forward for both contexts together; none where both compute unconditionally (first and last)
    assert reads == [0, 1, 1, 1, 1, 1, 1, 0]
    # a forward probes both segments before anything else of the stack; a skipping one runs no block at all
    for i, names in enumerate(calls):
        # (the first forward has no plane to compare with, the last one computes whatever it would measure)
        assert names.count("probe" if 0 < i < 7 else "probe_store") == 2 and names.count("probe_plain") == 0
        skipping = not log["cond"][i][2]
        assert ("attention" in names) == (not skipping)
        assert names.count("residual_add") == (2 if skipping else 0) and names.count("residual_sub") == (0 if skipping else 2)
        if skipping:
            assert names.count("gemm") == 2 and names.count("adaln_modulate") == 1      # the patch embedding and the head
    # a computing forward is the uncached forward; a skipping one is the head on h0 + r of the last computing forward
    for i in (0, 3, 4, 7):
        assert torch.equal(outs[i], plain(xs[i], ts, txt, return_dict=False)[0])
    ref = R.TeaCacheRef(sd, CFG, kw["coefficients"], 8, rel_l1_thresh=0.12, max_skip_steps=2)
    for i, x in enumerate(xs):
        for bi, c in enumerate(("cond", "uncond")):
            want = ref(c, x[bi:bi + 1], ts[bi:bi + 1], txt[bi:bi + 1])
            assert torch.allclose(outs[i][bi:bi + 1], want, rtol=1e-4, atol=1e-4), (i, c)
    assert [e[:3] for e in ref.log if e[0] == "cond"] == [e[:3] for e in log["cond"]]
    assert all(abs(a[3] - b[3]) <= 1e-4 * b[3] for a, b in zip(log["cond"][1:7], [e for e in ref.log if e[0] == "cond"][1:7]))
    assert m._step_cache_states == {}                            # both counters reached N = 8: both contexts started over


def test_mixed_decisions_overwrite_the_skipping_segment_alone():
    kw = dict(coefficients={"cond": [0.0], "uncond": [100.0]}, num_inference_steps=8)
    sd, m, xs, txt, ts = _setup(**kw)
    plain = _setup()[1]
    for i, x in enumerate(xs[:4]):
        m.ops.calls.clear()
        out = _fwd(m, x, ts, txt)
        want = plain(x, ts, txt, return_dict=False)[0]
        assert torch.equal(out[1], want[1])                          # "uncond" always computes
        assert torch.equal(out[0], want[0]) == (i == 0)
        if i:
            assert m.ops.calls.count("residual_add") == 1 and m.ops.calls.count("residual_sub") == 1
            assert "attention" in m.ops.calls                        # the stack ran, on all rows
    assert [e[2] for e in m.cache_log if e[0] == "cond"] == [C, K, K, K]
    assert [e[2] for e in m.cache_log if e[0] == "uncond"] == [C, C, C, C]


def test_calibrate_mode_computes_every_step_reads_nothing_and_files_once():
    sd, m, xs, txt, ts = _setup(calibrate=True, num_inference_steps=4)
    plain = _setup()[1]
    po = []
    for i in range(3):
        m.ops.calls.clear()
        with _Reads() as r:
            out = _fwd(m, xs[i], ts, txt)
        assert r.n == 0
        assert torch.equal(out, plain(xs[i], ts, txt, return_dict=False)[0])
        assert m.ops.calls.count("probe" if i else "probe_store") == 2
        assert m.ops.calls.count("probe_plain" if i else "probe_plain_store") == 2
        po.append(plain.ops and plain._ws)                       # (keeps the plain model's workspace alive)
    assert m.teacache_calibration is None                       # nothing is read before the context starts over
    with _Reads() as r:
        _fwd(m, xs[3], ts, txt)
    assert r.n == 2                                              # one read per context, when it starts over
    cal = m.teacache_calibration
    assert set(cal) == {"cond", "uncond"} and m._step_cache_states == {}
    assert m.cache_log == [(c, s, True, None, 0.0) for s in range(4) for c in ("cond", "uncond")]
    for c in ("cond", "uncond"):
        assert len(cal[c]["rel_l1_in"]) == len(cal[c]["rel_l1_out"]) == 4
        assert cal[c]["rel_l1_in"][0] is None and cal[c]["rel_l1_out"][0] is None
        assert all(0.0 < v < 1.0 for v in cal[c]["rel_l1_in"][1:] + cal[c]["rel_l1_out"][1:])
    # the restatement measures the same input distances
    ref = R.TeaCacheRef(sd, CFG, None, 4, calibrate=True)
    planes = []
    for x in xs[:4]:
        h0, temb, tproj, t2, rot, geo = __import__("tests.step_cache_ref", fromlist=["_embed"])._embed(sd, CFG, x[:1], ts[:1], txt[:1])
        planes.append(ref.probe(h0, tproj))
    want = [R.rel_l1(planes[i], planes[i - 1]) for i in range(1, 4)]
    assert all(abs(g - w) <= 1e-4 * w for g, w in zip(cal["cond"]["rel_l1_in"][1:], want))
    # a reset files what an unfinished context has recorded
    _fwd(m, xs[0][:1], ts[:1], txt[:1], ctxs=("extra",))
    _fwd(m, xs[1][:1], ts[:1], txt[:1], ctxs=("extra",))
    m._reset_stateful_cache()
    assert len(m.teacache_calibration["extra"]["rel_l1_in"]) == 2 and m.teacache_calibration["cond"] is cal["cond"]
    assert m.magcache_calibration is None                       # (MagCache's filing does not take these rows for its own)


def test_reset_and_other_rows_start_over():
    sd, m, xs, txt, ts = _setup(coefficients=[0.0], num_inference_steps=8)
    for x in xs[:3]:
        _fwd(m, x, ts, txt)
    assert [e[2] for e in m.cache_log if e[0] == "cond"] == [C, K, K]
    m._reset_stateful_cache()
    assert m._step_cache_states == {} and len(m.cache_log) == 6
    _fwd(m, xs[3], ts, txt)
    assert m.cache_log == [("cond", 0, C, None, 0.0), ("uncond", 0, C, None, 0.0)]
    _fwd(m, xs[4][:1], ts[:1], txt[:1], ctxs=("cond",))         # the same context, same rows: goes on
    assert m.cache_log[-1][:3] == ("cond", 1, K)
    with pytest.raises(ValueError, match="No context is set"):
        m._teacache_begin(1, 4, 8, torch.float32, "cpu")


# ------------------------------------------------------------------ the loop
def test_pipeline_limits_warning_and_reset():
    pipe = _pipe()
    tr = pipe.transformer
    tr.enable_cache(_config())
    assert pipe._step_cache_check(1) is True and pipe._step_cache_check(2) is True        # the eager loop; a batch is allowed
    pipe.use_hip_graph = True
    with pytest.raises(RuntimeError, match="use_hip_graph=True with TeaCache.*decided on the host"):
        pipe._step_cache_check(1)
    pipe.use_hip_graph = None
    pipe.parallel = object()
    with pytest.raises(NotImplementedError, match="TeaCache runs on one GPU"):
        pipe._step_cache_check(1)
    pipe.parallel = None
    with pytest.warns(UserWarning, match="TeaCache: this call runs 7 steps, the config says num_inference_steps=10"):
        S._TeaCachePolicy.loop_begins(tr._step_cache_config, 7)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        S._TeaCachePolicy.loop_begins(tr._step_cache_config, 10)
    with tr.cache_context("cond"):
        tr._teacache_begin(1, 4, 8, torch.bfloat16, "cpu")
    assert tr._step_cache_states
    pipe.maybe_free_model_hooks()
    assert tr._step_cache_states == {}


# ------------------------------------------------------------------ the C ABI
def test_the_new_symbols_are_declared_exported_and_bound():
    lib = _lib.lib()
    for name in ("fino_teacache_probe", "fino_teacache_workspace_bytes"):
        assert name in _lib.declared_symbols() and name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.fino_version() == 103 == _lib.ABI_VERSION
    assert len(_lib.SIGNATURES["fino_teacache_probe"]) == 17
    # one fp64 pair per wave; the wave count depends on the rows alone and is capped
    sizes = [lib.fino_teacache_workspace_bytes(r) for r in (0, 1, 4, 5, 1188, 24640, 2 ** 31 - 1)]
    assert sizes[0] == 0 and sizes[1] == sizes[2] == 4 * 16 and sizes[3] == 8 * 16 and sizes[4] == 1188 * 16
    assert sizes[5] == sizes[6] and sizes[5] % 16 == 0 and 24640 * 16 >= sizes[5] >= 4096 * 16


def test_the_c_abi_checks_before_any_launch():
    import ctypes
    lib = _lib.lib()
    a = 4096                                                      # any 16-byte aligned address: nothing is dereferenced
    ws = lib.fino_teacache_workspace_bytes(4)
    eps = ctypes.c_float(1e-6)
    good = [a, 8, 2 * a, 8, 4, 8, a, a, 8, a, eps, 1, 0, a, a, ws, 0]       # bf16 [4, 8]
    X, LDX, PLANE, LDP, ROWS, DIM, SHIFT, SCALE, MS, SEL, EPS_, COMPARE, DTYPE, STATS, WS, WS_BYTES = range(16)
    cases = [({p: 0}, b"null pointer") for p in (X, PLANE, STATS, WS)]
    cases += [({SHIFT: 0}, b"come together"), ({SCALE: 0}, b"come together"), ({SHIFT: 0, SCALE: 0}, b"selector needs"),
              ({DIM: 12, LDX: 16, LDP: 16}, b"dim=12"), ({DIM: 0}, b"dim=0"), ({DTYPE: 2}, b"dtype"), ({DTYPE: 3}, b"dtype"),
              ({ROWS: 0}, b"rows=0"), ({ROWS: 2 ** 31}, b"rows=2147483648"),
              ({LDX: 0}, b"row stride is below dim"), ({LDP: 0}, b"row stride is below dim"),
              ({X: a + 2}, b"alignment"), ({PLANE: a + 2}, b"alignment"), ({SHIFT: a + 4}, b"alignment"),
              ({SCALE: a + 4}, b"alignment"), ({STATS: a + 8}, b"alignment"), ({WS: a + 8}, b"alignment"),
              ({LDX: 12}, b"alignment"), ({MS: 6}, b"alignment"), ({PLANE: a}, b"the plane is x itself"),
              ({WS_BYTES: ws - 1}, b"workspace"), ({WS_BYTES: 0}, b"workspace"), ({ROWS: 5, WS_BYTES: ws}, b"workspace")]
    for change, word in cases:
        args = list(good)
        for k, v in change.items():
            args[k] = v
        assert lib.fino_teacache_probe(*args) == -1, (change, word)
        err = lib.fino_last_error()
        assert word in err and err.startswith(b"fino_teacache_probe"), (change, err)
    args = list(good)
    args[DIM], args[LDX], args[LDP], args[MS] = 4104, 4104, 4104, 4104
    assert lib.fino_teacache_probe(*args) == -3 and b"4096" in lib.fino_last_error()       # beyond eight passes: unsupported
    # the plain mode passes the same checks without modulation rows (rows = 0 is refused above: nothing here launches)
    args = list(good)
    args[SHIFT] = args[SCALE] = args[SEL] = 0
    args[WS_BYTES] = 0
    assert lib.fino_teacache_probe(*args) == -1 and b"workspace" in lib.fino_last_error()


def test_the_op_checks_its_arguments_before_the_library():
    from frameino_amd import ops
    x = torch.zeros(4, 8, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.teacache_probe(x, x.clone(), torch.zeros(2, dtype=torch.float64))
