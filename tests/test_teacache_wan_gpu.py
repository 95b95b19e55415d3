"""TeaCache on the Wan DiT (the tiny random model, geometry and helpers of tests/test_step_cache_wan_gpu.py) against the
cache-disabled forward and against the restatement in tests/teacache_ref.py (the oracle's blocks in bf16, built like
`MagCacheRef`).  Tolerance of a forward against the bf16 oracle: the one tests/test_step_cache_wan_gpu.py and
tests/test_magcache_wan_gpu.py state, rel-RMS < 1.5e-2.

The decisions depend on the data, so a test of decisions states a condition on its own inputs, checked on the CPU with the
restatement alone: every accumulated value the rule compares with the threshold lies outside [thresh / 2, 2 thresh].  The HIP
path's distance d and the restatement's differ by how the two patch embeddings round (D_DEVIATION below, a few 1e-4 relative),
which cannot move an accumulated value by a factor of two.

The logged d against the restatement's d.  Measured on the MI355X over the six compared forwards of
`test_the_log_has_skips_...`: the largest relative deviation is recorded with `record()` (the parity file the GPU suite
writes) on every run; it measured 1.284e-4 (distances of 0.0057 .. 0.75), and the assertion is four times that, D_DEVIATION = 5.2e-4 (the cap
would have been 5e-2)."""
import pytest
import torch

from frameino_amd.step_cache import TeaCacheConfig, fit_teacache_coefficients
from frameino_amd.window_attention import WindowAttentionConfig
from oracle import wan_dit as W
from tests import teacache_ref as R
from tests.parity import bf16_state_dict, hip_wan_model, record, rel_rms
from tests.test_step_cache_wan_gpu import CFG, DEV, TS

pytestmark = pytest.mark.gpu
BOUND = 1.5e-2
D_DEVIATION = 5.2e-4
C, K = True, False
THRESH = 0.2
STEPS = [0.0, 0.01, 0.01, 0.01, 1.0, 0.01, 0.01]                # how far each forward's latent moves from the previous one
RULE = dict(rel_l1_thresh=THRESH, max_skip_steps=2)


def _inputs(scale):
    """the weights, latents and text of tests/test_magcache_wan_gpu.py, every block's FFN output projection scaled by `scale`"""
    sd = W.wan_random_state_dict(CFG, seed=11, dtype=torch.float32, std=0.04)
    for k in sd:
        if ".ffn.net.2.weight" in k:
            sd[k] = sd[k] * scale
    g = torch.Generator().manual_seed(12)
    x = torch.randn(1, 16, 5, 16, 20, generator=g)
    dx = torch.randn(1, 16, 5, 16, 20, generator=g)
    txt = torch.randn(1, 77, 256, generator=g)
    return sd, bf16_state_dict(sd), x, dx, txt


def _latents(x, dx):
    out, pos = [], 0.0
    for step in STEPS:
        pos += step
        out.append(x + pos * dx)
    return out


@pytest.fixture(scope="module")
def setup():
    """inputs on which the restatement's skipping forward of a different latent and its uncached forward of that latent differ
    by at least 5 x BOUND (on the CPU, the restatement alone): otherwise no assertion could tell a re-used residual from a
    computed one.  The weights are scaled until they do.  -> also the restatement's outputs and its log of the latent
    sequence, computed once"""
    for scale in (1.0, 2.0, 4.0):
        sd, sdb, x, dx, txt = _inputs(scale)
        ref = R.TeaCacheRef(sdb, CFG, [0.0], 8)                       # the zero polynomial: every comparison skips
        computed = ref("c", x.bfloat16(), TS, txt.bfloat16())
        skipped = ref("c", dx.bfloat16(), TS, txt.bfloat16())         # another latent, x's residual
        uncached = ref.uncached(dx.bfloat16(), TS, txt.bfloat16())
        gap = rel_rms(skipped, uncached)
        print(f"restatement: skipping vs uncached forward rel-RMS {gap:.3e} at FFN scale {scale} (needs >= {5 * BOUND:.3e})")
        if gap >= 5 * BOUND:
            assert [e[2] for e in ref.log] == [C, K]
            seq = R.TeaCacheRef(sdb, CFG, [1.0, 0.0], 8, **RULE)      # the identity polynomial: acc accumulates d itself
            for xi in _latents(x, dx):
                seq("c", xi.bfloat16(), TS, txt.bfloat16())
            return sd, sdb, x, dx, txt, dict(computed=computed, skipped=skipped, uncached=uncached, gap=gap, log=seq.log,
                                             margins=seq.margins)
    raise AssertionError(f"no scale separates the skipping forward from the uncached one: last gap {gap}")


def _model(sd, **cfg):
    m = hip_wan_model(CFG, sd, DEV)
    if cfg:
        cfg.setdefault("num_inference_steps", 8)
        if not cfg.get("calibrate"):
            cfg.setdefault("coefficients", [1.0, 0.0])
        m.enable_cache(TeaCacheConfig(**cfg))
    return m


def _fwd(m, ctx, x, txt, ts=TS, **kw):
    with m.cache_context(ctx):
        return m(x.to(DEV).bfloat16(), ts.to(DEV), txt.to(DEV).bfloat16(), return_dict=False, **kw)[0]


def test_threshold_zero_never_skips_and_equals_the_uncached_forward(setup):
    sd, _, x, dx, txt, _ = setup
    plain, cached = _model(sd), _model(sd, rel_l1_thresh=0.0, num_inference_steps=3)
    for i, ts in enumerate((811.0, 700.0, 650.0, 600.0)):           # the fourth forward: the context has started over
        xi, t = x + 0.1 * i * dx, torch.tensor([ts])
        assert torch.equal(_fwd(cached, "c", xi, txt, t), _fwd(plain, "c", xi, txt, t))
    assert [e[:3] for e in cached.cache_log] == [("c", 0, C), ("c", 1, C), ("c", 2, C), ("c", 0, C)]
    assert cached.cache_log[1][3] > 0 and cached.cache_log[1][4] == 0.0 and cached.cache_log[0][3] is None


def test_the_log_has_skips_a_compute_by_accumulation_and_one_by_the_cap(setup):
    sd, _, x, dx, txt, want = setup
    # the condition on the inputs (CPU, the restatement alone): no compared acc within a factor of two of the threshold
    assert len(want["margins"]) == 6
    assert all(acc < thr / 2 or acc > 2 * thr for acc, thr in want["margins"]), [float(a) for a, _ in want["margins"]]
    assert [e[2] for e in want["log"]] == [C, K, K, C, C, K, K]
    big = [float(a) for a, _ in want["margins"]]
    assert big[2] < THRESH / 2 < 2 * THRESH < big[3]             # forward 3: the cap binds; forward 4: the accumulated distance
    m = _model(sd, **RULE)
    for xi in _latents(x, dx):
        assert bool(torch.isfinite(_fwd(m, "c", xi, txt)).all())
    assert [e[:3] for e in m.cache_log] == [e[:3] for e in want["log"]]
    dev = max(abs(a[3] - b[3]) / b[3] for a, b in zip(m.cache_log[1:], want["log"][1:]))
    print("logged d:", [e[3] for e in m.cache_log], "restatement:", [e[3] for e in want["log"]], f"largest deviation {dev:.3e}")
    record("teacache_wan", "logged_d_relative_deviation", dev, D_DEVIATION)
    assert dev <= D_DEVIATION
    assert all(abs(a[4] - float(b[4])) <= D_DEVIATION * THRESH for a, b in zip(m.cache_log, want["log"]))


def test_a_skipping_forward_of_another_latent_matches_the_restatement(setup):
    """... and is NOT the uncached forward of that latent: it carries the other latent's residual"""
    sd, _, x, dx, txt, want = setup
    assert want["gap"] >= 5 * BOUND
    m = _model(sd, coefficients=[0.0])
    out = _fwd(m, "c", x, txt)
    err0 = rel_rms(out, want["computed"])
    out = _fwd(m, "c", dx, txt)
    err, far = rel_rms(out, want["skipped"]), rel_rms(out, want["uncached"])
    print(f"computing forward: rel-RMS {err0:.3e}; skipping forward: {err:.3e} against the restatement, {far:.3e} against the "
          f"uncached restatement (gap {want['gap']:.3e})")
    assert [e[2] for e in m.cache_log] == [C, K] and m.cache_log[1][3] > 0.5 and m.cache_log[1][4] == 0.0
    assert err0 < BOUND and err < BOUND
    assert far > 3 * BOUND                                       # (and so it did not run the stack)


def test_a_batched_call_is_two_sequential_calls(setup):
    sd, _, x, dx, txt, _ = setup
    seq, bat = (_model(sd, **RULE) for _ in range(2))
    t2 = torch.cat([txt, txt.flip(1)])
    for xi in _latents(x, dx)[:5]:
        want = torch.cat([_fwd(seq, "cond", xi, t2[:1]), _fwd(seq, "uncond", xi, t2[1:])])
        got = _fwd(bat, "cfg", xi.expand(2, -1, -1, -1, -1), t2, _cache_contexts=("cond", "uncond"))
        assert rel_rms(got, want) < BOUND
    assert [e[:3] for e in bat.cache_log] == [e[:3] for e in seq.cache_log]
    assert [e[2] for e in bat.cache_log if e[0] == "cond"] == [C, K, K, C, C]
    for a, b in zip(bat.cache_log, seq.cache_log):               # the same rows through the same probe: the same distances
        assert (a[3] is None and b[3] is None) or abs(a[3] - b[3]) <= D_DEVIATION * b[3]
    with pytest.raises(ValueError, match="No context is set"):
        bat(x.to(DEV).bfloat16(), TS.to(DEV), txt.to(DEV).bfloat16(), return_dict=False)


def test_mixed_decisions_in_one_batched_call(setup):
    """a zero polynomial against a large constant: "cond" skips, "uncond" computes -- the stack runs on all rows and the
    skipping element's rows are overwritten"""
    sd, _, x, dx, txt, _ = setup
    coef = {"cond": [0.0], "uncond": [100.0]}
    seq, bat, plain = _model(sd, coefficients=coef), _model(sd, coefficients=coef), _model(sd)
    t2 = torch.cat([txt, txt.flip(1)])
    for i in range(3):
        xi = x + 0.3 * i * dx
        want = torch.cat([_fwd(seq, "cond", xi, t2[:1]), _fwd(seq, "uncond", xi, t2[1:])])
        got = _fwd(bat, "cfg", xi.expand(2, -1, -1, -1, -1), t2, _cache_contexts=("cond", "uncond"))
        assert rel_rms(got, want) < BOUND, i
        assert torch.equal(got[1:], _fwd(plain, "c", xi, t2[1:]))                  # the computing element: the uncached forward
        if i:
            assert rel_rms(got[:1], _fwd(plain, "c", xi, t2[:1])) > 1e-3             # the skipping one is not
    assert [e[2] for e in bat.cache_log if e[0] == "cond"] == [C, K, K]
    assert [e[2] for e in bat.cache_log if e[0] == "uncond"] == [C, C, C]
    m = _model(sd, coefficients={"uncond": [0.0]})
    with pytest.raises(ValueError, match="no \"cond\" entry"):
        _fwd(m, "c", x, txt)
    assert list(m.cache_log) == []


def test_calibrate_mode(setup):
    sd, sdb, x, dx, txt, _ = setup
    n = 6
    plain, cal = _model(sd), _model(sd, calibrate=True, num_inference_steps=n)
    lat = [x + 0.05 * i * i * dx for i in range(n)]              # growing steps: distinct distances to fit
    for xi in lat:
        assert cal.teacache_calibration is None                  # nothing is read before the contexts start over
        got = _fwd(cal, "cfg", xi.expand(2, -1, -1, -1, -1), torch.cat([txt, txt]), _cache_contexts=("cond", "uncond"))
        assert torch.equal(got[:1], _fwd(plain, "c", xi, txt))                      # bit for bit the uncached forward
    assert cal.cache_log == [(c, s, True, None, 0.0) for s in range(n) for c in ("cond", "uncond")]
    curves = cal.teacache_calibration
    assert set(curves) == {"cond", "uncond"}
    ref = R.TeaCacheRef(sdb, CFG, None, n, calibrate=True)
    from tests.step_cache_ref import _embed
    planes = []
    for xi in lat:
        h0, _, tproj, _, _, _ = _embed(sdb, CFG, xi.bfloat16(), TS, txt.bfloat16())
        planes.append(ref.probe(h0, tproj))
    for c in ("cond", "uncond"):
        cin, cout = curves[c]["rel_l1_in"], curves[c]["rel_l1_out"]
        assert len(cin) == len(cout) == n and cin[0] is None and cout[0] is None
        assert all(v > 0 for v in cin[1:] + cout[1:])
        for s in range(1, n):
            want = R.rel_l1(planes[s], planes[s - 1])
            print(f"{c} step {s}: rel_l1_in {cin[s]:.6f} (restatement {want:.6f}), rel_l1_out {cout[s]:.6f}")
            assert abs(cin[s] - want) <= D_DEVIATION * want
    # the fitted polynomial fed back in: it can be enabled and run, and the log is the rule's trace on the distances it logged
    coef = fit_teacache_coefficients(curves, degree=2)
    cfg = dict(coefficients=coef, num_inference_steps=n, rel_l1_thresh=0.3)
    m = _model(sd, **cfg)
    for xi in lat:
        assert bool(torch.isfinite(_fwd(m, "cond", xi, txt)).all())
    trace = R.rule_trace([e[3] for e in m.cache_log], n, coef["cond"], rel_l1_thresh=0.3)
    assert [(e[1], e[2]) for e in m.cache_log] == [(s, comp) for s, comp, _, _ in trace]


def test_starting_over_after_n_forwards_and_reset(setup):
    sd, _, x, dx, txt, _ = setup
    m = _model(sd, coefficients=[0.0], num_inference_steps=4)
    for i in range(6):
        _fwd(m, "c", x + 0.1 * i * dx, txt)
    # forward 3 is the last of its four and computes; the context starts over: forward 0 again has nothing to compare with
    assert [(e[1], e[2]) for e in m.cache_log] == [(0, C), (1, K), (2, K), (3, C), (0, C), (1, K)]
    assert m.cache_log[4][3] is None and m.cache_log[5][3] is not None
    m._reset_stateful_cache()
    assert m._step_cache_states == {}
    _fwd(m, "c", x, txt)
    assert m.cache_log == [("c", 0, C, None, 0.0)]


@pytest.mark.parametrize("feature", ["fp8_attention", "window_attention", "mxfp8_linears"])
def test_it_runs_beside(setup, feature):
    sd, _, x, dx, txt, _ = setup
    m = _model(sd, coefficients=[0.0])
    if feature == "fp8_attention":
        m.enable_fp8_attention(True)
    elif feature == "window_attention":
        m.enable_window_attention(WindowAttentionConfig(1))
    else:
        m.enable_mxfp8_linears()
    for i in range(3):
        assert bool(torch.isfinite(_fwd(m, "c", x + 0.1 * i * dx, txt)).all())
    assert [e[2] for e in m.cache_log] == [C, K, K] and all(e[3] > 0 for e in m.cache_log[1:])
