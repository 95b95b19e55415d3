"""MagCache on the Wan DiT (the tiny random model, geometry and helpers of tests/test_step_cache_wan_gpu.py) against the
cache-disabled forward and against the restatement in tests/magcache_ref.py (the oracle's blocks in bf16).  Tolerance of a
forward against the bf16 oracle: the one tests/test_step_cache_wan_gpu.py holds a skipped forward to against its restatement,
the one test_wan_model_gpu.py states, rel-RMS < 1.5e-2.  The decisions read the step counter and the curve alone, so no
difference between the HIP path and the oracle can flip one."""
import pytest
import torch

from frameino_amd.step_cache import MAG_FRESH, MagCacheConfig, magcache_curve, magcache_decide
from oracle import wan_dit as W
from tests import magcache_ref as R
from tests.parity import bf16_state_dict, hip_wan_model, rel_rms
from tests.test_step_cache_wan_gpu import CFG, DEV, TS

pytestmark = pytest.mark.gpu
BOUND = 1.5e-2
C, K = True, False


def _inputs(scale):
    """the weights, latents and text of tests/test_step_cache_wan_gpu.py, every block's FFN output projection scaled by `scale`"""
    sd = W.wan_random_state_dict(CFG, seed=11, dtype=torch.float32, std=0.04)
    for k in sd:
        if ".ffn.net.2.weight" in k:
            sd[k] = sd[k] * scale
    g = torch.Generator().manual_seed(12)
    x = torch.randn(1, 16, 5, 16, 20, generator=g)
    dx = torch.randn(1, 16, 5, 16, 20, generator=g)
    txt = torch.randn(1, 77, 256, generator=g)
    return sd, bf16_state_dict(sd), x, dx, txt


RULE = dict(retention_ratio=0.0, max_skip_steps=2)              # with ratios of 1.0: C S S C S S C


@pytest.fixture(scope="module")
def setup():
    """inputs on which the restatement's skipping forward of a different latent and its uncached forward of that latent differ
    by at least 5 x BOUND (on the CPU, the restatement alone): otherwise no assertion below could tell a re-used residual
    from a computed one.  The weights are scaled until they do.  -> also the restatement's outputs, computed once"""
    for scale in (1.0, 2.0, 4.0):
        sd, sdb, x, dx, txt = _inputs(scale)
        ref = R.MagCacheRef(sdb, CFG, [1.0] * 8, 8, **RULE)
        computed = ref("c", x.bfloat16(), TS, txt.bfloat16())
        skipped = ref("c", dx.bfloat16(), TS, txt.bfloat16())          # another latent, x's residual
        uncached = ref.uncached(dx.bfloat16(), TS, txt.bfloat16())
        gap = rel_rms(skipped, uncached)
        print(f"restatement: skipping vs uncached forward rel-RMS {gap:.3e} at FFN scale {scale} (needs >= {5 * BOUND:.3e})")
        if gap >= 5 * BOUND:
            assert [e[2] for e in ref.log] == [C, K]
            return sd, sdb, x, dx, txt, dict(computed=computed, skipped=skipped, uncached=uncached, gap=gap)
    raise AssertionError(f"no scale separates the skipping forward from the uncached one: last gap {gap}")


def _model(sd, **cfg):
    m = hip_wan_model(CFG, sd, DEV)
    if cfg:
        cfg.setdefault("num_inference_steps", 8)
        if not cfg.get("calibrate"):
            cfg.setdefault("mag_ratios", [1.0] * cfg["num_inference_steps"])
        m.enable_cache(MagCacheConfig(**cfg))
    return m


def _fwd(m, ctx, x, txt, ts=TS, **kw):
    """tests/test_step_cache_wan_gpu.py's `_fwd`, plus keyword arguments of the forward"""
    with m.cache_context(ctx):
        return m(x.to(DEV).bfloat16(), ts.to(DEV), txt.to(DEV).bfloat16(), return_dict=False, **kw)[0]


def test_retention_one_never_skips_and_equals_the_uncached_forward(setup):
    sd, _, x, dx, txt, _ = setup
    plain, cached = _model(sd), _model(sd, retention_ratio=1.0, num_inference_steps=3)
    for i, ts in enumerate((811.0, 700.0, 650.0, 600.0)):           # the fourth forward: the context has started over
        xi, t = x + 0.1 * i * dx, torch.tensor([ts])
        assert torch.equal(_fwd(cached, "c", xi, txt, t), _fwd(plain, "c", xi, txt, t))
    assert [e[:3] for e in cached.cache_log] == [("c", 0, C), ("c", 1, C), ("c", 2, C), ("c", 0, C)]


def test_the_log_follows_the_rule(setup):
    sd, _, x, dx, txt, _ = setup
    m = _model(sd, **RULE)
    for i in range(7):
        out = _fwd(m, "c", x + 0.1 * i * dx, txt)
        assert bool(torch.isfinite(out).all())
    assert [e[2] for e in m.cache_log] == [C, K, K, C, K, K, C]
    assert [(e[0], e[1], e[4]) for e in m.cache_log] == [("c", s, k) for s, k in enumerate([0, 1, 2, 0, 1, 2, 0])]
    assert all(e[3] == 0.0 for e in m.cache_log)                 # ratios of exactly 1.0: no error accumulates, the count binds


def test_a_skipping_forward_of_another_latent_matches_the_restatement(setup):
    """... and is NOT the uncached forward of that latent: it carries the other latent's residual"""
    sd, _, x, dx, txt, want = setup
    assert want["gap"] >= 5 * BOUND
    m = _model(sd, **RULE)
    out = _fwd(m, "c", x, txt)
    err0 = rel_rms(out, want["computed"])
    out = _fwd(m, "c", dx, txt)
    err, far = rel_rms(out, want["skipped"]), rel_rms(out, want["uncached"])
    print(f"computing forward: rel-RMS {err0:.3e}; skipping forward: {err:.3e} against the restatement, {far:.3e} against the "
          f"uncached restatement (gap {want['gap']:.3e})")
    assert [e[2] for e in m.cache_log] == [C, K]
    assert err0 < BOUND and err < BOUND
    assert far > 3 * BOUND                                       # (and so it did not run the stack)


def test_a_skipping_forward_of_the_same_inputs_repeats_the_computing_one(setup):
    """x_in + (x_out - x_in) rounds twice in bf16: within the bound of the computing forward's output, not bit-equal"""
    sd, _, x, _, txt, _ = setup
    m = _model(sd, **RULE)
    first = _fwd(m, "c", x, txt).clone()
    second = _fwd(m, "c", x, txt)
    err = rel_rms(second, first)
    print(f"skipping forward on the same inputs: rel-RMS {err:.3e} against the computing forward")
    assert [e[2] for e in m.cache_log] == [C, K] and err < BOUND


def test_contexts_are_independent_with_a_curve_each(setup):
    """"cond" skips on its flat curve, "uncond" computes on its steep one: a batch of 2 under ("cond", "uncond") gives, row by
    row, what the two batch-1 calls give -- the stack runs on all rows and the skipping element's rows are overwritten"""
    sd, _, x, dx, txt, _ = setup
    curves = {"cond": [1.0] * 8, "uncond": [0.5] * 8}
    seq, bat = (_model(sd, mag_ratios=curves, **RULE) for _ in range(2))
    t2 = torch.cat([txt, txt.flip(1)])
    for i in range(3):
        xi = x + 0.3 * i * dx
        want = torch.cat([_fwd(seq, "cond", xi, t2[:1]), _fwd(seq, "uncond", xi, t2[1:])])
        got = _fwd(bat, "cfg", xi.expand(2, -1, -1, -1, -1), t2, _cache_contexts=("cond", "uncond"))
        assert torch.equal(got, want), i
    assert bat.cache_log == seq.cache_log
    assert [e[2] for e in bat.cache_log if e[0] == "cond"] == [C, K, K]
    assert [e[2] for e in bat.cache_log if e[0] == "uncond"] == [C, C, C]
    # an unnamed context takes the "cond" curve; without one it raises, before the forward counts
    m = _model(sd, mag_ratios={"uncond": [1.0] * 8}, **RULE)
    with pytest.raises(ValueError, match="no \"cond\" entry"):
        _fwd(m, "c", x, txt)
    assert list(m.cache_log) == []
    with pytest.raises(ValueError, match="No context is set"):
        m(x.to(DEV).bfloat16(), TS.to(DEV), txt.to(DEV).bfloat16(), return_dict=False)


def test_calibrate_mode(setup):
    sd, _, x, dx, txt, _ = setup
    plain, cal = _model(sd), _model(sd, calibrate=True, num_inference_steps=4)
    probe = _model(sd, calibrate=True, num_inference_steps=8)    # the same forwards, its state still there after the fourth
    lat = [x + 0.25 * i * dx for i in range(4)]
    res = []
    for i, xi in enumerate(lat):
        assert cal.magcache_calibration is None                  # nothing is read before the context starts over
        assert torch.equal(_fwd(cal, "cond", xi, txt), _fwd(plain, "cond", xi, txt))      # bit for bit the uncached forward
        _fwd(probe, "cond", xi, txt)
        res.append(probe._step_cache_states["cond"].residual.cpu())                      # the stored residual, in bf16
    assert cal.cache_log == [("cond", s, True, None, None) for s in range(4)]
    curve = cal.magcache_calibration["cond"]
    assert len(curve["mag_ratios"]) == len(curve["cos_dist"]) == 4 and curve["mag_ratios"][0] == 1.0 and curve["cos_dist"][0] == 0.0
    for s in range(1, 4):
        ratio, cos = R.calibration(res[s], res[s - 1])
        print(f"step {s}: ratio {curve['mag_ratios'][s]:.9f} (restatement {ratio:.9f}), cos_dist {curve['cos_dist'][s]:.3e} ({cos:.3e})")
        assert abs(curve["mag_ratios"][s] - ratio) <= 1e-5 * ratio
    # the calibrated curve fed back in: the log the model writes is the rule's trace on that curve
    cfg = MagCacheConfig(mag_ratios={"cond": curve["mag_ratios"]}, num_inference_steps=4, retention_ratio=0.25, threshold=0.5)
    m = hip_wan_model(CFG, sd, DEV)
    m.enable_cache(cfg)
    for xi in lat:
        _fwd(m, "cond", xi, txt)
    want, st = [], MAG_FRESH
    for s in range(4):
        compute, st = magcache_decide(s, st, cfg, magcache_curve(cfg, "cond"))
        want.append(("cond", s, compute, st[2], st[1]))
    assert m.cache_log == want


def test_mxfp8_linears_at_retention_one_equal_mxfp8_without_the_cache(setup):
    sd, _, x, dx, txt, _ = setup
    plain = _model(sd).enable_mxfp8_linears()
    cached = _model(sd, retention_ratio=1.0).enable_mxfp8_linears()
    for i in range(2):
        assert torch.equal(_fwd(cached, "c", x + 0.2 * i * dx, txt), _fwd(plain, "c", x + 0.2 * i * dx, txt))
    assert [e[2] for e in cached.cache_log] == [C, C]
