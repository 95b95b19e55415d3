"""MagCache in the FrameINO Wan loop (the tiny golden pipeline of tests/test_taylorseer_pipeline_gpu.py): a 6-step call on curves
that skip runs eagerly, logs the rule's trace per context, gives finite latents that differ from the uncached ones, and the three
CFG execution forms agree; the graph loop is refused; the state is dropped at the end of a call; a calibrating call returns the
uncached latents bit for bit and files one curve per context; a call whose step count is not the config's warns."""
import pytest
import torch

from frameino_amd.step_cache import MAG_FRESH, MagCacheConfig, magcache_curve, magcache_decide
from tests.test_taylorseer_pipeline_gpu import _run
from tests.test_wan_pipeline_gpu import _pipe

pytestmark = pytest.mark.gpu
STEPS = 6
# R = int(0.2 * 6 + 0.5) = 1.  "cond": the error stays 0 and max_skip_steps = 2 binds, C S S C S S; "uncond": 0.03, then
# 0.0891 > 0.06, C S C S C S -- so some steps of the batched call skip one element and compute the other
CURVES = {"cond": [1.0] * STEPS, "uncond": [0.97] * STEPS}


def _config(**kw):
    return MagCacheConfig(**{"mag_ratios": CURVES, "num_inference_steps": STEPS, "max_skip_steps": 2, **kw})


def _trace(cfg, steps=STEPS):
    """the rule's trace of one call: per step "cond" then "uncond", as the loop runs them"""
    rows, st = [], {c: MAG_FRESH for c in ("cond", "uncond")}
    for s in range(steps):
        for ctx in ("cond", "uncond"):
            compute, st[ctx] = magcache_decide(s, st[ctx], cfg, magcache_curve(cfg, ctx))
            rows.append((ctx, s, compute, st[ctx][2], st[ctx][1]))
    return rows


def test_a_six_step_call_that_skips(golden):
    pipe, a = _pipe(golden)
    pipe.use_hip_graph = False
    plain = _run(pipe, a, STEPS)
    pipe.use_hip_graph = None
    cfg = _config()
    pipe.transformer.enable_cache(cfg)
    want = _trace(cfg)
    assert [e[2] for e in want if e[0] == "cond"] == [True, False, False, True, False, False]
    assert [e[2] for e in want if e[0] == "uncond"] == [True, False, True, False, True, False]
    forms = {}
    for name, batch_cfg, streams in (("batch_cfg", True, False), ("sequential", False, False), ("cfg_streams", False, True)):
        pipe.batch_cfg, pipe.cfg_streams = batch_cfg, streams
        forms[name] = (_run(pipe, a, STEPS), list(pipe.transformer.cache_log))
    pipe.batch_cfg, pipe.cfg_streams = True, False
    video, log = forms["batch_cfg"]
    assert log == want
    assert bool(torch.isfinite(video).all()) and video.shape == plain.shape and not torch.equal(video, plain)
    for name, (lat, lg) in forms.items():                      # batched CFG, two calls, two streams: equal latents and logs
        assert torch.equal(lat, video) and lg == log, name
    # a second call starts from fresh state and reproduces the first; the state is dropped at the end of __call__
    assert torch.equal(_run(pipe, a, STEPS), video) and pipe.transformer.cache_log == log
    pipe.maybe_free_model_hooks()
    assert pipe.transformer._step_cache_states == {} and pipe.transformer.cache_log == log
    # one captured step cannot contain it
    pipe.use_hip_graph = True
    with pytest.raises(RuntimeError, match="use_hip_graph=True with MagCache") as err:
        _run(pipe, a, STEPS)
    assert str(err.value) == str(pipe.transformer._step_cache_policy.capture_refusal())
    pipe.use_hip_graph = None
    pipe.transformer.disable_cache()
    pipe.use_hip_graph = False
    assert torch.equal(_run(pipe, a, STEPS), plain)


def test_a_calibrating_call_is_the_uncached_call_and_files_a_curve_per_context(golden):
    pipe, a = _pipe(golden)
    pipe.use_hip_graph = False
    plain = _run(pipe, a, STEPS)
    pipe.use_hip_graph = None
    tr = pipe.transformer
    tr.enable_cache(MagCacheConfig(calibrate=True, num_inference_steps=STEPS))
    assert torch.equal(_run(pipe, a, STEPS), plain)
    assert tr.cache_log == [(ctx, s, True, None, None) for s in range(STEPS) for ctx in ("cond", "uncond")]
    cal = tr.magcache_calibration
    assert sorted(cal) == ["cond", "uncond"]
    for ctx in cal:
        ratios, cos = cal[ctx]["mag_ratios"], cal[ctx]["cos_dist"]
        assert len(ratios) == len(cos) == STEPS and ratios[0] == 1.0 and cos[0] == 0.0
        assert all(0.0 < r < float("inf") for r in ratios) and all(-1e-6 <= c <= 2.0 + 1e-6 for c in cos)
    assert cal["cond"]["mag_ratios"][1:] != cal["uncond"]["mag_ratios"][1:]          # each context measured its own residuals
    pipe.maybe_free_model_hooks()
    assert tr._step_cache_states == {} and tr.magcache_calibration == cal
    # the curves go straight back in
    tr.disable_cache()
    cfg = MagCacheConfig(mag_ratios={c: cal[c]["mag_ratios"] for c in cal}, num_inference_steps=STEPS, threshold=0.5)
    tr.enable_cache(cfg)
    out = _run(pipe, a, STEPS)
    assert bool(torch.isfinite(out).all()) and tr.cache_log == _trace(cfg)


def test_a_mismatching_step_count_warns(golden):
    pipe, a = _pipe(golden)
    pipe.transformer.enable_cache(_config(mag_ratios=[1.0] * 4, num_inference_steps=4))
    with pytest.warns(UserWarning, match="runs 6 steps, the config says num_inference_steps=4"):
        out = _run(pipe, a, STEPS)
    assert bool(torch.isfinite(out).all())
    assert [e[1] for e in pipe.transformer.cache_log if e[0] == "cond"] == [0, 1, 2, 3, 0, 1]      # the context started over
