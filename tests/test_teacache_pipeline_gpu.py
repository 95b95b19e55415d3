"""TeaCache in the FrameINO Wan loop (the tiny golden pipeline of tests/test_magcache_pipeline_gpu.py): at threshold 0 a 6-step
call gives the latents of the plain eager call bit for bit; a config that skips runs eagerly, gives finite latents that differ
from the uncached ones and a log with skips, from fresh state per call and per sample of a batch; the graph loop is refused; a
call whose step count is not the config's warns."""
import pytest
import torch

from frameino_amd.step_cache import TeaCacheConfig
from tests.test_taylorseer_pipeline_gpu import DEV, _run
from tests.test_wan_pipeline_gpu import _pipe

pytestmark = pytest.mark.gpu
STEPS = 6
C, K = True, False


def _config(**kw):
    # the zero polynomial: nothing ever accumulates, so every comparison skips until `max_skip_steps` binds -- C K K C K, and
    # the last step computes: decisions that no rounding can move
    return TeaCacheConfig(**{"coefficients": [0.0], "num_inference_steps": STEPS, "max_skip_steps": 2, **kw})


def test_threshold_zero_is_the_plain_eager_call(golden):
    pipe, a = _pipe(golden)
    pipe.use_hip_graph = False
    plain = _run(pipe, a, STEPS)
    pipe.use_hip_graph = None
    pipe.transformer.enable_cache(TeaCacheConfig(coefficients=[1.0, 0.0], rel_l1_thresh=0.0, num_inference_steps=STEPS))
    assert torch.equal(_run(pipe, a, STEPS), plain)
    log = pipe.transformer.cache_log
    assert [e[:3] for e in log] == [(ctx, s, C) for s in range(STEPS) for ctx in ("cond", "uncond")]
    # forwards 1 .. N - 2 measured a distance (and computed, as nothing is below 0); the first and the last compare nothing
    assert all((e[3] is None) == (e[1] in (0, STEPS - 1)) for e in log) and all(e[4] == 0.0 for e in log)
    assert all(e[3] > 0 for e in log if e[3] is not None)


def test_a_six_step_call_that_skips(golden):
    pipe, a = _pipe(golden)
    pipe.use_hip_graph = False
    plain = _run(pipe, a, STEPS)
    pipe.use_hip_graph = None
    pipe.transformer.enable_cache(_config())
    video = _run(pipe, a, STEPS)
    log = list(pipe.transformer.cache_log)
    for ctx in ("cond", "uncond"):
        assert [(e[1], e[2]) for e in log if e[0] == ctx] == list(enumerate([C, K, K, C, K, C]))
    assert bool(torch.isfinite(video).all()) and video.shape == plain.shape and not torch.equal(video, plain)
    # two calls, two streams: the same decisions, finite latents
    for batch_cfg, streams in ((False, False), (False, True)):
        pipe.batch_cfg, pipe.cfg_streams = batch_cfg, streams
        out = _run(pipe, a, STEPS)
        assert bool(torch.isfinite(out).all())
        assert [e[:3] for e in pipe.transformer.cache_log] == [e[:3] for e in log], (batch_cfg, streams)
    pipe.batch_cfg, pipe.cfg_streams = True, False
    # a second call starts from fresh state and reproduces the first; the state is dropped at the end of __call__
    assert torch.equal(_run(pipe, a, STEPS), video) and pipe.transformer.cache_log == log
    pipe.maybe_free_model_hooks()
    assert pipe.transformer._step_cache_states == {} and pipe.transformer.cache_log == log
    # a batch runs sample by sample, every sample from fresh state: row 0 is the single call, and the log is the last sample's
    b = dict(a)
    g = torch.Generator().manual_seed(9)
    b["latents0"] = torch.cat([a["latents0"], torch.randn(a["latents0"].shape, generator=g)], dim=0)
    both = _run(pipe, b, STEPS)
    assert both.shape[0] == 2 and torch.equal(both[:1], video) and not torch.equal(both[1:], video)
    assert [e[:3] for e in pipe.transformer.cache_log] == [e[:3] for e in log]
    # one captured step cannot contain it
    pipe.use_hip_graph = True
    with pytest.raises(RuntimeError, match="use_hip_graph=True with TeaCache") as err:
        _run(pipe, a, STEPS)
    assert str(err.value) == str(pipe.transformer._step_cache_policy.capture_refusal())
    pipe.use_hip_graph = None
    pipe.transformer.disable_cache()
    pipe.use_hip_graph = False
    assert torch.equal(_run(pipe, a, STEPS), plain)


def test_a_mismatching_step_count_warns(golden):
    pipe, a = _pipe(golden)
    pipe.transformer.enable_cache(_config(num_inference_steps=4))
    with pytest.warns(UserWarning, match="runs 6 steps, the config says num_inference_steps=4"):
        out = _run(pipe, a, STEPS)
    assert bool(torch.isfinite(out).all())
    assert [e[1] for e in pipe.transformer.cache_log if e[0] == "cond"] == [0, 1, 2, 3, 0, 1]      # the context started over
