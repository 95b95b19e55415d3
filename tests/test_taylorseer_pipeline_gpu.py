"""TaylorSeer caching in the FrameINO Wan loop (the tiny golden pipeline of tests/test_pab_pipeline_gpu.py), default and lite
mode: cache_interval 1 equals the uncached eager loop bit for bit; warm-up 2 / interval 3 over 8 steps decides C C P P C P P C in
both contexts and gives a finite video that differs from the uncached one; the three CFG execution forms agree; the graph loop
is refused; every call starts from fresh state."""
import pytest
import torch

from frameino_amd.step_cache import TaylorSeerCacheConfig
from tests.test_wan_pipeline_gpu import _pipe

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = pytest.mark.parametrize("lite", [False, True], ids=["default", "lite"])
C, P = True, False
SCHEDULE = [C, C, P, P, C, P, P, C]


def _run(pipe, a, steps=None):
    d = lambda k: a[k].to(DEV)          # noqa: E731
    return pipe.denoise(d("latents0"), d("condition"), d("traj_latents"), d("id_latent"), d("mask"), d("prompt_embeds"),
                        d("negative_embeds"), float(a["guidance"]), int(a["steps"]) if steps is None else steps)


def _enable(pipe, lite, interval=3, warmup=2):
    pipe.transformer.enable_cache(TaylorSeerCacheConfig(cache_interval=interval, disable_cache_before_step=warmup,
                                                        use_lite_mode=lite))


@MODES
def test_interval_1_equals_the_uncached_eager_loop(golden, lite):
    pipe, a = _pipe(golden)
    pipe.use_hip_graph = False
    plain = _run(pipe, a)
    pipe.use_hip_graph = None
    _enable(pipe, lite, interval=1)
    assert torch.equal(_run(pipe, a), plain)
    log = pipe.transformer.cache_log
    assert log == [(ctx, s, True) for s in range(int(a["steps"])) for ctx in ("cond", "uncond")]


@MODES
def test_warmup_2_interval_3_over_8_steps(golden, lite):
    pipe, a = _pipe(golden)
    pipe.use_hip_graph = False
    plain = _run(pipe, a, 8)
    pipe.use_hip_graph = None
    _enable(pipe, lite)
    forms = _forms_8(pipe, a)
    video, log = forms["batch_cfg"]
    assert log == [(ctx, s, c) for s, c in enumerate(SCHEDULE) for ctx in ("cond", "uncond")]
    assert bool(torch.isfinite(video).all()) and video.shape == plain.shape and not torch.equal(video, plain)
    for name, (lat, lg) in forms.items():                      # batched CFG, two calls, two streams: equal latents and logs
        assert torch.equal(lat, video) and lg == log, name
    # a second call starts from fresh state and reproduces the first; the state is dropped at the end of __call__
    assert torch.equal(_run(pipe, a, 8), video) and pipe.transformer.cache_log == log
    assert pipe.transformer._step_cache_states
    pipe.maybe_free_model_hooks()
    assert pipe.transformer._step_cache_states == {} and pipe.transformer.cache_log == log


def _forms_8(pipe, a):
    out = {}
    for name, batch_cfg, streams in (("batch_cfg", True, False), ("sequential", False, False), ("cfg_streams", False, True)):
        pipe.batch_cfg, pipe.cfg_streams = batch_cfg, streams
        out[name] = (_run(pipe, a, 8), list(pipe.transformer.cache_log))
    pipe.batch_cfg, pipe.cfg_streams = True, False
    return out


def test_graph_mode_is_refused_and_returns_after_disable(golden):
    pipe, a = _pipe(golden)
    never = _run(pipe, a)                                    # default: graph replay, no cache
    _enable(pipe, False)
    pipe.use_hip_graph = True
    with pytest.raises(RuntimeError, match="use_hip_graph=True with TaylorSeer"):
        _run(pipe, a)
    pipe.use_hip_graph = None
    _run(pipe, a)                                            # None falls back to the eager loop
    pipe.transformer.disable_cache()
    assert torch.equal(_run(pipe, a), never)


def test_a_batch_of_two_equals_the_two_single_calls(golden):
    pipe, a = _pipe(golden)
    _enable(pipe, False)
    d = lambda k: a[k].to(DEV)          # noqa: E731
    lat0 = d("latents0")
    lat1 = torch.randn(lat0.shape, generator=torch.Generator().manual_seed(5)).to(lat0)
    args = (d("condition"), d("traj_latents"), d("id_latent"), d("mask"), d("prompt_embeds"), d("negative_embeds"),
            float(a["guidance"]), 5)
    singles = [pipe.denoise(lat, *args) for lat in (lat0, lat1)]
    log = list(pipe.transformer.cache_log)
    both = pipe.denoise(torch.cat([lat0, lat1]), *args)
    assert torch.equal(both, torch.cat(singles))
    assert pipe.transformer.cache_log == log                 # (the log of the last sample: every sample starts afresh)
    assert [e[2] for e in log if e[0] == "cond"] == [C, C, P, P, C]
