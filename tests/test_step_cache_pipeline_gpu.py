"""First-block caching in the FrameINO Wan loop (golden wan_pipe_tiny pipeline, 3-block random pipeline): threshold 0 equals the
uncached eager loop bit for bit, threshold inf skips every step after the first and matches the restated loop, the three CFG
execution forms decide alike, the state starts fresh per call, and the graph loop comes back after disable_cache()."""
import math

import pytest
import torch

from frameino_amd.step_cache import FirstBlockCacheConfig
from tests.parity import bf16_state_dict, hip_wan_model, rel_rms
from tests.step_cache_ref import FirstBlockCacheRef, loop_forward
from tests.test_wan_pipeline_gpu import _pipe, _run

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _pipe3(golden):
    """the golden pipeline's inputs on a 3-block random DiT of the same geometry"""
    from oracle import wan_dit as W
    from frameino_amd.pipeline_wan_i2v_motion_frameino import WanImageToVideoPipeline
    from frameino_amd.schedulers import FlowMatchEulerDiscreteScheduler
    cfg, _, a = golden("wan_pipe_tiny")
    cfg = dict(cfg, num_layers=3)
    sd = W.wan_random_state_dict(cfg, seed=21, dtype=torch.float32, std=0.04)
    pipe = WanImageToVideoPipeline(scheduler=FlowMatchEulerDiscreteScheduler(shift=5.0), transformer=hip_wan_model(cfg, sd, DEV),
                                   expand_timesteps=True)
    return pipe, a, cfg, sd


def _forms(pipe, a):
    out = {}
    for name, batch_cfg, streams in (("batch_cfg", True, False), ("sequential", False, False), ("cfg_streams", False, True)):
        pipe.batch_cfg, pipe.cfg_streams = batch_cfg, streams
        out[name] = (_run(pipe, a), list(pipe.transformer.cache_log))
    pipe.batch_cfg, pipe.cfg_streams = True, False
    return out


def test_threshold_zero_equals_the_uncached_eager_loop(golden):
    pipe, a = _pipe(golden)
    pipe.use_hip_graph = False
    plain = _run(pipe, a)
    pipe.use_hip_graph = None
    pipe.transformer.enable_cache(FirstBlockCacheConfig(threshold=0.0))
    cached = _run(pipe, a)
    assert torch.equal(plain, cached)
    log = pipe.transformer.cache_log
    assert len(log) == 2 * int(a["steps"]) and all(e[3] for e in log)
    assert [e[0] for e in log[:2]] == ["cond", "uncond"]


def test_threshold_inf_skips_every_later_step_and_matches_the_restated_loop(golden):
    from oracle.schedulers import FlowMatchEulerOracle
    from oracle.wan_pipeline import wan_denoise_loop
    pipe, a, cfg, sd = _pipe3(golden)
    pipe.transformer.enable_cache(FirstBlockCacheConfig(threshold=math.inf))
    out = _run(pipe, a)
    log = pipe.transformer.cache_log
    assert [(e[0], e[1], e[3]) for e in log[:2]] == [("cond", 0, True), ("uncond", 0, True)]
    assert len(log) == 2 * int(a["steps"]) and not any(e[3] for e in log[2:])
    ref = FirstBlockCacheRef(bf16_state_dict(sd), cfg, math.inf)
    pe, ne = a["prompt_embeds"], a["negative_embeds"]
    fwd = loop_forward(ref, pe.bfloat16(), ne.bfloat16())
    want = wan_denoise_loop(None, cfg, FlowMatchEulerOracle(shift=5.0), a["latents0"], a["condition"], a["traj_latents"],
                            a["id_latent"], a["mask"], pe, ne, float(a["guidance"]), int(a["steps"]), model_dtype=torch.bfloat16,
                            forward=lambda x, t, e: fwd(x, t, e).float())
    assert [e[3] for e in ref.log] == [e[3] for e in log]
    assert rel_rms(out, want) < 5e-2


def test_cfg_forms_decide_alike_and_give_equal_latents(golden):
    pipe, a, _, _ = _pipe3(golden)
    tr = pipe.transformer
    tr.enable_cache(FirstBlockCacheConfig(threshold=0.0))
    forms = _forms(pipe, a)
    ref_lat, ref_log = forms["batch_cfg"]
    for lat, log in forms.values():
        assert torch.equal(lat, ref_lat) and log == ref_log
    # a threshold between the two branches' first diffs: step 1 computes one branch and skips the other (a mixed step)
    d_cond, d_uncond = ref_log[2][2], ref_log[3][2]
    assert ref_log[2][:2] == ("cond", 1) and ref_log[3][:2] == ("uncond", 1)
    lo, hi = sorted((d_cond, d_uncond))
    assert hi > lo, (d_cond, d_uncond)           # (every form computes these same bits: any threshold between them will do)
    tr.disable_cache()
    tr.enable_cache(FirstBlockCacheConfig(threshold=(lo + hi) / 2))
    forms = _forms(pipe, a)
    ref_lat, ref_log = forms["batch_cfg"]
    assert ref_log[2][3] != ref_log[3][3]                                   # mixed
    for lat, log in forms.values():
        assert torch.equal(lat, ref_lat) and log == ref_log


def test_state_is_fresh_per_call_and_reset_at_the_end_of_call(golden):
    pipe, a = _pipe(golden)
    tr = pipe.transformer
    tr.enable_cache(FirstBlockCacheConfig(threshold=0.05))
    first, log1 = _run(pipe, a), list(tr.cache_log)
    second, log2 = _run(pipe, a), list(tr.cache_log)
    assert torch.equal(first, second) and log1 == log2
    reset = []
    orig = tr._reset_stateful_cache
    tr._reset_stateful_cache = lambda *k: (reset.append(1), orig(*k))[1]
    try:
        pipe.maybe_free_model_hooks()
    finally:
        del tr._reset_stateful_cache
    assert reset and tr._step_cache_states == {} and tr.cache_log == log2


def test_graph_mode_is_refused_with_the_cache_and_returns_after_disable(golden):
    pipe, a = _pipe(golden)
    never = _run(pipe, a)                                    # default: graph replay, no cache
    tr = pipe.transformer
    tr.enable_cache(FirstBlockCacheConfig(threshold=0.05))
    pipe.use_hip_graph = True
    with pytest.raises(RuntimeError, match="use_hip_graph=True"):
        _run(pipe, a)
    pipe.use_hip_graph = None
    _run(pipe, a)
    tr.disable_cache()
    from frameino_amd import graph_step
    captured = []
    orig = graph_step.StepGraph.step

    def spy(self):
        captured.append(self.enabled)
        return orig(self)
    graph_step.StepGraph.step = spy
    try:
        back = _run(pipe, a)
    finally:
        graph_step.StepGraph.step = orig
    assert captured and all(captured)                        # the graph loop again
    assert torch.equal(back, never)


def test_a_batch_with_the_cache_is_refused(golden):
    pipe, a = _pipe(golden)
    pipe.transformer.enable_cache(FirstBlockCacheConfig(threshold=0.05))
    d = lambda k: a[k].to(DEV)          # noqa: E731
    with pytest.raises(NotImplementedError, match="batch"):
        pipe.denoise(d("latents0").repeat(2, 1, 1, 1, 1), d("condition"), d("traj_latents"), d("id_latent"), d("mask"),
                     d("prompt_embeds"), d("negative_embeds"), float(a["guidance"]), int(a["steps"]))
