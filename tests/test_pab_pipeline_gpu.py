"""Pyramid Attention Broadcast in the FrameINO Wan loop (golden wan_pipe_tiny pipeline, 3-block random pipeline): a timestep
range that excludes every step equals the uncached eager loop bit for bit; spatial 2 + cross 3 over the full range matches the
restated loop (tests/pab_ref.py driving oracle.wan_pipeline.wan_denoise_loop) within the bound
tests/test_step_cache_pipeline_gpu.py uses for the same comparison, rel-RMS 5e-2, with equal logs; the three CFG execution
forms give equal latents and logs; the state starts fresh per call; the graph loop is refused and comes back after
disable_cache(); a batch of 2 equals the two single calls."""
import pytest
import torch

from frameino_amd.step_cache import PyramidAttentionBroadcastConfig
from tests.parity import bf16_state_dict, rel_rms
from tests.pab_ref import PyramidAttentionBroadcastRef, loop_forward
from tests.test_step_cache_pipeline_gpu import _forms, _pipe3
from tests.test_wan_pipeline_gpu import _pipe, _run

pytestmark = pytest.mark.gpu
DEV = "cuda"
FULL = (-1, 1001)           # every timestep of a schedule lies strictly inside


def _enable(pipe, spatial=2, cross=3, rng=FULL):
    pipe.transformer.enable_cache(PyramidAttentionBroadcastConfig(
        spatial_attention_block_skip_range=spatial, cross_attention_block_skip_range=cross,
        spatial_attention_timestep_skip_range=rng, cross_attention_timestep_skip_range=rng,
        current_timestep_callback=lambda: pipe.current_timestep))


def _schedule(steps, spatial=2, cross=3):
    """the decisions of a call whose every timestep is in range, per forward (cond, uncond alternate)"""
    return [(it == 0 or it % spatial == 0, it == 0 or it % cross == 0) for it in range(steps) for _ in range(2)]


def test_a_range_that_excludes_every_timestep_equals_the_uncached_eager_loop(golden):
    pipe, a = _pipe(golden)
    pipe.use_hip_graph = False
    plain = _run(pipe, a)
    pipe.use_hip_graph = None
    _enable(pipe, rng=(2000, 3000))
    cached = _run(pipe, a)
    assert torch.equal(plain, cached)
    log = pipe.transformer.cache_log
    assert len(log) == 2 * int(a["steps"]) and all(e[3] and e[4] for e in log)
    assert [e[:2] for e in log[:4]] == [("cond", 0), ("uncond", 0), ("cond", 1), ("uncond", 1)]
    assert [e[2] for e in log[0::2]] == [float(t) for t in pipe.scheduler.timesteps]


def test_spatial_2_cross_3_matches_the_restated_loop(golden):
    from oracle.schedulers import FlowMatchEulerOracle
    from oracle.wan_pipeline import wan_denoise_loop
    pipe, a, cfg, sd = _pipe3(golden)
    _enable(pipe)
    out = _run(pipe, a)
    log = pipe.transformer.cache_log
    steps = int(a["steps"])
    assert [(e[3], e[4]) for e in log] == _schedule(steps) and not all(e[3] for e in log) and not all(e[4] for e in log)
    clock = {"t": None}
    ref = PyramidAttentionBroadcastRef(bf16_state_dict(sd), cfg, lambda: clock["t"], spatial=2, cross=3, spatial_range=FULL,
                                       cross_range=FULL)
    pe, ne = a["prompt_embeds"], a["negative_embeds"]
    fwd = loop_forward(ref, pe.bfloat16(), ne.bfloat16())

    def forward(x, t, e):
        clock["t"] = float(t.max())                         # the loop's t (the first frame's tokens carry 0)
        return fwd(x, t, e).float()

    want = wan_denoise_loop(None, cfg, FlowMatchEulerOracle(shift=5.0), a["latents0"], a["condition"], a["traj_latents"],
                            a["id_latent"], a["mask"], pe, ne, float(a["guidance"]), steps, model_dtype=torch.bfloat16,
                            forward=forward)
    # entry by entry: context, iteration and both decisions exactly; the timestep as the two schedulers compute it
    assert [e[:2] + e[3:] for e in ref.log] == [e[:2] + e[3:] for e in log]
    assert [e[2] for e in ref.log] == pytest.approx([e[2] for e in log], abs=1e-2)
    err = rel_rms(out, want)
    print(f"spatial 2 + cross 3, {steps} steps: rel-RMS {err:.3e} against the restated loop")
    assert err < 5e-2


def test_cfg_forms_give_equal_latents_and_logs(golden):
    pipe, a, _, _ = _pipe3(golden)
    _enable(pipe)
    forms = _forms(pipe, a)
    ref_lat, ref_log = forms["batch_cfg"]
    assert [(e[3], e[4]) for e in ref_log] == _schedule(int(a["steps"]))
    for name, (lat, log) in forms.items():
        assert torch.equal(lat, ref_lat) and log == ref_log, name


def test_state_is_fresh_per_call_and_reset_at_the_end_of_call(golden):
    pipe, a = _pipe(golden)
    tr = pipe.transformer
    _enable(pipe)
    first, log1 = _run(pipe, a), list(tr.cache_log)
    second, log2 = _run(pipe, a), list(tr.cache_log)
    assert torch.equal(first, second) and log1 == log2 and log1[0][1] == 0
    assert tr._step_cache_states                               # (denoise leaves the state to the end of __call__)
    pipe.maybe_free_model_hooks()
    assert tr._step_cache_states == {} and tr.cache_log == log2


def test_graph_mode_is_refused_and_returns_after_disable(golden):
    pipe, a = _pipe(golden)
    never = _run(pipe, a)                                    # default: graph replay, no cache
    tr = pipe.transformer
    _enable(pipe)
    pipe.use_hip_graph = True
    with pytest.raises(RuntimeError, match="use_hip_graph=True"):
        _run(pipe, a)
    pipe.use_hip_graph = None
    _run(pipe, a)                                            # None falls back to the eager loop
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


def test_a_batch_of_two_equals_the_two_single_calls(golden):
    pipe, a = _pipe(golden)
    _enable(pipe)
    d = lambda k: a[k].to(DEV)          # noqa: E731
    lat0 = d("latents0")
    lat1 = torch.randn(lat0.shape, generator=torch.Generator().manual_seed(5)).to(lat0)
    args = (d("condition"), d("traj_latents"), d("id_latent"), d("mask"), d("prompt_embeds"), d("negative_embeds"),
            float(a["guidance"]), int(a["steps"]))
    singles = [pipe.denoise(lat, *args) for lat in (lat0, lat1)]
    log = list(pipe.transformer.cache_log)
    both = pipe.denoise(torch.cat([lat0, lat1]), *args)
    assert torch.equal(both, torch.cat(singles))
    assert pipe.transformer.cache_log == log                 # (the log of the last sample: every sample starts afresh)
