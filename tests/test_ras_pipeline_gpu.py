"""Region-adaptive sampling in the FrameINO Wan loop (the tiny golden pipeline of tests/test_wan_pipeline_gpu.py): a 10-step call
with warmup_steps = 2 and full_step_interval = 3 follows `ras_decide`, equals a hand loop over `forward`, differs from the
uncached call, and is reproduced by a second call (the state is reset per call); sample_ratio = 1 is the uncached call bit for
bit; the graph loop is refused; a call whose step count is not the config's warns."""
import pytest
import torch

from frameino_amd.step_cache import RegionAdaptiveSamplingConfig, ras_active_count, ras_decide
from tests.test_taylorseer_pipeline_gpu import _run
from tests.test_wan_pipeline_gpu import _pipe

pytestmark = pytest.mark.gpu
DEV = "cuda"
STEPS = 10


def _config(**kw):
    return RegionAdaptiveSamplingConfig(**{"sample_ratio": 0.5, "warmup_steps": 2, "full_step_interval": 3, "full_steps_at_end": 2,
                                           "num_inference_steps": STEPS, **kw})


def _hand_loop(pipe, a, steps):
    """the denoising loop restated over `transformer.forward`: the CFG batch as one call that names its two contexts"""
    tr, o = pipe.transformer, pipe.transformer.ops
    d = lambda k: a[k].to(DEV)          # noqa: E731
    tr._reset_stateful_cache()
    pipe.scheduler.set_timesteps(steps, device=DEV)
    st = pipe.make_state(d("latents0"), d("condition"), d("traj_latents"), d("id_latent"), d("mask"), d("prompt_embeds"),
                         d("negative_embeds"), float(a["guidance"]))
    assert st.cfg and st.pe_ne is not None and st.unipc is None
    ts, dts = pipe.scheduler.timesteps.to(DEV).float(), pipe.scheduler.dts.to(DEV)
    live = {"live_rows": st.live_rows} if st.live_rows is not None else {}
    for i in range(steps):
        st.t_rows[1:2].copy_(ts[i:i + 1])
        st.dt.copy_(dts[i:i + 1])
        x = o.wan_model_input(st.lat, st.cond, st.idl, st.traj, tr.dtype, out=st.x)[None]
        with tr.cache_context("cfg"):
            both = tr(hidden_states=x.expand(2, -1, -1, -1, -1), timestep=None, encoder_hidden_states=st.pe_ne, return_dict=False,
                      timestep_rows=(st.t_rows, st.sel), _cache_contexts=("cond", "uncond"), **live)[0]
        o.cfg_euler_step_(st.lat, both[0], both[1], st.guidance, st.dt,
                          round_out=getattr(pipe.scheduler, "cast_output_to_model_dtype", True))
    return (1 - d("mask")) * d("condition") + d("mask") * st.lat[None]


def test_a_ten_step_call_follows_the_schedule_and_a_hand_loop(golden):
    pipe, a = _pipe(golden)
    pipe.use_hip_graph = False
    plain = _run(pipe, a, STEPS)
    pipe.use_hip_graph = None
    cfg = _config()
    tr = pipe.transformer
    tr.enable_cache(cfg)
    video = _run(pipe, a, STEPS)
    log = list(tr.cache_log)
    full = [ras_decide(s, cfg) for s in range(STEPS)]
    assert full == [True, True, False, False, True, False, False, True, True, True]
    assert [(c, s, f) for c, s, f, _ in log] == [(c, s, full[s]) for s in range(STEPS) for c in ("cond", "uncond")]
    rows = {r for _, _, f, r in log if f}, {r for _, _, f, r in log if not f}
    assert len(rows[0]) == 1 and len(rows[1]) == 1 and 0 < min(rows[1]) < min(rows[0])      # partial steps ran fewer rows
    n = min(rows[0])
    assert min(rows[1]) in {ras_active_count(0.5, e) for e in range(n // 4, n + 1)}
    assert bool(torch.isfinite(video).all()) and video.shape == plain.shape
    assert not torch.equal(video, plain)                        # (without the feature the cached call IS the uncached call)
    # the state is dropped at the end of a call; a second call starts from fresh state and reproduces the first
    assert torch.equal(_run(pipe, a, STEPS), video) and tr.cache_log == log
    pipe.maybe_free_model_hooks()
    assert tr._step_cache_states == {} and tr.cache_log == log
    # a hand loop over forward
    assert torch.equal(_hand_loop(pipe, a, STEPS), video) and tr.cache_log == log
    # one captured step cannot contain it
    pipe.use_hip_graph = True
    with pytest.raises(RuntimeError, match="use_hip_graph=True with region-adaptive sampling"):
        _run(pipe, a, STEPS)
    pipe.use_hip_graph = None
    tr.disable_cache()
    pipe.use_hip_graph = False
    assert torch.equal(_run(pipe, a, STEPS), plain)


def test_a_ratio_of_one_is_the_uncached_call_bit_for_bit(golden):
    pipe, a = _pipe(golden)
    pipe.use_hip_graph = False
    plain = _run(pipe, a, STEPS)
    pipe.use_hip_graph = None
    pipe.transformer.enable_cache(_config(sample_ratio=1.0))
    assert torch.equal(_run(pipe, a, STEPS), plain)
    assert all(e[2] for e in pipe.transformer.cache_log) and len(pipe.transformer.cache_log) == 2 * STEPS


def test_a_mismatching_step_count_warns(golden):
    pipe, a = _pipe(golden)
    pipe.transformer.enable_cache(_config(num_inference_steps=6))
    with pytest.warns(UserWarning, match="runs 10 steps, the config says num_inference_steps=6"):
        out = _run(pipe, a, STEPS)
    assert bool(torch.isfinite(out).all())
    assert all(f for _, s, f, _ in pipe.transformer.cache_log if s >= 4)          # from 6 - 2 on every forward is full
