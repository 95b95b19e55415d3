"""Pyramid Attention Broadcast through the CogVideoX FrameINO denoise loop (pipeline_cogvideox_i2v_motion_frameino.py) on the tiny
pipeline of tests/test_cog_model_gpu.py (the weights and conditions of tests/golden/cog_pipe_tiny.npz), DDIM, 8 steps.  Every
step's CFG batch of 2 runs under `cache_context("cond_uncond")` and makes one decision; the loop runs eagerly; the state is fresh
in every single-video loop.  The restated loop is oracle.cog_pipeline.cog_denoise_loop in bf16 with its model call replaced by
the restatement of tests/cog_pab_ref.py; tolerance: the bound the Cog loop tests hold the plain loop to against the bf16 oracle
loop (tests/test_cog_model_gpu.py: 6e-2)."""
import pytest
import torch

from frameino_amd.step_cache import PyramidAttentionBroadcastConfig, pab_decide
from tests.cog_pab_ref import CogPyramidAttentionBroadcastRef
from tests.parity import record, rel_rms
from tests.test_cog_model_gpu import _cog_pipe

pytestmark = pytest.mark.gpu
DEV = "cuda"
STEPS = 8
LOOP_BOUND = 6e-2
RANGE = (200, 800)


def _run(pipe, a, rows=slice(0, 1), **over):
    d = lambda k: over[k] if k in over else a[k].to(DEV)          # noqa: E731
    return pipe.denoise(d("latents0")[rows], d("image_latents"), d("traj_latents"), d("id_latent"), d("prompt_embeds")[rows],
                        d("negative_embeds")[rows], float(a["guidance"]), STEPS)


def _enable(pipe, spatial=2, rng=RANGE):
    pipe.transformer.enable_cache(PyramidAttentionBroadcastConfig(
        spatial_attention_block_skip_range=spatial, spatial_attention_timestep_skip_range=rng,
        current_timestep_callback=lambda: pipe.current_timestep))


def test_a_range_that_excludes_every_timestep_equals_the_uncached_eager_loop(golden):
    pipe, a, _ = _cog_pipe(golden)
    tr = pipe.transformer
    pipe.use_hip_graph = False
    want = _run(pipe, a)                                           # (the default model: its last block skips the dead rows)
    tr.skip_dead_rows = False
    want_all_rows = _run(pipe, a)                                  # every block on all rows, as under the cache
    tr.skip_dead_rows = True
    _enable(pipe, rng=(2000, 3000))
    pipe.use_hip_graph = None
    out = _run(pipe, a)
    assert torch.isfinite(out.float()).all() and torch.equal(out, want_all_rows) and torch.equal(out, want)
    log = tr.cache_log
    assert len(log) == STEPS and all(e[0] == "cond_uncond" and e[3] and e[4] for e in log)
    assert [e[1] for e in log] == list(range(STEPS)) and [e[2] for e in log] == [float(t) for t in pipe.scheduler.timesteps]
    assert pipe.current_timestep is None and tr._step_cache_states == {}


def test_spatial_2_over_the_middle_steps_matches_the_restated_loop(golden, monkeypatch):
    from oracle import cog_pipeline as P
    pipe, a, (cfg, sd, _, _) = _cog_pipe(golden)
    tr = pipe.transformer
    pipe.use_hip_graph = False
    plain = _run(pipe, a)
    _enable(pipe)
    out = _run(pipe, a)
    log = tr.cache_log                                             # readable after the call
    ts = [e[2] for e in log]
    want = [pab_decide(i, t, i > 0, 2, RANGE) for i, t in enumerate(ts)]
    assert len(log) == STEPS and [e[3] for e in log] == want
    # the first step and the steps outside (200, 800) compute, inside every second forward (by the call's counter) does
    assert want[0] and all(w for w, t in zip(want, ts) if not RANGE[0] < t < RANGE[1])
    inside = [(i, w) for i, (w, t) in enumerate(zip(want, ts)) if RANGE[0] < t < RANGE[1] and i > 0]
    assert len(inside) >= 3 and all(w == (i % 2 == 0) for i, w in inside) and not all(w for _, w in inside)
    assert not torch.equal(out, plain)
    # the restated loop: the oracle's, in bf16, its model call under the restated cache
    sdb = {k: v.bfloat16() for k, v in sd.items()}
    clock = {}
    ref = CogPyramidAttentionBroadcastRef(sdb, cfg, lambda: clock["t"], spatial=2, timestep_range=RANGE)

    def forward(sd_, cfg_, x, prompt, timestep, rotary):
        clock["t"] = float(timestep[0])
        return ref("cond_uncond", x, prompt, timestep, rotary)
    monkeypatch.setattr(P, "cog_forward", forward)
    b = lambda k: a[k].bfloat16()       # noqa: E731
    restated = P.cog_denoise_loop(sdb, cfg, b("latents0"), b("image_latents"), b("traj_latents"), b("id_latent"),
                                  b("prompt_embeds"), b("negative_embeds"), (a["rope_cos"], a["rope_sin"]), float(a["guidance"]),
                                  STEPS)
    assert ref.log == log
    err, far = rel_rms(out, restated), rel_rms(plain, restated)
    print(f"cached loop vs the restated loop: rel-RMS {err:.3e} (the uncached loop against it: {far:.3e})")
    record("cog_pab_loop[tiny, 8 steps, spatial 2 over (200, 800)]", "rel_rms hip bf16 vs the restated bf16 loop", err, LOOP_BOUND)
    assert out.shape == restated.shape and err < LOOP_BOUND
    assert far > 2 * LOOP_BOUND                                    # (the restated loops differ by 0.23: the bound can tell them apart)


def test_state_is_fresh_per_call_and_the_log_outlives_it(golden):
    pipe, a, _ = _cog_pipe(golden)
    tr = pipe.transformer
    _enable(pipe)
    first = _run(pipe, a)
    log = list(tr.cache_log)
    assert len(log) == STEPS and tr._step_cache_states == {} and tr.is_cache_enabled
    again = _run(pipe, a)                                          # iteration 0 again: the same decisions, the same bits
    assert torch.equal(again, first) and tr.cache_log == log and tr.cache_log is not log
    pipe.maybe_free_model_hooks()
    assert tr.cache_log == log


def test_graph_mode_is_refused_and_returns_after_disable_cache(golden):
    pipe, a, _ = _cog_pipe(golden)
    tr = pipe.transformer
    pipe.use_hip_graph = True
    graphed = _run(pipe, a)                                        # (True makes a failed capture an error)
    _enable(pipe)
    with pytest.raises(RuntimeError, match="use_hip_graph=True with Pyramid Attention Broadcast"):
        _run(pipe, a)
    assert tr.cache_log == ()                                      # refused before any forward
    tr.disable_cache()
    assert torch.equal(_run(pipe, a), graphed)


def test_a_batch_of_two_equals_the_two_single_calls(golden):
    pipe, a, _ = _cog_pipe(golden)
    _enable(pipe)
    g = torch.Generator().manual_seed(3)
    lat = torch.cat([a["latents0"], torch.randn(a["latents0"].shape, generator=g)]).to(DEV)
    pe = torch.cat([a["prompt_embeds"], a["prompt_embeds"].flip(1)]).to(DEV)
    ne = torch.cat([a["negative_embeds"], a["negative_embeds"]]).to(DEV)
    over = dict(latents0=lat, prompt_embeds=pe, negative_embeds=ne)
    both = _run(pipe, a, rows=slice(0, 2), **over)
    assert both.shape[0] == 2 and not torch.equal(both[0], both[1])
    assert len(pipe.transformer.cache_log) == STEPS               # the last video's loop
    for i in range(2):
        assert torch.equal(_run(pipe, a, rows=slice(i, i + 1), **over), both[i:i + 1]), i


@pytest.mark.parametrize("extra", [[], ["--mxfp8", "--fp8-attention", "--smooth-k", "--window-frames", "1"]], ids=["fp16", "fp8-path-window"])
def test_the_example_script_s_pab_flags(extra):
    """examples/run_cogvideox_frameino.py --smoke --pab 2 [--pab-range LO HI]: three DDIM steps at 999, 666, 333 -- the second lies
    inside (100, 800) at an odd iteration and re-uses the branch"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "run_cogvideox_frameino.py"), "--smoke", "--scheduler", "ddim",
                        "--pab", "2", "--pab-range", "100", "800"] + extra, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "clip (9 frames 64x96" in r.stdout and "2 of 3 steps computed the attention branch" in r.stdout, r.stdout[-2000:]
