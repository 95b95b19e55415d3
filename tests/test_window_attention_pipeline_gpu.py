"""Window attention through the FrameINO Wan denoise loop (pipeline_wan_i2v_motion_frameino.py): the tiny DiT of the golden
wan_pipe_tiny run on a clip large enough for a window to bite -- 6 generated latent frames + 1 identity-reference frame of
9 x 11 tokens (693 rows: three q-blocks, eleven key tiles, tokens per frame no multiple of the tile), 4 Euler steps, CFG 5.
The loop passes `id_frames` from the ID latent it was given; hipGraph replay must equal the eager loop bit for bit (the range
table is a static device tensor), and a timestep range makes the loop eager."""
import pytest
import torch

from frameino_amd.window_attention import WindowAttentionConfig
from tests.parity import hip_wan_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
FG, NID, H, W_ = 6, 1, 18, 22


def _pipe(golden):
    from frameino_amd.pipeline_wan_i2v_motion_frameino import WanImageToVideoPipeline
    from frameino_amd.schedulers import FlowMatchEulerDiscreteScheduler
    cfg, sd, a = golden("wan_pipe_tiny")
    m = hip_wan_model(cfg, {k[4:]: v for k, v in sd.items() if k.startswith("dit.")}, DEV)
    pipe = WanImageToVideoPipeline(scheduler=FlowMatchEulerDiscreteScheduler(shift=5.0), transformer=m, expand_timesteps=True)
    g = torch.Generator().manual_seed(77)
    rnd = lambda *s: torch.randn(*s, generator=g).to(DEV)          # noqa: E731
    mask = torch.ones(1, 1, FG, H, W_)
    mask[:, :, 0] = 0
    args = (rnd(1, 4, FG, H, W_), rnd(1, 4, 1, H, W_), rnd(1, 4, FG + NID, H, W_), rnd(1, 4, NID, H, W_), mask.to(DEV),
            a["prompt_embeds"].to(DEV), a["negative_embeds"].to(DEV), 5.0, 4)
    return pipe, args


def _window(pipe, **kw):
    pipe.transformer.disable_window_attention()
    pipe.transformer.enable_window_attention(WindowAttentionConfig(**{"window_frames": 1, "sink_frames": (0,), **kw}))


def test_graph_replay_equals_eager_and_differs_from_dense(golden):
    pipe, args = _pipe(golden)
    pipe.use_hip_graph = False
    dense = pipe.denoise(*args)
    _window(pipe)
    eager = pipe.denoise(*args)
    log = list(pipe.transformer.window_attention_log)
    assert log == [(i, None, True) for i in range(4)]                  # one CFG-batched forward per step
    assert any(k[0] == "window" and k[4] == NID for k in pipe.transformer._rope_cache)      # id_frames reached the model
    pipe.use_hip_graph = True                                          # a failed capture is an error
    graphed = pipe.denoise(*args)
    assert torch.equal(eager, graphed)
    assert torch.isfinite(eager).all() and not torch.equal(eager, dense)
    rel = ((eager - dense).pow(2).mean().sqrt() / dense.pow(2).mean().sqrt()).item()
    print(f"windowed vs dense latents after 4 steps: rel-RMS {rel:.3e}")
    # a window that covers the clip: the dense loop, bit for bit
    _window(pipe, window_frames=FG + NID)
    assert torch.equal(pipe.denoise(*args), dense)


def test_a_timestep_range_runs_the_loop_eagerly(golden):
    pipe, args = _pipe(golden)
    pipe.use_hip_graph = False
    dense = pipe.denoise(*args)
    _window(pipe)
    always = pipe.denoise(*args)
    _window(pipe, timestep_range=(200, 950), current_timestep_callback=lambda: pipe.current_timestep)
    pipe.use_hip_graph = True
    with pytest.raises(RuntimeError, match="use_hip_graph=True with window attention"):
        pipe.denoise(*args)
    pipe.use_hip_graph = None                                          # automatic: the loop is eager under a range
    out = pipe.denoise(*args)
    log = pipe.transformer.window_attention_log
    ts = [float(t) for t in pipe.scheduler.timesteps]
    assert [(i, t) for i, t, _ in log] == list(enumerate(ts))          # every step read the callback: nothing was replayed
    on = [200 < t < 950 for t in ts]
    assert [w for _, _, w in log] == on and any(on) and not all(on), ts
    assert not torch.equal(out, dense) and not torch.equal(out, always)
