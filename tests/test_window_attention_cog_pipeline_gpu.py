"""Window attention through the CogVideoX FrameINO denoise loop (pipeline_cogvideox_i2v_motion_frameino.py): the tiny DiT and
geometry of tests/cog_window_attn_ref.py (8 generated latent frames + the ID frame, 150 tokens each, so that window_frames = 1 is
not all-covering), 5 steps.  The loop passes `id_frames` = the ID latent's frame count (0 for FrameOut); without a timestep range
the table is a static device tensor and the step replays from a captured graph; with a range the loop runs eagerly."""
import pytest
import torch

from frameino_amd.window_attention import WindowAttentionConfig
from tests import cog_window_attn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
STEPS = 5


def _pipe(stage1=False, **over):
    from frameino_amd.cogvideox_transformer_3d import CogVideoXTransformer3DModel
    from frameino_amd.schedulers import CogVideoXDDIMScheduler
    if stage1:
        from frameino_amd.pipeline_cogvideox_i2v_motion import CogVideoXImageToVideoPipeline
    else:
        from frameino_amd.pipeline_cogvideox_i2v_motion_frameino import CogVideoXImageToVideoPipeline
    m = CogVideoXTransformer3DModel(**{**R.TINY_CFG, **over}).to(DEV)
    m.load_reference_state_dict(R.tiny_state_dict(11, 0.05, 4.0, 0.5), dtype=torch.bfloat16)
    return CogVideoXImageToVideoPipeline(transformer=m.eval(), scheduler=CogVideoXDDIMScheduler())


def _conditions(frame_out=False):
    g = torch.Generator().manual_seed(5)
    nlf, C = R.FRAMES - 1, 2
    shape = (1, nlf, C, R.LAT_H, R.LAT_W)
    lat = torch.randn(shape, generator=g)
    img = torch.cat([torch.randn(1, 1, C, R.LAT_H, R.LAT_W, generator=g), torch.zeros(1, nlf - 1, C, R.LAT_H, R.LAT_W)], 1)
    trj = torch.randn(shape, generator=g)
    idl = None if frame_out else torch.randn(1, 1, C, R.LAT_H, R.LAT_W, generator=g)
    pe, ne = torch.randn(1, R.TEXT, 16, generator=g), torch.randn(1, R.TEXT, 16, generator=g)
    rot = tuple(t.to(DEV) for t in R.tiny_inputs()[3])
    d = lambda t: None if t is None else t.to(DEV)          # noqa: E731
    return d(lat), d(img), d(trj), d(idl), d(pe), d(ne), rot


def _run(pipe, cond):
    lat, img, trj, idl, pe, ne, rot = cond
    return pipe.denoise(lat, img, trj, idl, pe, ne, 6.0, STEPS, image_rotary_emb=rot)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "mxfp8-linears-fp8-attention-smooth-k"])
def test_graph_replay_equals_the_eager_loop_with_a_window_on(fp8):
    pipe, cond = _pipe(), _conditions()
    tr = pipe.transformer
    pipe.use_hip_graph = False
    plain = _run(pipe, cond)
    if fp8:
        tr.enable_mxfp8_linears()
        tr.enable_fp8_attention(smooth_k=True)
    tr.enable_window_attention(WindowAttentionConfig(window_frames=1, sink_frames=(0,)))
    eager = _run(pipe, cond)
    n_eager = len(tr.window_attention_log)
    assert n_eager == STEPS and all(on and t is None for _, t, on in tr.window_attention_log)
    pipe.use_hip_graph = True                  # (True makes a failed capture an error)
    graphed = _run(pipe, cond)
    assert torch.isfinite(eager.float()).all() and torch.equal(eager, graphed)
    assert len(tr.window_attention_log) - n_eager == 2       # step 0 eager, step 1 captured, the rest replays
    assert not torch.equal(eager, plain)                     # (the window reaches the loop)
    assert any(k[0] == "window" and k[5] == 1 for k in tr._pos_cache)        # id_frames = the ID latent's one frame


def test_a_window_at_least_as_large_as_the_clip_equals_the_plain_call_bit_for_bit():
    pipe, cond = _pipe(), _conditions()
    want = _run(pipe, cond)
    pipe.transformer.enable_window_attention(WindowAttentionConfig(window_frames=R.FRAMES))
    assert torch.equal(_run(pipe, cond), want)
    pipe.transformer.disable_window_attention()
    assert torch.equal(_run(pipe, cond), want)


def test_a_timestep_range_runs_eagerly_and_a_required_graph_raises():
    pipe, cond = _pipe(), _conditions()
    tr = pipe.transformer
    pipe.use_hip_graph = False
    dense = _run(pipe, cond)
    tr.enable_window_attention(WindowAttentionConfig(window_frames=1))
    windowed = _run(pipe, cond)
    tr.enable_window_attention(WindowAttentionConfig(window_frames=1, timestep_range=(300, 700),
                                                     current_timestep_callback=lambda: pipe.current_timestep))
    pipe.use_hip_graph = None                  # the default: would replay, were the loop capturable
    out = _run(pipe, cond)
    log = tr.window_attention_log
    assert len(log) == STEPS and [i for i, _, _ in log] == list(range(STEPS))        # every step ran eagerly, one read each
    assert [on for _, _, on in log] == [300 < t < 700 for _, t, _ in log]
    assert any(on for _, _, on in log) and not all(on for _, _, on in log)
    assert not torch.equal(out, dense) and not torch.equal(out, windowed)
    assert pipe.current_timestep is None
    pipe.use_hip_graph = True
    with pytest.raises(RuntimeError, match="use_hip_graph=True"):
        _run(pipe, cond)


def test_frame_out_has_no_id_frame_and_stage_1_shares_the_loop():
    """FrameOut (no identity reference): id_frames = 0, the only sink is the config's; the stage-1 pipeline shares the model call"""
    pipe, cond = _pipe(), _conditions(frame_out=True)
    tr = pipe.transformer
    plain = _run(pipe, cond)
    tr.enable_window_attention(WindowAttentionConfig(window_frames=1))
    out = _run(pipe, cond)
    assert out.shape == plain.shape and torch.isfinite(out.float()).all() and not torch.equal(out, plain)
    keys = [k for k in tr._pos_cache if k[0] == "window"]
    assert keys and all(k[1] == R.FRAMES - 1 and k[5] == 0 for k in keys)
    s1 = _pipe(stage1=True, use_FrameIn=False, sample_frames=29)
    lat, img, trj, _, pe, ne, rot = cond
    n = (R.FRAMES - 1) * R.TPF
    rot = (rot[0][:n], rot[1][:n])
    plain = s1.denoise(lat, img, trj, pe, ne, 6.0, 3, image_rotary_emb=rot)
    s1.transformer.enable_window_attention(WindowAttentionConfig(window_frames=1))
    out = s1.denoise(lat, img, trj, pe, ne, 6.0, 3, image_rotary_emb=rot)
    assert torch.isfinite(out.float()).all() and not torch.equal(out, plain)
    assert all(k[5] == 0 for k in s1.transformer._pos_cache if k[0] == "window")
