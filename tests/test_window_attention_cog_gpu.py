"""Sliding-window self-attention over frames on the CogVideoX DiT (CogVideoXTransformer3DModel.enable_window_attention) against
the restatement in tests/cog_window_attn_ref.py: oracle.cog_dit's pieces in bf16 with the joint self-attention under the boolean
block mask expanded from the same range table.  The tiny DiT of the fixtures' shape (2 layers, 2 heads x 64, 8 text rows) on 9
latent frames of 150 tokens: L = 1358 = six q-blocks, 22 key tiles with 14 keys in the last, window_frames = 1, sink frame 0, the
last frame an ID frame.  Tolerances: the dense tiny forward's bound against the bf16 oracle (tests/test_cog_model_gpu.py: 3e-2)
and, with fp8 attention, the bound the tiny-model fp8 attention test holds the dense model to
(tests/test_attention_fp8_smooth_gpu.py: COG_FP8_BOUND = 6e-2)."""
import pytest
import torch

from frameino_amd.window_attention import WindowAttentionConfig, frame_window_ranges, ranges_cover_all, ranges_density
from tests import cog_window_attn_ref as R
from tests.parity import record, rel_rms

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOUND = 3e-2
FP8_BOUND = 6e-2
CFG, FRAMES, TPF, TEXT, L, SINKS = R.TINY_CFG, R.FRAMES, R.TPF, R.TEXT, R.L, R.SINKS
# The bf16 model skips the text rows' queries in its last block (skip_dead_rows, the default): that block's queries are the video
# rows [TEXT, L) and its q-blocks are counted from row TEXT.  With fp8 attention every block runs all L rows.
VIDEO_ROWS = (TEXT, L)


def _ref(sdb, x, txt, ts, rot, masks):
    return R.window_forward(sdb, CFG, x.bfloat16(), txt.bfloat16(), ts, rot, masks).float()


@pytest.fixture(scope="module")
def setup():
    """inputs on which the restatement's windowed and dense outputs differ by at least 5 x BOUND (on the CPU, the restatement
    alone): otherwise no assertion below could tell a window from none.  The weights are scaled until they do."""
    x, txt, ts, rot = R.tiny_inputs(batch=2)
    masks = R.layer_masks(2, FRAMES, TPF, TEXT, 1, SINKS, live_rows=VIDEO_ROWS)
    for v_scale, gate in ((4.0, 0.5), (8.0, 1.0), (16.0, 1.0)):
        sd = R.tiny_state_dict(11, 0.05, v_scale, gate)
        sdb = {k: v.bfloat16() for k, v in sd.items()}
        dense = _ref(sdb, x[:1], txt[:1], ts[:1], rot, {})
        windowed = _ref(sdb, x[:1], txt[:1], ts[:1], rot, masks)
        gap = rel_rms(windowed, dense)
        print(f"restatement: windowed vs dense rel-RMS {gap:.3e} at value scale {v_scale}, gate {gate} (needs >= {5 * BOUND:.3e})")
        if gap >= 5 * BOUND:
            return sd, sdb, (x, txt, ts, rot), dense, windowed, gap
    raise AssertionError(f"no scale separates the window from the dense model: last gap {gap}")


def _model(sd, fp8=None, **cfg):
    from frameino_amd.cogvideox_transformer_3d import CogVideoXTransformer3DModel
    m = CogVideoXTransformer3DModel(**CFG).to(DEV)
    m.load_reference_state_dict(sd, dtype=torch.bfloat16)
    m = m.eval()
    if fp8 is not None:
        m.enable_fp8_attention(**fp8)
    if cfg:
        m.enable_window_attention(WindowAttentionConfig(**{"window_frames": 1, "sink_frames": (0,), **cfg}))
    return m


def _fwd(m, inp, rows=slice(0, 1), ts=None, **kw):
    x, txt, t, rot = inp
    t = t[rows] if ts is None else ts
    return m(hidden_states=x[rows].to(DEV, torch.bfloat16), encoder_hidden_states=txt[rows].to(DEV, torch.bfloat16),
             timestep=t.to(DEV), image_rotary_emb=(rot[0].to(DEV), rot[1].to(DEV)), return_dict=False, **kw)[0]


def test_the_geometry_is_the_one_the_issue_asks_for():
    table = frame_window_ranges(FRAMES, TPF, 1, SINKS, prefix_rows=TEXT)
    assert L == 1358 and table.shape[0] == 6 and -(-L // 64) == 22 and L % 64 == 14
    assert round(ranges_density(table, L), 3) == 0.735 and not ranges_cover_all(table, L)
    assert table[0].tolist() == [[0, 22], [0, 0], [0, 0]]                                # it holds the text rows: dense
    assert len([1 for a, b in table[2].tolist() if b > a]) == 3


def test_windowed_forward_matches_the_restatement(setup):
    sd, sdb, inp, dense, windowed, gap = setup
    assert gap >= 5 * BOUND
    m = _model(sd, window_frames=1)
    out = _fwd(m, inp, id_frames=1)
    err, far = rel_rms(out, windowed), rel_rms(out, dense)
    print(f"windowed forward: rel-RMS {err:.3e} against the restatement, {far:.3e} against the dense restatement")
    record("cog_window_attention[tiny, bf16]", f"rel_rms vs the masked restatement (vs the dense one: {far:.3e})", err, BOUND)
    assert err < BOUND
    assert far > 3 * BOUND                                   # (and so it is not the dense model)
    assert m.window_attention_log == [(0, None, True)]
    # the dense model on the same weights is within the bound of the DENSE restatement
    assert rel_rms(_fwd(_model(sd), inp), dense) < BOUND
    # id_frames = 0: the last frame is no sink -- another mask, another result, against its own restatement
    out0 = _fwd(m, inp, id_frames=0)
    want0 = _ref(sdb, inp[0][:1], inp[1][:1], inp[2][:1], inp[3], R.layer_masks(2, FRAMES, TPF, TEXT, 1, (0,), live_rows=VIDEO_ROWS))
    assert not torch.equal(out0, out) and rel_rms(out0, want0) < BOUND
    assert torch.equal(_fwd(m, inp), out0)                   # (the default)


@pytest.mark.parametrize("fp8", [dict(), dict(smooth_k=True), dict(p_mode="exp2")], ids=["ramp", "ramp-smooth-k", "exp2"])
def test_fp8_attention_with_a_window_matches_the_restatement(setup, fp8):
    sd, sdb, inp, dense, _, _ = setup
    windowed = _ref(sdb, inp[0][:1], inp[1][:1], inp[2][:1], inp[3], R.layer_masks(2, FRAMES, TPF, TEXT, 1, SINKS))
    m = _model(sd, fp8=fp8, window_frames=1)
    assert m.fp8_attention                                   # (every block runs all rows: one table, q-blocks from row 0)
    out = _fwd(m, inp, id_frames=1)
    err, far = rel_rms(out, windowed), rel_rms(out, dense)
    print(f"fp8 attention {fp8} + window: rel-RMS {err:.3e} against the restatement, {far:.3e} against the dense restatement")
    record(f"cog_window_attention[tiny, fp8 attention {fp8}]", f"rel_rms vs the masked restatement (vs the dense one: {far:.3e})",
           err, FP8_BOUND)
    assert torch.isfinite(out.float()).all() and err < FP8_BOUND
    assert far > err                                         # farther from the dense restatement than from the windowed one
    # the switch reaches the kernel: not the bf16 windowed forward, not the dense fp8 forward
    assert not torch.equal(out, _fwd(_model(sd, window_frames=1), inp, id_frames=1))
    assert not torch.equal(out, _fwd(_model(sd, fp8=fp8), inp))


@pytest.mark.parametrize("fp8", [None, dict(), dict(smooth_k=True)], ids=["bf16", "fp8", "fp8-smooth-k"])
def test_an_all_covering_window_is_the_dense_forward_bit_for_bit(setup, fp8):
    sd, inp = setup[0], setup[2]
    want = _fwd(_model(sd, fp8=fp8), inp)
    m = _model(sd, fp8=fp8, window_frames=FRAMES)
    assert torch.equal(_fwd(m, inp, id_frames=1), want)
    m.disable_window_attention()
    m.enable_window_attention(WindowAttentionConfig(window_frames=1, skip_layers=(0, 1)))      # every layer dense
    assert torch.equal(_fwd(m, inp, id_frames=1), want)
    m.disable_window_attention()
    assert torch.equal(_fwd(m, inp, id_frames=1), want) and not m.is_window_attention_enabled


@pytest.mark.parametrize("skip", [(0,), (1,)])
def test_skip_layers_stay_dense(setup, skip):
    sd, sdb, inp, dense, windowed, _ = setup
    want = _ref(sdb, inp[0][:1], inp[1][:1], inp[2][:1], inp[3], R.layer_masks(2, FRAMES, TPF, TEXT, 1, SINKS, skip_layers=skip,
                                                                                    live_rows=VIDEO_ROWS))
    out = _fwd(_model(sd, window_frames=1, skip_layers=skip), inp, id_frames=1)
    err = rel_rms(out, want)
    print(f"skip_layers {skip}: rel-RMS {err:.3e} against the restatement; restatement vs all-windowed "
          f"{rel_rms(want, windowed):.3e}, vs dense {rel_rms(want, dense):.3e}")
    assert err < BOUND
    assert not torch.equal(out, _fwd(_model(sd, window_frames=1), inp, id_frames=1))


def test_live_frames_build_the_last_block_s_table_from_the_live_rows(setup):
    """under live_frames the last block's queries are rows [r0, r1) of the joint sequence: its table has q_rows = (r0, r1)"""
    sd, sdb, inp = setup[:3]
    live = (TEXT, TEXT + (FRAMES - 1) * TPF)                               # the caller drops the ID frame's prediction
    want = _ref(sdb, inp[0][:1], inp[1][:1], inp[2][:1], inp[3], R.layer_masks(2, FRAMES, TPF, TEXT, 1, SINKS, live_rows=live))
    m = _model(sd, window_frames=1)
    assert m.skip_dead_rows
    out = _fwd(m, inp, id_frames=1, live_frames=FRAMES - 1)
    err = rel_rms(out[:, :FRAMES - 1], want[:, :FRAMES - 1])
    print(f"live frames: rel-RMS {err:.3e} against the restatement")
    assert err < BOUND
    assert float(out[:, FRAMES - 1].abs().max()) == 0.0
    assert any(k[0] == "window" and k[6] == live for k in m._pos_cache)      # (the table of the live query rows was built)
    assert all(v is None or v.is_cuda for k, v in m._pos_cache.items() if k[0] == "window")
    m.reset_caches()
    assert not any(k[0] == "window" for k in m._pos_cache)


@pytest.mark.parametrize("fp8", [None, dict()], ids=["bf16", "fp8"])
def test_a_batch_of_two_equals_two_single_calls(setup, fp8):
    sd, inp = setup[0], setup[2]
    m = _model(sd, fp8=fp8, window_frames=1)
    both = _fwd(m, inp, rows=slice(0, 2), id_frames=1)
    for i in range(2):
        assert torch.equal(both[i:i + 1], _fwd(m, inp, rows=slice(i, i + 1), id_frames=1)), i
    assert not torch.equal(both[:1], both[1:])


def test_the_timestep_range_and_its_log(setup):
    sd, inp = setup[0], setup[2]
    clock = {"t": 999.0}
    dense, windowed = _model(sd), _model(sd, window_frames=1)
    m = _model(sd, window_frames=1, timestep_range=(100, 800), current_timestep_callback=lambda: clock["t"])
    seen = []
    for t in (999.0, 800.0, 500.0, 100.0, 50.0):                             # (800 and 100: the bounds are strict)
        clock["t"] = t
        ts = torch.tensor([t])
        out = _fwd(m, inp, ts=ts, id_frames=1)
        on = 100 < t < 800
        assert torch.equal(out, _fwd(windowed, inp, ts=ts, id_frames=1) if on else _fwd(dense, inp, ts=ts)), t
        seen.append(on)
    assert m.window_attention_log == [(i, t, on) for i, (t, on) in enumerate(zip((999.0, 800.0, 500.0, 100.0, 50.0), seen))]
    assert seen == [False, False, True, False, False]


def test_refusals(setup):
    from frameino_amd.attention_processor import MI355CogVideoXAttnProcessor
    sd, inp = setup[0], setup[2]
    m = _model(sd, window_frames=1)

    class Mine(MI355CogVideoXAttnProcessor):
        pass

    # what can only be seen by the forward: a processor installed afterwards
    m.transformer_blocks[0].attn1.set_processor(Mine())
    with pytest.raises(NotImplementedError, match="attention processor"):
        _fwd(m, inp, id_frames=1)
    m.transformer_blocks[0].attn1.set_processor(MI355CogVideoXAttnProcessor())
    m.reset_caches()
    with pytest.raises(ValueError, match="id_frames"):
        _fwd(m, inp, id_frames=FRAMES)
    assert _fwd(m, inp, id_frames=1).shape == (1, FRAMES, 2, R.LAT_H, R.LAT_W)
    m2 = _model(sd)
    m2.transformer_blocks[1].attn1.set_processor(Mine())
    with pytest.raises(NotImplementedError, match="attention processor"):
        m2.enable_window_attention(WindowAttentionConfig(1))
