"""FasterCache in the FrameINO Wan loop (the tiny golden pipeline of tests/test_wan_pipeline_gpu.py), Euler and UniPC: six steps
with `unconditional_batch_skip_range=2` and ranges that cover every timestep run the unconditional branch on steps 0, 2 and 4;
the latents equal, bit for bit, a loop this test drives by hand from the uncached model, ops.fastercache_delta /
ops.fastercache_apply and the sampler kernels, with the decisions and weights of tests/fastercache_ref.py; the three CFG
execution forms agree; a batch of two gives the two single calls; the graph loop is refused."""
import pytest
import torch

from frameino_amd.step_cache import FasterCacheConfig
from tests import fastercache_ref as R
from tests.test_wan_pipeline_gpu import _pipe

pytestmark = pytest.mark.gpu
DEV = "cuda"
STEPS = 6
ALL = (-1, 1001)
SAMPLERS = pytest.mark.parametrize("sampler", ["euler", "unipc"])


def _config(pipe, attention=None):
    return FasterCacheConfig(unconditional_batch_skip_range=2, unconditional_batch_timestep_skip_range=ALL,
                             spatial_attention_block_skip_range=attention, spatial_attention_timestep_skip_range=ALL,
                             low_frequency_weight_update_timestep_range=ALL, high_frequency_weight_update_timestep_range=(-1, 500),
                             attention_weight_callback=lambda m: 0.5, current_timestep_callback=lambda: pipe.current_timestep)


def _sampler(pipe, sampler):
    if sampler == "unipc":
        from frameino_amd.schedulers import UniPCMultistepScheduler
        pipe.scheduler = UniPCMultistepScheduler(flow_shift=5.0)
    return pipe


def _args(a):
    d = lambda k: a[k].to(DEV)          # noqa: E731
    return (d("latents0"), d("condition"), d("traj_latents"), d("id_latent"), d("mask"), d("prompt_embeds"), d("negative_embeds"),
            float(a["guidance"]))


def _by_hand(pipe, a, cfg):
    """the denoise loop with the unconditional-branch rule spelled out: the uncached model (batch 2 on a computing step, the
    "cond" element alone on a skipping one), the two ops, the sampler kernel"""
    tr = pipe.transformer
    o = tr.ops
    assert not tr.is_cache_enabled
    lat, cond, traj, idl, mask, pe, ne, guidance = _args(a)
    pipe.scheduler.set_timesteps(STEPS, device=DEV)
    timesteps = pipe.scheduler.timesteps
    st = pipe.make_state(lat, cond, traj, idl, mask, pe, ne, guidance)
    if st.unipc is not None:
        coefs = pipe.scheduler.coefs.to(DEV).clone()
        coefs[:, 0] = st.guidance
    else:
        dts = pipe.scheduler.dts.to(DEV)
    ts_dev = timesteps.to(DEV).float()
    live = {"live_rows": st.live_rows} if st.live_rows is not None else {}
    dl = dh = None
    al = ah = 1.0
    log = []
    for i in range(STEPS):
        t = float(timesteps[i])
        st.t_rows[1:2].copy_(ts_dev[i:i + 1])
        x = o.wan_model_input(st.lat, st.cond, st.idl, st.traj, tr.dtype, out=st.x)[None]
        kw = dict(timestep=None, return_dict=False, timestep_rows=(st.t_rows, st.sel), **live)
        skip = R.uncond_skips(i, t, dl is not None, cfg)
        with tr.cache_context("by-hand"):
            if skip:
                pc = tr(hidden_states=x, encoder_hidden_states=st.pe, **kw)[0][0]
                al, ah = R.weights(t, al, ah, cfg)
                pu = o.fastercache_apply(pc, dl, dh, al, ah)
            else:
                both = tr(hidden_states=x.expand(2, -1, -1, -1, -1), encoder_hidden_states=st.pe_ne, **kw)[0]
                pc, pu = both[0], both[1]
                dl, dh = o.fastercache_delta(pu, pc)
                al = ah = 1.0
        log += [("cond", i, t, True, True), ("uncond", i, t, not skip, not skip)]
        if st.unipc is not None:
            st.coef.copy_(coefs[i])
            o.cfg_unipc_step_(st.lat, *st.unipc, pc, pu, st.coef)
        else:
            st.dt.copy_(dts[i:i + 1])
            o.cfg_euler_step_(st.lat, pc, pu, st.guidance, st.dt, round_out=getattr(pipe.scheduler, "cast_output_to_model_dtype", True))
    return (1 - mask) * cond + mask * st.lat[None], log


@SAMPLERS
def test_six_steps_equal_the_loop_driven_by_hand(golden, sampler):
    pipe, a = _pipe(golden)
    _sampler(pipe, sampler)
    cfg = _config(pipe)
    want, want_log = _by_hand(pipe, a, cfg)
    pipe.use_hip_graph = False
    plain = pipe.denoise(*_args(a), STEPS)
    pipe.use_hip_graph = None
    pipe.transformer.enable_cache(cfg)
    forms = {}
    for name, batch_cfg, streams in (("batch_cfg", True, False), ("sequential", False, False), ("cfg_streams", False, True)):
        pipe.batch_cfg, pipe.cfg_streams = batch_cfg, streams
        forms[name] = (pipe.denoise(*_args(a), STEPS), list(pipe.transformer.cache_log))
    pipe.batch_cfg, pipe.cfg_streams = True, False
    got, log = forms["batch_cfg"]
    assert [e[3] for e in log if e[0] == "uncond"] == [True, False, True, False, True, False]
    assert log == want_log
    assert torch.equal(got, want)
    assert bool(torch.isfinite(got).all()) and got.shape == plain.shape and not torch.equal(got, plain)
    for name, (lat, lg) in forms.items():                      # batched CFG, two calls, two streams: equal latents and logs
        assert torch.equal(lat, got) and lg == log, name
    # a second call starts from fresh state and reproduces the first; the state is dropped at the end of __call__
    assert torch.equal(pipe.denoise(*_args(a), STEPS), got) and pipe.transformer.cache_log == log
    assert pipe.transformer._step_cache_states
    pipe.maybe_free_model_hooks()
    assert pipe.transformer._step_cache_states == {} and pipe.transformer.cache_log == log


def test_a_batch_of_two_equals_the_two_single_calls(golden):
    pipe, a = _pipe(golden)
    pipe.transformer.enable_cache(_config(pipe, attention=2))
    lat0, *rest = _args(a)
    lat1 = torch.randn(lat0.shape, generator=torch.Generator().manual_seed(5)).to(lat0)
    singles = [pipe.denoise(lat, *rest, STEPS) for lat in (lat0, lat1)]
    log = list(pipe.transformer.cache_log)
    both = pipe.denoise(torch.cat([lat0, lat1]), *rest, STEPS)
    assert torch.equal(both, torch.cat(singles)) and bool(torch.isfinite(both).all())
    assert pipe.transformer.cache_log == log                 # (the log of the last sample: every sample starts afresh)
    assert [e[3:] for e in log if e[0] == "uncond"] == [(True, True), (False, False)] * 3
    assert [e[3:] for e in log if e[0] == "cond"] == [(True, True), (True, False)] * 3


def test_graph_mode_is_refused_and_returns_after_disable(golden):
    pipe, a = _pipe(golden)
    never = pipe.denoise(*_args(a), STEPS)                   # default: graph replay, no cache
    pipe.transformer.enable_cache(_config(pipe))
    pipe.use_hip_graph = True
    with pytest.raises(RuntimeError, match="use_hip_graph=True with FasterCache"):
        pipe.denoise(*_args(a), STEPS)
    pipe.use_hip_graph = None
    pipe.denoise(*_args(a), STEPS)                           # None falls back to the eager loop
    pipe.transformer.disable_cache()
    assert torch.equal(pipe.denoise(*_args(a), STEPS), never)
