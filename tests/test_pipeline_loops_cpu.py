"""The two sampler loops without a GPU: the ordered trace of everything a `denoise` does -- every `ops` call, every transformer
call (batch size, keyword names, the `cache_context` it ran under, `pipe.current_timestep` at that moment), the device slots of
every step, every callback, the returned latents -- against tests/golden/pipeline_loop_traces.json, which this same recorder wrote
on the commit before the loops were folded into frameino_amd/pipeline_base.py:

    python -m tests.test_pipeline_loops_cpu tests/golden/pipeline_loop_traces.json

Then what the shared driver adds: the captured graph is closed and `current_timestep` cleared when a step or a callback raises,
`StepGraph.close()` synchronises before it drops the graph, and the step-count warnings come from the cache policies.

The fakes use elementwise arithmetic only, so the latents are the same floats on every machine and are compared exactly; what comes
out of a scheduler's transcendental functions (timesteps, coefficient rows, noise) is compared to 1e-6."""
import contextlib
import json
import math
import os
import sys
import warnings
from types import SimpleNamespace

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pipeline_loop_traces.json")
C, FG, H, W, STEPS = 4, 3, 4, 6, 4


def _ramp(*shape, k=1):
    """a deterministic tensor in [-0.5, 0.5): exactly representable steps of 1/128, no generator"""
    n = math.prod(shape)
    return (((torch.arange(n, dtype=torch.float32) * (37 + 2 * k) + 11 * k) % 128) / 128 - 0.5).reshape(shape)


def _num(x):
    return None if x is None else float(x)


class _Ops:
    """stands in for `ops`: records every call by name; the step functions move the latents by a fixed elementwise rule"""

    def __init__(self, trace):
        self.trace = trace

    def guider_workspace_bytes(self, n):
        self.trace.append(["op", "guider_workspace_bytes"])
        return 40

    def wan_model_input(self, lat, cond, idl, traj, dtype, out=None):
        self.trace.append(["op", "wan_model_input"])
        c, fg = lat.shape[:2]
        out[:c, :fg] = lat
        out[:c, :1] = cond
        if idl is not None:
            out[:c, fg:] = idl
        out[c:] = traj
        return out

    def _coefs(self, name, g_dev, zero_dev):
        self.trace.append(["op", name, _num(g_dev), _num(zero_dev)])

    def guider_coefs(self, pc, pu, gen_frames, args, g_dev, zero_dev, workspace, ab):
        self._coefs("guider_coefs", g_dev, zero_dev)

    def guider_coefs_rows(self, pred, n_lat, args, g_dev, zero_dev, workspace, ab):
        self._coefs("guider_coefs_rows", g_dev, zero_dev)

    # Wan: lat [C, F, h, w], predictions [C, F + ids, h, w]
    def _wan(self, name, lat, pc, pu):
        self.trace.append(["op", name])
        for p, k in ((pc, 0.0625), (pu, 0.03125)):
            if p is not None:
                lat.add_(k * p[:, :lat.shape[1]].float())

    def cfg_euler_step_(self, lat, pc, pu, guidance, dt, round_out=True):
        self._wan("cfg_euler_step_", lat, pc, pu)

    def guided_euler_step_(self, lat, pc, pu, ab, dt, round_out=True):
        self._wan("guided_euler_step_", lat, pc, pu)

    def cfg_unipc_step_(self, lat, last, m0, m1, pc, pu, coef):
        self._wan("cfg_unipc_step_", lat, pc, pu)

    def guided_unipc_step_(self, lat, last, m0, m1, pc, pu, coef, ab):
        self._wan("guided_unipc_step_", lat, pc, pu)

    # Cog: lat [F, C, h, w], pred [nb, F + ids, C, h, w]
    def _cog(self, name, lat, pred, noise=None, **kw):
        self.trace.append(["op", name, _num(None if noise is None else noise.flatten()[0])] + sorted(kw.items()))
        for row, k in zip(pred, (0.0625, 0.03125)):
            lat.add_((k * row[:lat.shape[0]].float()).to(lat.dtype))

    def cfg_vpred_step_(self, lat, pred, coef, has_uncond=True):
        self._cog("cfg_vpred_step_", lat, pred, has_uncond=bool(has_uncond))

    def guided_vpred_step_(self, lat, pred, coef, ab):
        self._cog("guided_vpred_step_", lat, pred)

    def cfg_dpm_step_(self, lat, pred, x0_old, noise, coef, has_uncond=True):
        self._cog("cfg_dpm_step_", lat, pred, noise, has_uncond=bool(has_uncond))

    def guided_dpm_step_(self, lat, pred, x0_old, noise, coef, ab):
        self._cog("guided_dpm_step_", lat, pred, noise)


class _FakeDiT:
    dtype = torch.bfloat16

    def __init__(self, trace):
        self.trace, self.ctx, self.pipe = trace, None, None

    @contextlib.contextmanager
    def cache_context(self, name):
        old, self.ctx = self.ctx, name
        try:
            yield
        finally:
            self.ctx = old

    def _seen(self, what, batch, kw):
        self.trace.append([what, batch, sorted(kw), self.ctx, _num(self.pipe.current_timestep)])


class _FakeWanDiT(_FakeDiT):
    device = torch.device("cpu")
    config = SimpleNamespace(patch_size=(1, 2, 2))

    def __init__(self, trace):
        super().__init__(trace)
        self.ops = _Ops(trace)

    def _out(self, hidden_states, encoder_hidden_states):
        b, c = hidden_states.shape[0], hidden_states.shape[1] // 2
        e = encoder_hidden_states[:, 0, 0].float().view(-1, 1, 1, 1, 1)
        return (hidden_states[:, :c].float() * 0.5 + hidden_states[:, c:].float() * 0.25 + e * 0.125).to(self.dtype)

    def __call__(self, hidden_states, encoder_hidden_states=None, **kw):
        self._seen("dit", hidden_states.shape[0], dict(kw, hidden_states=None, encoder_hidden_states=None))
        return (self._out(hidden_states, encoder_hidden_states),)

    def forward_steps(self, hidden_states, encoder_hidden_states=None, **kw):
        for k in range(2):
            self._seen(f"dit_steps[{k}]", hidden_states.shape[0], dict(kw, hidden_states=None, encoder_hidden_states=None))
            yield
        self._seen("dit_steps[end]", hidden_states.shape[0], dict(kw, hidden_states=None, encoder_hidden_states=None))
        return (self._out(hidden_states, encoder_hidden_states),)


class _FakeCogDiT(_FakeDiT):
    def __call__(self, hidden_states, encoder_hidden_states=None, **kw):
        self._seen("dit", hidden_states.shape[0], dict(kw, hidden_states=None, encoder_hidden_states=None))
        c = hidden_states.shape[2] // 3
        e = encoder_hidden_states[:, 0, 0].float().view(-1, 1, 1, 1, 1)
        hs = hidden_states.float()
        return ((hs[:, :, :c] * 0.5 + hs[:, :, c:2 * c] * 0.25 + hs[:, :, 2 * c:] * 0.125 + e * 0.125).to(self.dtype),)


def _watch(pipe, trace, slots):
    """record the scheduler's `set_timesteps` and, in front of every step, the device slots the loop refreshed"""
    step, set_ts = pipe._step, pipe.scheduler.set_timesteps

    def _step(st):
        trace.append(["slots"] + [getattr(st, n).flatten().tolist() for n in slots(st)])
        return step(st)

    def set_timesteps(n, **kw):
        trace.append(["set_timesteps", n])
        return set_ts(n, **kw)
    pipe._step, pipe.scheduler.set_timesteps = _step, set_timesteps


def _callback(trace, replace=(), interrupt_at=None):
    def cb(pipe, i, t, kw):
        trace.append(["callback", i, _num(t), sorted(kw)])
        if interrupt_at == i:
            pipe._interrupt = True
        out = {}
        if "latents" in replace:
            out["latents"] = kw["latents"] * 0.5
        if "prompt_embeds" in replace:
            out["prompt_embeds"] = kw["prompt_embeds"] + 1.0
        return out
    return cb


# --------------------------------------------------------------------------------------------------------------- Wan
def _wan_pipe(trace, kind="euler", stage1=False):
    from frameino_amd.schedulers import FlowMatchEulerDiscreteScheduler, UniPCMultistepScheduler
    if stage1:
        from frameino_amd.pipeline_wan_i2v_motion import WanImageToVideoPipeline
    else:
        from frameino_amd.pipeline_wan_i2v_motion_frameino import WanImageToVideoPipeline
    sched = FlowMatchEulerDiscreteScheduler(shift=5.0) if kind == "euler" else UniPCMultistepScheduler(flow_shift=5.0)
    pipe = WanImageToVideoPipeline(scheduler=sched, transformer=_FakeWanDiT(trace), expand_timesteps=True)
    pipe.transformer.pipe = pipe
    pipe._current_timestep = None
    _watch(pipe, trace, lambda st: ("t_rows", "dt") if st.unipc is None else ("t_rows", "coef"))
    return pipe


def _wan_case(kind="euler", guidance=5.0, negative=True, ids=1, batch=1, stage1=False, setup=None, callback=None, inputs=("latents",)):
    trace = []
    pipe = _wan_pipe(trace, kind, stage1)
    plan = setup(pipe, trace) if setup else None
    mask = torch.ones(1, 1, FG, H, W)
    mask[:, :, 0] = 0
    cb = _callback(trace, **callback) if callback is not None else None
    out = pipe.denoise(_ramp(batch, C, FG, H, W, k=1), _ramp(1, C, FG, H, W, k=2), _ramp(1, C, FG + ids, H, W, k=3),
                       _ramp(1, C, ids, H, W, k=4) if ids else None, mask, _ramp(batch, 8, 16, k=5),
                       _ramp(batch, 8, 16, k=6) if negative else None, guidance, STEPS, None, cb, inputs)
    pipe._interrupt = False
    if plan is not None and hasattr(plan, "shards"):
        trace.append(["issue_streams", [s.issue_stream for s in plan.shards]])
    trace.append(["current_timestep", _num(pipe.current_timestep)])
    return {"trace": trace, "shape": list(out.shape), "latents": out.float().flatten().tolist()}


def _no_batch_cfg(pipe, trace):
    pipe.batch_cfg = False


def _guider(pipe, trace):
    from frameino_amd.guiders import CFGZeroStarConfig
    pipe.set_guider(CFGZeroStarConfig(zero_init_steps=2))


def _cfg_ways(idx):
    def setup(pipe, trace):
        def exchange_cfg(mine):
            trace.append(["exchange_cfg", idx])
            return (mine, mine * 0.5) if idx == 0 else (mine * 0.5, mine)
        pipe.parallel = SimpleNamespace(interleave=False, cfg_ways=2, cfg_idx=idx, world=2, rank=idx, token_group=None,
                                        cfg_group=None, exchange_cfg=exchange_cfg)
        return pipe.parallel
    return setup


def _interleaved(pipe, trace):
    pipe.parallel = SimpleNamespace(interleave=True, cfg_ways=1, world=2, rank=0, token_group=None, cfg_group=None,
                                    shards=[SimpleNamespace(issue_stream="stale"), SimpleNamespace(issue_stream="stale")])
    return pipe.parallel


ALL = ("latents", "prompt_embeds", "negative_prompt_embeds")
CASES = {}
for _kind in ("euler", "unipc"):
    CASES[f"wan-{_kind}-batch_cfg"] = lambda k=_kind: _wan_case(k)
    CASES[f"wan-{_kind}-sequential"] = lambda k=_kind: _wan_case(k, setup=_no_batch_cfg)
    CASES[f"wan-{_kind}-guidance1"] = lambda k=_kind: _wan_case(k, guidance=1.0)
    CASES[f"wan-{_kind}-no_negative"] = lambda k=_kind: _wan_case(k, negative=False)
    CASES[f"wan-{_kind}-guider"] = lambda k=_kind: _wan_case(k, setup=_guider)
CASES["wan-no_id"] = lambda: _wan_case(ids=0)
CASES["wan-callback-replaces"] = lambda: _wan_case(callback=dict(replace=("latents", "prompt_embeds")), inputs=ALL)
CASES["wan-callback-interrupts"] = lambda: _wan_case(callback=dict(interrupt_at=1))
CASES["wan-batch2"] = lambda: _wan_case(batch=2)
CASES["wan-batch2-unipc-callback"] = lambda: _wan_case("unipc", batch=2, callback=dict(replace=("latents",)))
CASES["wan-cfg_ways2-cond"] = lambda: _wan_case(setup=_cfg_ways(0))
CASES["wan-cfg_ways2-uncond"] = lambda: _wan_case(setup=_cfg_ways(1))
CASES["wan-interleaved"] = lambda: _wan_case(setup=_interleaved)
CASES["wan-interleaved-guidance1"] = lambda: _wan_case(setup=_interleaved, guidance=1.0)
CASES["wan-stage1"] = lambda: _wan_case(ids=0, stage1=True)


# --------------------------------------------------------------------------------------------------------------- Cog
def _cog_case(monkeypatch, kind="ddim", guidance=6.0, ids=1, batch=1, stage1=False, dynamic=False, guider=False, callback=None,
              generators=False, rot=True):
    import frameino_amd.pipeline_cogvideox_i2v_motion_frameino as mod
    from frameino_amd.schedulers import CogVideoXDDIMScheduler, CogVideoXDPMScheduler
    trace = []
    monkeypatch.setattr(mod, "ops", _Ops(trace))
    cls = mod.CogVideoXImageToVideoPipeline
    if stage1:
        from frameino_amd.pipeline_cogvideox_i2v_motion import CogVideoXImageToVideoPipeline as cls
    pipe = cls(transformer=_FakeCogDiT(trace), scheduler=CogVideoXDDIMScheduler() if kind == "ddim" else CogVideoXDPMScheduler())
    pipe.transformer.pipe = pipe
    _watch(pipe, trace, lambda st: ("t", "coef"))
    if guider:
        from frameino_amd.guiders import CFGZeroStarConfig
        pipe.set_guider(CFGZeroStarConfig(zero_init_steps=1))
    f, c, h, w = FG, 2, 4, 4
    if generators:
        gen = [torch.Generator().manual_seed(7 + i) for i in range(batch)]
    else:
        gen = torch.Generator().manual_seed(0)
    cb = _callback(trace, **callback) if callback is not None else None
    args = [_ramp(batch, f, c, h, w, k=1), _ramp(1, f, c, h, w, k=2), _ramp(1, f, c, h, w, k=3)]
    if not stage1:
        args.append(_ramp(1, 1, c, h, w, k=4) if ids else None)
    out = pipe.denoise(*args, _ramp(batch, 8, 16, k=5), _ramp(batch, 8, 16, k=6), guidance, STEPS, use_dynamic_cfg=dynamic,
                       image_rotary_emb=(torch.zeros(1, 2), torch.zeros(1, 2)) if rot else None, callback_on_step_end=cb,
                       generator=gen)
    trace.append(["current_timestep", _num(pipe.current_timestep)])
    return {"trace": trace, "shape": list(out.shape), "latents": out.float().flatten().tolist()}


for _kind in ("ddim", "dpm"):
    CASES[f"cog-{_kind}-cfg"] = lambda mp, k=_kind: _cog_case(mp, k)
    CASES[f"cog-{_kind}-guidance1"] = lambda mp, k=_kind: _cog_case(mp, k, guidance=1.0)
    CASES[f"cog-{_kind}-no_id"] = lambda mp, k=_kind: _cog_case(mp, k, ids=0)
    CASES[f"cog-{_kind}-guider"] = lambda mp, k=_kind: _cog_case(mp, k, guider=True)
CASES["cog-dynamic_cfg"] = lambda mp: _cog_case(mp, dynamic=True)
CASES["cog-dynamic_cfg-guider"] = lambda mp: _cog_case(mp, dynamic=True, guider=True)
CASES["cog-callback-replaces"] = lambda mp: _cog_case(mp, callback=dict(replace=("latents",)))
CASES["cog-callback-interrupts"] = lambda mp: _cog_case(mp, callback=dict(interrupt_at=1))
CASES["cog-batch2-generators"] = lambda mp: _cog_case(mp, "dpm", batch=2, generators=True)
CASES["cog-stage1"] = lambda mp: _cog_case(mp, stage1=True)
CASES["cog-stage1-dpm"] = lambda mp: _cog_case(mp, "dpm", stage1=True)


def _run_case(name, monkeypatch):
    return json.loads(json.dumps(CASES[name](monkeypatch) if name.startswith("cog") else CASES[name]()))


def _same(got, want, where):
    """floats to 1e-6 (what a scheduler's exp / cos / randn gave), everything else exactly"""
    if isinstance(want, list):
        assert isinstance(got, list) and len(got) == len(want), where
        for i, (g, w) in enumerate(zip(got, want)):
            _same(g, w, f"{where}[{i}]")
    elif isinstance(want, float) and isinstance(got, float):
        assert got == pytest.approx(want, rel=1e-6, abs=1e-9), where
    else:
        assert got == want, where


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_has_every_case(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_loop_trace(name, golden, monkeypatch):
    got, want = _run_case(name, monkeypatch), golden[name]
    assert got["shape"] == want["shape"]
    _same(got["trace"], want["trace"], name)
    assert got["latents"] == want["latents"]                # exact: the same launches in the same order on the same data
    assert any(e[0] == "dit" or e[0].startswith("dit_steps") for e in got["trace"])


# ------------------------------------------------------------------------------------------- cleanup when the loop fails
class _SpyGraph:
    made = []

    def __init__(self, step_fn, mode, capturable, total_steps, error_mode="global"):
        self.step_fn, self.closed, self.ran = step_fn, 0, 0
        _SpyGraph.made.append(self)

    def step(self):
        self.ran += 1
        self.step_fn()

    def close(self):
        self.closed += 1


class _Boom(Exception):
    pass


def _failing(pipe, how):
    """-> the callback to pass.  `how`: "step" (the step function raises at step 2) or "callback" (the callback does)"""
    if how == "step":
        step, n = pipe._step, [0]

        def _step(st):
            n[0] += 1
            if n[0] == 3:
                raise _Boom("step 2")
            return step(st)
        pipe._step = _step
        return None

    def cb(pipe_, i, t, kw):
        if i == 2:
            raise _Boom("callback at step 2")
        return {}
    return cb


def _wan_denoise(pipe, cb):
    mask = torch.ones(1, 1, FG, H, W)
    mask[:, :, 0] = 0
    return pipe.denoise(_ramp(1, C, FG, H, W, k=1), _ramp(1, C, FG, H, W, k=2), _ramp(1, C, FG + 1, H, W, k=3),
                        _ramp(1, C, 1, H, W, k=4), mask, _ramp(1, 8, 16, k=5), _ramp(1, 8, 16, k=6), 5.0, STEPS, None, cb)


def _cog_denoise(pipe, cb):
    f, c, h, w = FG, 2, 4, 4
    return pipe.denoise(_ramp(1, f, c, h, w, k=1), _ramp(1, f, c, h, w, k=2), _ramp(1, f, c, h, w, k=3), _ramp(1, 1, c, h, w, k=4),
                        _ramp(1, 8, 16, k=5), _ramp(1, 8, 16, k=6), 6.0, STEPS,
                        image_rotary_emb=(torch.zeros(1, 2), torch.zeros(1, 2)), callback_on_step_end=cb)


def _cog_pipe(trace, monkeypatch):
    import frameino_amd.pipeline_cogvideox_i2v_motion_frameino as mod
    from frameino_amd.schedulers import CogVideoXDDIMScheduler
    monkeypatch.setattr(mod, "ops", _Ops(trace))
    pipe = mod.CogVideoXImageToVideoPipeline(transformer=_FakeCogDiT(trace), scheduler=CogVideoXDDIMScheduler())
    pipe.transformer.pipe = pipe
    return pipe


@pytest.mark.parametrize("how", ["step", "callback"])
@pytest.mark.parametrize("which", ["wan", "cog"])
def test_a_failing_loop_closes_the_graph_and_clears_the_timestep(which, how, monkeypatch):
    from frameino_amd import graph_step
    monkeypatch.setattr(graph_step, "StepGraph", _SpyGraph)
    monkeypatch.setattr(_SpyGraph, "made", [])
    trace = []
    pipe = _wan_pipe(trace) if which == "wan" else _cog_pipe(trace, monkeypatch)
    run = _wan_denoise if which == "wan" else _cog_denoise
    with pytest.raises(_Boom, match="step 2"):
        run(pipe, _failing(pipe, how))
    assert len(_SpyGraph.made) == 1
    spy = _SpyGraph.made[0]
    assert spy.ran == 3 and spy.closed == 1
    assert pipe.current_timestep is None
    # and a loop that ends well closes it once, too
    pipe2 = _wan_pipe(trace) if which == "wan" else _cog_pipe(trace, monkeypatch)
    run(pipe2, None)
    assert len(_SpyGraph.made) == 2 and _SpyGraph.made[1].ran == STEPS and _SpyGraph.made[1].closed == 1
    assert pipe2.current_timestep is None


def test_stepgraph_close_synchronises_before_it_drops_the_graph(monkeypatch):
    from frameino_amd.graph_step import StepGraph
    sg = StepGraph(lambda: None, None, False, 4)
    sg.graph = object()
    alive = []
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: alive.append(sg.graph is not None))
    sg.close()
    assert alive == [True] and sg.graph is None
    sg.close()                                        # nothing captured (any more): nothing to wait for
    assert alive == [True]


# ------------------------------------------------------------------------- what the loop asks of the cache policy
class _CachedWanDiT(_FakeWanDiT):
    is_cache_enabled = True

    def _reset_stateful_cache(self):
        self.trace.append(["reset"])


def _cached_run(policy, config, steps):
    trace = []
    pipe = _wan_pipe(trace)
    pipe.transformer.__class__ = _CachedWanDiT
    pipe.transformer._step_cache_policy, pipe.transformer._step_cache_config = policy, config
    mask = torch.ones(1, 1, FG, H, W)
    mask[:, :, 0] = 0
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        pipe.denoise(_ramp(1, C, FG, H, W, k=1), _ramp(1, C, FG, H, W, k=2), _ramp(1, C, FG + 1, H, W, k=3),
                     _ramp(1, C, 1, H, W, k=4), mask, _ramp(1, 8, 16, k=5), _ramp(1, 8, 16, k=6), 5.0, steps)
    return [str(w.message) for w in seen], trace


MAG_TEXT = ("MagCache: this call runs 4 steps, the config says num_inference_steps=6; its curve (`mag_ratios`, resampled to 6 "
            "entries) is misaligned with the loop and a context starts over after 6 forwards.  Build the config with the call's "
            "step count.")
RAS_TEXT = ("region-adaptive sampling: this call runs 4 steps, the config says num_inference_steps=6; its full steps at the end "
            "sit at forwards 6 - full_steps_at_end and later, and every forward from 6 on is full.  Build the config with the "
            "call's step count.")


@pytest.mark.parametrize("policy,text", [("_MagCachePolicy", MAG_TEXT), ("_RegionAdaptivePolicy", RAS_TEXT)])
def test_step_count_warnings_come_from_the_policy(policy, text):
    from frameino_amd import step_cache as S
    policy = getattr(S, policy)
    seen, _ = _cached_run(policy, SimpleNamespace(num_inference_steps=6), 4)
    assert seen == [text]                                         # once per denoise, today's words
    seen, _ = _cached_run(policy, SimpleNamespace(num_inference_steps=4), 4)
    assert seen == []                                             # only when the counts differ
    # the other caches say nothing
    for other in (S._FirstBlockPolicy, S._PabPolicy, S._TaylorSeerPolicy, S._FasterCachePolicy):
        seen, _ = _cached_run(other, SimpleNamespace(num_inference_steps=6), 4)
        assert seen == []


def test_only_fastercache_reads_the_timestep_on_the_host():
    from frameino_amd import step_cache as S
    assert [p.name for p in S._POLICIES.values() if p.reads_timestep_on_host] == ["FasterCacheConfig"]
    # ... and under it `current_timestep` is the host copy of the schedule: the same values, step by step
    _, cached = _cached_run(S._FasterCachePolicy, SimpleNamespace(), 4)
    _, plain = _cached_run(S._PabPolicy, SimpleNamespace(), 4)
    ts = [e[4] for e in cached if e[0] == "dit"]
    assert ts == [e[4] for e in plain if e[0] == "dit"] and len(ts) == 4 and None not in ts


# --------------------------------------------------------------------------------------- the shared VideoProcessor
def test_video_processor_takes_a_list_of_images_and_returns_pil():
    import numpy as np
    import PIL.Image
    from frameino_amd.pipeline_base import VideoProcessor
    from frameino_amd.pipeline_wan_i2v_motion_frameino import VideoProcessor as FromWan
    assert FromWan is VideoProcessor
    vp = VideoProcessor()
    rgb = [PIL.Image.fromarray(((np.arange(8 * 6 * 3).reshape(8, 6, 3) * (3 + k)) % 256).astype("uint8")) for k in range(2)]
    one = [vp.preprocess(im, height=16, width=32) for im in rgb]
    assert one[0].shape == (1, 3, 16, 32) and float(one[0].min()) >= -1.0 and float(one[0].max()) <= 1.0
    assert torch.equal(vp.preprocess(rgb, height=16, width=32), torch.cat(one))          # stacked, each as the single call
    assert vp.preprocess(rgb[0].convert("L"), height=16, width=32).shape == (1, 1, 16, 32)
    t = torch.rand(3, 4, 4)
    assert torch.equal(vp.preprocess(t, 4, 4), 2.0 * t[None] - 1.0) and torch.equal(vp.preprocess(t - 0.5, 4, 4), (t - 0.5)[None])
    with pytest.raises(ValueError, match="`image` has to be of type"):
        vp.preprocess("a.png", 4, 4)
    video = torch.rand(2, 3, 5, 4, 6) * 2 - 1                                             # [B, C, F, H, W]
    arr = vp.postprocess_video(video, "np")
    pil = vp.postprocess_video(video, "pil")
    assert arr.shape == (2, 5, 4, 6, 3) and tuple(vp.postprocess_video(video, "pt").shape) == (2, 5, 3, 4, 6)
    assert len(pil) == 2 and len(pil[0]) == 5 and pil[1][4].size == (6, 4)
    assert np.array_equal(np.asarray(pil[1][4]), (arr[1, 4] * 255).round().astype("uint8"))
    with pytest.raises(ValueError, match="unsupported output_type"):
        vp.postprocess_video(video, "mp4")


if __name__ == "__main__":
    # writes the golden file: run on the commit whose behaviour is the reference
    class _Patch:
        def setattr(self, obj, name, value):
            setattr(obj, name, value)
    with open(sys.argv[1], "w") as f:
        json.dump({n: _run_case(n, _Patch()) for n in sorted(CASES)}, f, separators=(",", ":"))
        f.write("\n")
