"""Guiders (frameino_amd/guiders.py) without a GPU: `coefficients()` -- the (A, B) form the kernel mirrors -- against the tensor
form of tests/guiders_ref.py in fp64, the configs' validation, the conventions of the degenerate inputs, the pipelines' switch
and its two refusals, and the calls both loops issue, seen by a recording stand-in for `ops`."""
import contextlib
import math
from types import SimpleNamespace

import pytest
import torch

from frameino_amd.guiders import (AdaptiveProjectedGuidanceConfig, CFGZeroStarConfig, GuidanceRescaleConfig,
                                  GuiderPipelineMixin, coefficients, kernel_args)
from tests import guiders_ref as R
from tests.guiders_ref import CONFIGS, degenerate_cases

def _ab_form(cfg, c, u, g, step):
    a, b = coefficients(cfg, R.moments(c, u), c.numel(), g, step)
    return a * c.double() + b * u.double()


@pytest.mark.parametrize("name", sorted(CONFIGS))
@pytest.mark.parametrize("n", [2, 1000, 4097])
def test_coefficients_equal_the_tensor_form(name, n):
    cfg = CONFIGS[name]
    c, u = R.family(n, seed=n)
    for g in (1.5, 5.0, 7.5):
        for step in (0, 1, 3):
            got, want = _ab_form(cfg, c, u, g, step), R.combine(cfg, c, u, g, step)
            scale = max(float(want.abs().max()), float(c.abs().max()))
            assert float((got - want).abs().max()) <= 1e-12 * scale, (name, n, g, step)
    # the clip of "apg_clipping" binds on the larger samples (|c - u| ~ 0.63 sqrt(n)), and not on two elements
    if name == "apg_clipping":
        dd = float(((c - u) ** 2).sum())
        assert (math.sqrt(dd) > 15.0) == (n >= 1000)


def test_zero_init_steps_and_plain_cfg():
    c, u = R.family(257, seed=1)
    m = R.moments(c, u)
    cfg = CFGZeroStarConfig(zero_init_steps=2)
    assert coefficients(cfg, m, 257, 5.0, 0) == (0.0, 0.0) and coefficients(cfg, m, 257, 5.0, 1) == (0.0, 0.0)
    a, b = coefficients(cfg, m, 257, 5.0, 2)
    assert a == 5.0 and b == (1.0 - 5.0) * m[4] / (m[3] + 1e-8)
    assert coefficients(CFGZeroStarConfig(zero_init_steps=0), m, 257, 5.0, 0) == (a, b)
    # guidance rescale with phi = 0 and APG without clip and with eta = 1 are plain CFG: A = g, B = 1 - g
    assert coefficients(GuidanceRescaleConfig(guidance_rescale=0.0), m, 257, 5.0) == (5.0, -4.0)
    a, b = coefficients(AdaptiveProjectedGuidanceConfig(norm_threshold=0.0, eta=1.0), m, 257, 5.0)
    assert a == 5.0 and b == -4.0


def test_config_validation():
    for bad in (-1, 1.5, True, None):
        with pytest.raises(ValueError, match="zero_init_steps"):
            CFGZeroStarConfig(zero_init_steps=bad)
    for cls in (CFGZeroStarConfig, AdaptiveProjectedGuidanceConfig, GuidanceRescaleConfig):
        for bad in (-0.1, 1.1, float("nan"), "0.5", None):
            with pytest.raises(ValueError, match="guidance_rescale"):
                cls(guidance_rescale=bad)
    for bad in (float("inf"), float("nan"), "15", None):
        with pytest.raises(ValueError, match="norm_threshold"):
            AdaptiveProjectedGuidanceConfig(norm_threshold=bad)
        with pytest.raises(ValueError, match="eta"):
            AdaptiveProjectedGuidanceConfig(eta=bad)
    with pytest.raises(ValueError, match="momentum"):
        AdaptiveProjectedGuidanceConfig(momentum="0.5")
    d = AdaptiveProjectedGuidanceConfig()
    assert (d.norm_threshold, d.eta, d.momentum, d.guidance_rescale) == (15.0, 1.0, None, 0.0)
    assert (CFGZeroStarConfig().zero_init_steps, CFGZeroStarConfig().guidance_rescale) == (1, 0.0)
    assert GuidanceRescaleConfig().guidance_rescale == 0.7
    assert kernel_args(d) == (2, 15.0, 1.0, 0.0) and kernel_args(CFGZeroStarConfig()) == (1, 0.0, 1.0, 0.0)
    assert kernel_args(GuidanceRescaleConfig()) == (0, 0.0, 1.0, 0.7)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_degenerate_inputs_follow_the_stated_conventions(name):
    cfg, g = CONFIGS[name], 5.0
    for case, (c, u) in degenerate_cases().items():
        a, b = coefficients(cfg, R.moments(c, u), c.numel(), g, step=1)
        assert math.isfinite(a) and math.isfinite(b), (name, case, a, b)
        want = R.combine(cfg, c, u, g, step=1)
        got = a * c + b * u
        assert bool(torch.isfinite(want).all()) and float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), \
            (name, case)
    plain = type(cfg)(**{**cfg.__dict__, "guidance_rescale": 0.0})
    phi = cfg.guidance_rescale
    c, u = degenerate_cases()["u=0"]
    a, b = coefficients(cfg, R.moments(c, u), 64, g, 1)
    if cfg.kind == 1:
        assert b == 0.0                                     # s = 0 / (0 + 1e-8): the unconditional branch drops out
    c, u = degenerate_cases()["c=0"]
    a, b = coefficients(cfg, R.moments(c, u), 64, g, 1)
    a0, b0 = coefficients(plain, R.moments(c, u), 64, g, 1)
    if cfg.kind == 2:
        s = min(1.0, cfg.norm_threshold / math.sqrt(R.moments(c, u)[3])) if cfg.norm_threshold > 0 else 1.0
        assert (a0, b0) == (g * s, 1.0 - g * s)             # Scc == 0: no projection (p = 0)
    if cfg.kind == 1:
        assert (a, b) == (g, 0.0)                           # s = 0, v = 0: var_p = 0 -> f = 1
    elif phi > 0:
        assert (a, b) == ((1.0 - phi) * a0, (1.0 - phi) * b0)     # var_c = 0 -> f = 0: the rescale shrinks v by 1 - phi
    c, u = degenerate_cases()["c==u"]
    a0, b0 = coefficients(plain, R.moments(c, u), 64, g, 1)
    if cfg.kind == 2:
        assert (a0, b0) == (g, 1.0 - g)                     # dd == 0: s = 1, and c - u has no part along c: v = u
    c, u = degenerate_cases()["constants"]
    a1, b1 = coefficients(cfg, R.moments(c, u), 64, g, 1)
    a0, b0 = coefficients(type(cfg)(**{**cfg.__dict__, "guidance_rescale": 0.0}), R.moments(c, u), 64, g, 1)
    assert (a1, b1) == (a0, b0)                             # every variance is 0: var_p <= 0 -> f = 1
    c, u = degenerate_cases()["n=1"]
    a1, b1 = coefficients(cfg, R.moments(c, u), 1, g, 1)
    a0, b0 = coefficients(type(cfg)(**{**cfg.__dict__, "guidance_rescale": 0.0}), R.moments(c, u), 1, g, 1)
    assert (a1, b1) == (a0, b0)                             # n < 2: f = 1


# ---------------------------------------------------------------------------------------------- the pipelines' switch
class _Recorder:
    """stands in for `ops`: records (name, zero flag at the time of the call | None)"""

    def __init__(self):
        self.calls, self.g_seen = [], []

    def guider_workspace_bytes(self, n):
        self.calls.append(("guider_workspace_bytes", None))
        return 40

    def wan_model_input(self, lat, cond, idl, traj, dtype, out=None):
        self.calls.append(("wan_model_input", None))
        return out

    def _coefs(self, name, zero_dev):
        self.calls.append((name, None if zero_dev is None else float(zero_dev)))

    def guider_coefs(self, pc, pu, gen_frames, args, g_dev, zero_dev, workspace, ab):
        assert pc.shape == pu.shape and workspace.numel() == 40 and ab.shape == (2,) and g_dev.shape == (1,)
        self.g_seen.append(float(g_dev))
        self._coefs("guider_coefs", zero_dev)

    def guider_coefs_rows(self, pred, n_lat, args, g_dev, zero_dev, workspace, ab):
        assert pred.shape[0] == 2 and workspace.numel() == 40 and ab.shape == (2,) and g_dev.shape == (1,)
        self.g_seen.append(float(g_dev))
        self._coefs("guider_coefs_rows", zero_dev)

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def call(*a, **k):
            self.calls.append((name, None))
            return a[0] if a else None
        return call


class _FakeWanDiT:
    dtype, device = torch.bfloat16, torch.device("cpu")
    config = SimpleNamespace(patch_size=(1, 2, 2))

    def __init__(self):
        self.ops = _Recorder()

    def cache_context(self, name):
        return contextlib.nullcontext()

    def __call__(self, hidden_states, **kw):
        b, c2 = hidden_states.shape[:2]
        return (torch.zeros((b, c2 // 2) + tuple(hidden_states.shape[2:]), dtype=self.dtype),)


def _wan(kind="euler"):
    from frameino_amd.pipeline_wan_i2v_motion_frameino import WanImageToVideoPipeline
    from frameino_amd.schedulers import FlowMatchEulerDiscreteScheduler, UniPCMultistepScheduler
    sched = FlowMatchEulerDiscreteScheduler(shift=5.0) if kind == "euler" else UniPCMultistepScheduler(flow_shift=5.0)
    return WanImageToVideoPipeline(scheduler=sched, transformer=_FakeWanDiT(), expand_timesteps=True)


def _wan_run(pipe, steps=4, guidance=5.0, negative=True):
    c, fg, h, w = 4, 3, 4, 6
    mask = torch.ones(1, 1, fg, h, w)
    mask[:, :, 0] = 0
    pipe.transformer.ops.calls.clear()
    pipe.transformer.ops.g_seen.clear()
    out = pipe.denoise(torch.randn(1, c, fg, h, w), torch.randn(1, c, fg, h, w), torch.randn(1, c, fg + 1, h, w),
                       torch.randn(1, c, 1, h, w), mask, torch.randn(1, 8, 16), torch.randn(1, 8, 16) if negative else None,
                       guidance, steps)
    assert out.shape == (1, c, fg, h, w)
    return [n for n in pipe.transformer.ops.calls]


@pytest.mark.parametrize("kind,plain,guided", [("euler", "cfg_euler_step_", "guided_euler_step_"),
                                               ("unipc", "cfg_unipc_step_", "guided_unipc_step_")])
def test_wan_loop_calls(kind, plain, guided):
    pipe = _wan(kind)
    today = [("wan_model_input", None), (plain, None)] * 4
    assert pipe.guider is None and _wan_run(pipe) == today
    cfg = CFGZeroStarConfig(zero_init_steps=2)
    assert pipe.set_guider(cfg) is pipe and pipe.guider is cfg
    calls = _wan_run(pipe)
    assert calls[0] == ("guider_workspace_bytes", None)
    want = []
    for i in range(4):
        want += [("wan_model_input", None), ("guider_coefs", 1.0 if i < 2 else 0.0), (guided, None)]
    assert calls[1:] == want and pipe.transformer.ops.g_seen == [5.0] * 4
    # the other guiders carry no zero-init flag
    pipe.set_guider(AdaptiveProjectedGuidanceConfig())
    assert _wan_run(pipe)[1:] == [("wan_model_input", None), ("guider_coefs", None), (guided, None)] * 4
    # guidance off (scale <= 1, or no negative prompt): today's calls, guider or not
    assert _wan_run(pipe, guidance=1.0) == today and _wan_run(pipe, negative=False) == today
    assert pipe.disable_guider() is pipe and pipe.guider is None and _wan_run(pipe) == today


class _FakeCogDiT:
    dtype = torch.bfloat16

    def __call__(self, hidden_states, **kw):
        nb, nf, c3 = hidden_states.shape[:3]
        return (torch.zeros((nb, nf, c3 // 3) + tuple(hidden_states.shape[3:]), dtype=self.dtype),)


def _cog_run(pipe, rec, steps=4, guidance=6.0, dynamic=False):
    f, c, h, w = 3, 2, 4, 4
    rec.calls.clear()
    rec.g_seen.clear()
    rot = (torch.zeros(1, 2), torch.zeros(1, 2))
    out = pipe.denoise(torch.randn(1, f, c, h, w), torch.randn(1, f, c, h, w), torch.randn(1, f, c, h, w),
                       torch.randn(1, 1, c, h, w), torch.randn(1, 8, 16), torch.randn(1, 8, 16), guidance, steps,
                       use_dynamic_cfg=dynamic, image_rotary_emb=rot, generator=torch.Generator().manual_seed(0))
    assert out.shape == (1, f, c, h, w)
    return list(rec.calls)


@pytest.mark.parametrize("kind,plain,guided", [("ddim", "cfg_vpred_step_", "guided_vpred_step_"),
                                               ("dpm", "cfg_dpm_step_", "guided_dpm_step_")])
def test_cog_loop_calls(kind, plain, guided, monkeypatch):
    import frameino_amd.pipeline_cogvideox_i2v_motion_frameino as mod
    from frameino_amd.schedulers import CogVideoXDDIMScheduler, CogVideoXDPMScheduler
    rec = _Recorder()
    monkeypatch.setattr(mod, "ops", rec)
    pipe = mod.CogVideoXImageToVideoPipeline(transformer=_FakeCogDiT(),
                                             scheduler=CogVideoXDDIMScheduler() if kind == "ddim" else CogVideoXDPMScheduler())
    today = [(plain, None)] * 4
    assert _cog_run(pipe, rec) == today
    pipe.set_guider(CFGZeroStarConfig(zero_init_steps=1))
    calls = _cog_run(pipe, rec)
    want = [("guider_workspace_bytes", None)]
    for i in range(4):
        want += [("guider_coefs_rows", 1.0 if i < 1 else 0.0), (guided, None)]
    assert calls == want and rec.g_seen == [6.0] * 4
    # use_dynamic_cfg: the guider reads the step's value where the coefficient row carries it
    _cog_run(pipe, rec, dynamic=True)
    ts = pipe.scheduler.timesteps.tolist()
    dyn = [1 + 6.0 * ((1 - math.cos(math.pi * ((4 - int(t)) / 4) ** 5.0)) / 2) for t in ts]
    assert rec.g_seen == [torch.tensor(g, dtype=torch.float32).item() for g in dyn] and len(set(rec.g_seen)) > 1
    assert _cog_run(pipe, rec, guidance=1.0) == today
    pipe.disable_guider()
    assert _cog_run(pipe, rec) == today


def test_the_stage1_pipelines_inherit_the_switch():
    from frameino_amd.pipeline_cogvideox_i2v_motion import CogVideoXImageToVideoPipeline as Cog1
    from frameino_amd.pipeline_wan_i2v_motion import WanImageToVideoPipeline as Wan1
    for cls in (Cog1, Wan1):
        assert issubclass(cls, GuiderPipelineMixin)


def test_refusals_come_before_any_launch():
    pipe = _wan()
    with pytest.raises(TypeError, match="set_guider takes one of"):
        pipe.set_guider({"zero_init_steps": 1})
    pipe.set_guider(AdaptiveProjectedGuidanceConfig(momentum=-0.5))
    with pytest.raises(NotImplementedError, match="momentum"):
        _wan_run(pipe)
    assert pipe.transformer.ops.calls == []
    pipe.set_guider(GuidanceRescaleConfig())
    pipe.parallel = SimpleNamespace(world=2)
    with pytest.raises(NotImplementedError, match="parallel plan"):
        _wan_run(pipe)
    assert pipe.transformer.ops.calls == []
    pipe.parallel = None
    pipe.disable_guider()
    pipe.parallel = SimpleNamespace(world=2)       # without a guider the plan is none of the guider's business
    assert pipe._guider_check() is None
    import frameino_amd.pipeline_cogvideox_i2v_motion_frameino as mod
    cog = mod.CogVideoXImageToVideoPipeline(transformer=_FakeCogDiT(), scheduler=None)
    cog.set_guider(AdaptiveProjectedGuidanceConfig(momentum=0.1))
    with pytest.raises(NotImplementedError, match="momentum"):
        cog.denoise(torch.zeros(1, 3, 2, 4, 4), None, None, None, None, None)
    cog.set_guider(CFGZeroStarConfig())
    cog.parallel = object()
    with pytest.raises(NotImplementedError, match="parallel plan"):
        cog.denoise(torch.zeros(1, 3, 2, 4, 4), None, None, None, None, None)
