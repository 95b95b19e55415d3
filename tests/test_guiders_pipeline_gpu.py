"""Guiders in both sampler loops, on the tiny golden pipelines (Wan: Euler and UniPC; CogVideoX: DDIM, DDIM with
`use_dynamic_cfg`, DPM), 3 steps, every guider:

  * the hipGraph loop (step 0 eager, step 1 captured, step 2 replayed) equals the eager loop bit for bit;
  * the eager loop against a host loop over the same transformer whose combine is tests/guiders_ref.py in fp64 (tensor form)
    and whose sampler step is the coefficient row's linear form in fp64 (`HostGuidedOps`), within the bound the pipeline's own
    HIP-vs-oracle test states: rel-RMS 5e-2 for Wan (tests/test_wan_pipeline_gpu.py), 6e-2 for CogVideoX
    (tests/test_cog_model_gpu.py);
  * the result differs from plain CFG;
one composition run, a guider with first-block caching; and, on Wan, that a guided call does not depend on whether the transformer
honours the loop's `live_rows` (the guider's moments cover the first frame: tests that a no-op callback, which switches `live_rows`
off, and `skip_dead_rows = False` change nothing)."""
import pytest
import torch

from frameino_amd.guiders import AdaptiveProjectedGuidanceConfig, CFGZeroStarConfig, GuidanceRescaleConfig
from tests.guiders_ref import HostGuidedOps
from tests.parity import rel_rms

pytestmark = pytest.mark.gpu
DEV = "cuda"
STEPS = 3
GUIDERS = {
    "zero_star": CFGZeroStarConfig(zero_init_steps=1),
    # (the flag is 1 at the eager step 0 AND at the captured step 1, 0 at the replayed step 2: the replay has to read it anew)
    "zero_star_2": CFGZeroStarConfig(zero_init_steps=2, guidance_rescale=0.4),
    "apg": AdaptiveProjectedGuidanceConfig(norm_threshold=2.0, eta=0.5, guidance_rescale=0.3),
    "rescale": GuidanceRescaleConfig(guidance_rescale=0.7),
}


# ------------------------------------------------------------------------------------------------------------------- Wan
@pytest.fixture(scope="module")
def wan(golden):
    from tests.test_wan_pipeline_gpu import _pipe
    return _pipe(golden)


def _wan_run(pipe, a, graph):
    pipe.use_hip_graph = graph
    d = lambda k: a[k].to(DEV)          # noqa: E731
    try:
        return pipe.denoise(d("latents0"), d("condition"), d("traj_latents"), d("id_latent"), d("mask"), d("prompt_embeds"),
                            d("negative_embeds"), float(a["guidance"]), STEPS)
    finally:
        pipe.use_hip_graph = None


def _wan_scheduler(kind):
    from frameino_amd.schedulers import FlowMatchEulerDiscreteScheduler, UniPCMultistepScheduler
    return FlowMatchEulerDiscreteScheduler(shift=5.0) if kind == "euler" else UniPCMultistepScheduler(flow_shift=5.0)


@pytest.fixture(scope="module")
def wan_plain(wan):
    pipe, a = wan
    out = {}
    for kind in ("euler", "unipc"):
        pipe.scheduler = _wan_scheduler(kind)
        pipe.disable_guider()
        out[kind] = _wan_run(pipe, a, False)
    return out


@pytest.mark.parametrize("kind", ["euler", "unipc"])
@pytest.mark.parametrize("name", sorted(GUIDERS))
def test_wan_loop(wan, wan_plain, kind, name):
    pipe, a = wan
    pipe.scheduler = _wan_scheduler(kind)
    pipe.set_guider(GUIDERS[name])
    real = pipe.transformer.ops
    try:
        eager = _wan_run(pipe, a, False)
        graphed = _wan_run(pipe, a, True)               # True: a failed capture is an error
        assert torch.equal(eager, graphed)
        pipe.transformer.ops = HostGuidedOps(real, GUIDERS[name])
        host = _wan_run(pipe, a, False)
    finally:
        pipe.transformer.ops = real
        pipe.disable_guider()
    assert bool(torch.isfinite(eager).all())
    r = rel_rms(eager, host)
    print(f"wan {kind} {name}: rel_rms vs the fp64 host loop {r:.3e}; vs plain CFG {rel_rms(eager, wan_plain[kind]):.3e}")
    assert r < 5e-2, r
    assert not torch.equal(eager, wan_plain[kind])
    assert torch.equal(eager[:, :, 0].cpu(), a["condition"][:, :, 0])          # the re-imposed first frame is exact


@pytest.mark.parametrize("kind", ["euler", "unipc"])
def test_wan_guided_call_does_not_depend_on_live_rows(wan, kind):
    """Plain CFG never reads the first frame's prediction (the frame is re-imposed from the condition), so the loop lets the
    transformer skip it (`live_rows`, honoured under `skip_dead_rows`).  A guider reads it through its moments: under a guider the
    loop keeps only the ID frames dead, and the latents are the same bits whether or not the rows are skipped."""
    pipe, a = wan
    tr = pipe.transformer
    pipe.scheduler = _wan_scheduler(kind)
    assert tr.skip_dead_rows and len(tr.blocks) > 1                 # the configuration under which dead rows come back as zeros
    d = lambda k: a[k].to(DEV)          # noqa: E731
    assert bool((d("mask")[0, 0, 0] == 0).all())                    # the first frame is dead for plain CFG
    for name in ("zero_star", "apg"):
        pipe.set_guider(GUIDERS[name])
        try:
            base = _wan_run(pipe, a, False)
            tr.skip_dead_rows = False
            assert torch.equal(_wan_run(pipe, a, False), base), (name, "skip_dead_rows")
            tr.skip_dead_rows = True
            seen = []
            with_cb = pipe.denoise(d("latents0"), d("condition"), d("traj_latents"), d("id_latent"), d("mask"),
                                   d("prompt_embeds"), d("negative_embeds"), float(a["guidance"]), STEPS,
                                   callback_on_step_end=lambda p, i, t, kw: seen.append(i) or {})
            assert seen == list(range(STEPS)) and torch.equal(with_cb, base), (name, "callback")
        finally:
            tr.skip_dead_rows = True
            pipe.disable_guider()


def test_wan_guider_with_first_block_caching(wan):
    """the guider sits after the model: with a cache that recomputes every step the latents are the guider's own, bit for bit;
    the cached loop is eager, and asking for the graph is refused as without a guider"""
    from frameino_amd.step_cache import FirstBlockCacheConfig
    pipe, a = wan
    pipe.scheduler = _wan_scheduler("euler")
    pipe.set_guider(GUIDERS["zero_star"])
    try:
        alone = _wan_run(pipe, a, False)
        pipe.transformer.enable_cache(FirstBlockCacheConfig(threshold=0.0))
        assert torch.equal(_wan_run(pipe, a, None), alone)
        pipe.transformer.disable_cache()
        pipe.transformer.enable_cache(FirstBlockCacheConfig(threshold=0.2))
        out = _wan_run(pipe, a, None)
        assert bool(torch.isfinite(out).all()) and len(pipe.transformer.cache_log) > 0
        with pytest.raises(RuntimeError, match="use_hip_graph=True"):
            _wan_run(pipe, a, True)
    finally:
        pipe.transformer.disable_cache()
        pipe.disable_guider()


# ------------------------------------------------------------------------------------------------------------- CogVideoX
@pytest.fixture(scope="module")
def cog(golden):
    from tests.test_cog_model_gpu import _cog_pipe
    pipe, a, _ = _cog_pipe(golden)
    return pipe, a


def _cog_scheduler(kind):
    from frameino_amd.schedulers import CogVideoXDDIMScheduler, CogVideoXDPMScheduler
    return CogVideoXDPMScheduler() if kind == "dpm" else CogVideoXDDIMScheduler()


def _cog_run(pipe, a, graph, kind):
    pipe.use_hip_graph = graph
    d = lambda k: a[k].to(DEV)          # noqa: E731
    try:
        return pipe.denoise(d("latents0"), d("image_latents"), d("traj_latents"), d("id_latent"), d("prompt_embeds"),
                            d("negative_embeds"), float(a["guidance"]), STEPS, use_dynamic_cfg=(kind == "ddim_dynamic"),
                            generator=torch.Generator().manual_seed(5))
    finally:
        pipe.use_hip_graph = None


@pytest.mark.parametrize("kind", ["ddim", "ddim_dynamic", "dpm"])
@pytest.mark.parametrize("name", sorted(GUIDERS))
def test_cog_loop(cog, kind, name, monkeypatch):
    import frameino_amd.pipeline_cogvideox_i2v_motion_frameino as mod
    pipe, a = cog
    pipe.scheduler = _cog_scheduler(kind)
    pipe.disable_guider()
    plain = _cog_run(pipe, a, False, kind)
    pipe.set_guider(GUIDERS[name])
    try:
        eager = _cog_run(pipe, a, False, kind)
        graphed = _cog_run(pipe, a, True, kind)
        assert torch.equal(eager, graphed)
        monkeypatch.setattr(mod, "ops", HostGuidedOps(mod.ops, GUIDERS[name]))
        host = _cog_run(pipe, a, False, kind)
    finally:
        pipe.disable_guider()
    assert bool(torch.isfinite(eager.float()).all())
    r = rel_rms(eager, host)
    print(f"cog {kind} {name}: rel_rms vs the fp64 host loop {r:.3e}; vs plain CFG {rel_rms(eager, plain):.3e}")
    assert r < 6e-2, r
    assert not torch.equal(eager, plain)
