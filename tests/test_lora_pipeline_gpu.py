"""LoRA through the pipelines (tiny Wan / CogVideoX setups of tests/test_wan_pipeline_gpu.py and tests/test_cog_model_gpu.py):
load_lora_weights from a folder, hipGraph replay == eager with an adapter merged, call scales between calls, the loop guard
against LoRA changes from a step callback, fuse_lora / unfuse_lora."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _wan(golden):
    from tests.test_wan_pipeline_gpu import _pipe
    pipe, a = _pipe(golden)
    d = lambda k: a[k].to(DEV)          # noqa: E731

    def run(**kw):
        return pipe.denoise(d("latents0"), d("condition"), d("traj_latents"), d("id_latent"), d("mask"), d("prompt_embeds"),
                            d("negative_embeds"), float(a["guidance"]), int(a["steps"]), **kw)
    return pipe, run


def _cog(golden):
    from tests.test_cog_model_gpu import _cog_pipe
    pipe, a, _ = _cog_pipe(golden)
    d = lambda k: a[k].to(DEV)          # noqa: E731

    def run(**kw):
        return pipe.denoise(d("latents0"), d("image_latents"), d("traj_latents"), d("id_latent"), d("prompt_embeds"),
                            d("negative_embeds"), float(a["guidance"]), 3, generator=torch.Generator().manual_seed(3), **kw)
    return pipe, run


def _adapter(model, seed=5, rank=4):
    """a seeded diffusers-layout adapter on every block linear of the transformer (and nothing else)"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, p in model.named_parameters():
        if name.startswith(("blocks.", "transformer_blocks.")) and name.endswith(".weight") and p.dim() == 2:
            mod = name[:-len(".weight")]
            sd[f"transformer.{mod}.lora_A.weight"] = torch.randn(rank, p.shape[1], generator=g) / rank ** 0.5
            sd[f"transformer.{mod}.lora_B.weight"] = torch.randn(p.shape[0], rank, generator=g) * p.float().std().item()
    assert sd
    return sd


@pytest.fixture(params=["wan", "cog"])
def setup(request, golden):
    return (_wan if request.param == "wan" else _cog)(golden)


def test_load_from_folder_graph_replay_and_call_scales(setup, tmp_path):
    from safetensors.torch import save_file
    pipe, run = setup
    pipe.use_hip_graph = False
    base = run()
    sd = _adapter(pipe.transformer)
    save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / "pytorch_lora_weights.safetensors"))
    assert pipe.load_lora_weights(str(tmp_path), adapter_name="a") == "a"
    assert pipe.get_active_adapters() == ["a"] and pipe.get_list_adapters() == {"transformer": ["a"]}
    eager = run()
    assert not torch.equal(eager, base)
    pipe.use_hip_graph = True
    assert torch.equal(run(), eager)
    # two calls in a row at scales 1.0 and 0.3: each equals a fresh pipe loaded at that scale (alpha = 0.3 r)
    s03 = run(attention_kwargs={"scale": 0.3})
    assert torch.equal(run(attention_kwargs={"scale": 1.0}), eager)
    pipe.unload_lora_weights()
    assert torch.equal(run(), base)
    rank = next(v for k, v in sd.items() if k.endswith("lora_A.weight")).shape[0]
    sd_alpha = dict(sd)
    sd_alpha.update({k.replace(".lora_A.weight", ".alpha"): torch.tensor(0.3 * rank) for k in sd if k.endswith("lora_A.weight")})
    pipe.load_lora_weights(sd_alpha)
    assert torch.equal(run(), s03)


def test_loop_guard_and_fuse(setup):
    pipe, run = setup
    pipe.use_hip_graph = False
    pipe.load_lora_weights(_adapter(pipe.transformer), adapter_name="a")

    def cb(p, *args):
        p.set_adapters(["a"], [0.5])
        return args[-1]
    with pytest.raises(RuntimeError, match="denoise loop"):
        run(callback_on_step_end=cb)
    full = run()
    half = run(attention_kwargs={"scale": 0.5})
    # fuse_lora(0.5) pins the scale: a later call scale leaves the fused adapter alone
    pipe.fuse_lora(lora_scale=0.5)
    assert torch.equal(run(), half)
    assert torch.equal(run(attention_kwargs={"scale": 1.0}), half)
    pipe.unfuse_lora()
    assert torch.equal(run(), full)
    pipe.disable_lora()
    off = run()
    pipe.enable_lora()
    assert torch.equal(run(), full) and not torch.equal(off, full)
