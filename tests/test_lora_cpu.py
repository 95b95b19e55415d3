"""LoRA loading on the host (no GPU): key layouts, scales, loud failures, adapter bookkeeping, and the C-ABI entry of the
merge kernel (frameino_amd/lora.py, fino_lora_merge)."""
import json
import math
import os

import pytest
import torch

from oracle import wan_dit as W
from tests.parity import model_cfg

CFG = dict(W.WAN22_5B_CFG, num_attention_heads=2, attention_head_dim=128, in_channels=8, out_channels=4, text_dim=64,
           ffn_dim=512, num_layers=2)
D = 256

# original Wan-repo names -> the diffusers names they must land on
PAIRS = [("blocks.0.self_attn.q", "blocks.0.attn1.to_q"), ("blocks.1.self_attn.o", "blocks.1.attn1.to_out.0"),
         ("blocks.0.cross_attn.k", "blocks.0.attn2.to_k"), ("blocks.1.cross_attn.v", "blocks.1.attn2.to_v"),
         ("blocks.0.ffn.0", "blocks.0.ffn.net.0.proj"), ("blocks.1.ffn.2", "blocks.1.ffn.net.2"),
         ("head.head", "proj_out"), ("text_embedding.0", "condition_embedder.text_embedder.linear_1"),
         ("text_embedding.2", "condition_embedder.text_embedder.linear_2"),
         ("time_embedding.0", "condition_embedder.time_embedder.linear_1"),
         ("time_embedding.2", "condition_embedder.time_embedder.linear_2"),
         ("time_projection.1", "condition_embedder.time_proj")]


@pytest.fixture(scope="module")
def model():
    from frameino_amd.transformer_wan import WanTransformer3DModel
    return WanTransformer3DModel(**model_cfg(CFG))


def _factors(model, rank=4, seed=0):
    """{diffusers module: (A, B)} for every target of PAIRS, seeded"""
    g = torch.Generator().manual_seed(seed)
    params = dict(model.named_parameters())
    out = {}
    for _, mod in PAIRS:
        n, k = params[mod + ".weight"].shape
        out[mod] = (torch.randn(rank, k, generator=g), torch.randn(n, rank, generator=g))
    return out


def diffusers_sd(f, alpha=None):
    sd = {}
    for mod, (a, b) in f.items():
        sd[f"transformer.{mod}.lora_A.weight"], sd[f"transformer.{mod}.lora_B.weight"] = a, b
        if alpha is not None:
            sd[f"transformer.{mod}.alpha"] = torch.tensor(float(alpha))
    return sd


def wan_sd(f, alpha=None, names=("lora_down", "lora_up")):
    back = {d: o for o, d in PAIRS}
    sd = {}
    for mod, (a, b) in f.items():
        sd[f"diffusion_model.{back[mod]}.{names[0]}.weight"], sd[f"diffusion_model.{back[mod]}.{names[1]}.weight"] = a, b
        if alpha is not None:
            sd[f"diffusion_model.{back[mod]}.alpha"] = torch.tensor(float(alpha))
    return sd


def parse(model, sd, config=None):
    from frameino_amd.lora import parse_adapter
    return parse_adapter(sd, dict(model.named_parameters()), config=config, wan_layout=True)


def canon(factors):
    return sorted((t, a.tolist(), b.tolist(), s) for t, a, b, s in factors)


def test_both_wan_layouts_parse_to_the_same_targets(model):
    f = _factors(model)
    ref, _ = parse(model, diffusers_sd(f, alpha=2.0))
    assert sorted(t for t, *_ in ref) == sorted(m + ".weight" for _, m in PAIRS)
    assert all(s == 0.5 for *_, s in ref)
    for names in (("lora_down", "lora_up"), ("lora_A", "lora_B")):
        got, _ = parse(model, wan_sd(f, alpha=2.0, names=names))
        assert canon(got) == canon(ref)
    # the diffusers layout without the "transformer." prefix, and with PEFT's "base_model.model." one
    bare = {k[len("transformer."):]: v for k, v in diffusers_sd(f).items()}
    assert canon(parse(model, bare)[0]) == canon(parse(model, diffusers_sd(f))[0])
    peft = {"base_model.model." + k: v for k, v in bare.items()}
    assert canon(parse(model, peft)[0]) == canon(parse(model, bare)[0])


def test_scale_alpha_rslora_and_adapter_config(model, tmp_path):
    from safetensors.torch import save_file
    from frameino_amd.lora import read_adapter
    f = {"blocks.0.attn1.to_q": _factors(model, rank=8)["blocks.0.attn1.to_q"]}
    assert parse(model, diffusers_sd(f))[0][0][3] == 1.0                          # no alpha: scale 1, as diffusers
    assert parse(model, diffusers_sd(f, alpha=4))[0][0][3] == 0.5
    bare = {k[len("transformer."):]: v for k, v in diffusers_sd(f).items()}
    assert parse(model, bare, config={"r": 8, "lora_alpha": 16})[0][0][3] == 2.0
    assert math.isclose(parse(model, bare, config={"r": 8, "lora_alpha": 16, "use_rslora": True})[0][0][3], 16 / math.sqrt(8))
    # the PEFT folder form: adapter_model.safetensors + adapter_config.json
    folder = tmp_path / "peft"
    folder.mkdir()
    save_file({"base_model.model." + k: v.contiguous() for k, v in bare.items()}, str(folder / "adapter_model.safetensors"))
    (folder / "adapter_config.json").write_text(json.dumps({"r": 8, "lora_alpha": 4, "use_rslora": False}))
    sd, cfg = read_adapter(str(folder))
    assert cfg["lora_alpha"] == 4 and parse(model, sd, cfg)[0][0][3] == 0.5
    # weight_name= picks another file of the folder; the default names are tried otherwise
    save_file({k: v.contiguous() for k, v in diffusers_sd(f).items()}, str(folder / "my_lora.safetensors"))
    sd2, _ = read_adapter(str(folder), weight_name="my_lora.safetensors")
    assert sorted(sd2) == sorted(diffusers_sd(f))
    with pytest.raises(OSError):
        read_adapter(str(tmp_path))


def test_diff_and_diff_b_map_onto_parameters(model):
    g = torch.Generator().manual_seed(3)
    sd = {"diffusion_model.blocks.0.self_attn.q.diff_b": torch.randn(D, generator=g),
          "diffusion_model.blocks.1.self_attn.norm_k.diff": torch.randn(D, generator=g),
          "diffusion_model.blocks.0.cross_attn.norm_q.diff": torch.randn(D, generator=g),
          "diffusion_model.blocks.0.norm3.diff": torch.randn(D, generator=g),
          "diffusion_model.blocks.0.norm3.diff_b": torch.randn(D, generator=g),
          "diffusion_model.head.head.diff_b": torch.randn(CFG["out_channels"] * 4, generator=g)}
    factors, diffs = parse(model, sd)
    assert not factors
    got = {t: d for t, d in diffs}
    assert sorted(got) == sorted(["blocks.0.attn1.to_q.bias", "blocks.1.attn1.norm_k.weight", "blocks.0.attn2.norm_q.weight",
                                  "blocks.0.norm2.weight", "blocks.0.norm2.bias", "proj_out.bias"])
    assert torch.equal(got["blocks.1.attn1.norm_k.weight"], sd["diffusion_model.blocks.1.self_attn.norm_k.diff"])


@pytest.mark.parametrize("case", ["unknown", "target", "shape", "conv", "rank_pattern", "alpha_pattern", "dora", "half"])
def test_loud_failures_name_the_key(model, case):
    from frameino_amd.lora import LoraError
    f = {"blocks.0.attn1.to_q": _factors(model)["blocks.0.attn1.to_q"]}
    sd, config, key = diffusers_sd(f), None, None
    if case == "unknown":
        key = "transformer.blocks.0.attn1.to_q.lora_X.weight"
        sd[key] = torch.zeros(1)
    elif case == "target":
        key = "transformer.blocks.7.attn1.to_q.lora_A.weight"
        sd[key], sd["transformer.blocks.7.attn1.to_q.lora_B.weight"] = f["blocks.0.attn1.to_q"]
    elif case == "shape":
        key = "transformer.blocks.0.attn1.to_q.lora_A.weight"
        sd[key] = torch.zeros(4, D + 1)
    elif case == "conv":
        key = "diffusion_model.patch_embedding.lora_down.weight"
        sd[key], sd["diffusion_model.patch_embedding.lora_up.weight"] = torch.zeros(4, 8, 1, 2, 2), torch.zeros(D, 4, 1, 1, 1)
    elif case in ("rank_pattern", "alpha_pattern"):
        key = "blocks.0.attn1.to_q"
        config = {"r": 4, "lora_alpha": 4, case: {key: 8}}
    elif case == "dora":
        key = "transformer.blocks.0.attn1.to_q.lora_magnitude_vector"
        sd[key] = torch.ones(D)
    elif case == "half":
        key = "transformer.blocks.0.attn1.to_q.lora_A.weight"
        del sd["transformer.blocks.0.attn1.to_q.lora_B.weight"]
    with pytest.raises(LoraError, match=key.replace(".", r"\.")):
        parse(model, sd, config)


def test_adapter_bookkeeping_on_a_host_model():
    """A model built on the CPU loads adapters without touching a device; the PeftAdapterMixin names keep their books."""
    from frameino_amd.transformer_wan import WanTransformer3DModel
    m = WanTransformer3DModel(**model_cfg(CFG))
    before = {k: v.clone() for k, v in m.state_dict().items()}
    f = _factors(m)
    assert m.load_lora_adapter(diffusers_sd(f)) == "default_0"
    assert m.load_lora_adapter(wan_sd(f), adapter_name="style") == "style"
    with pytest.raises(ValueError, match="already in use"):
        m.load_lora_adapter(wan_sd(f), adapter_name="style")
    assert m.active_adapters() == ["default_0", "style"] and m.get_list_adapters() == ["default_0", "style"]
    m.set_adapters(["style"], weights=0.5)
    assert m.active_adapters() == ["style"]
    with pytest.raises(ValueError, match="unknown"):
        m.set_adapters(["nope"])
    with pytest.raises(ValueError, match="weights"):
        m.set_adapters(["style", "default_0"], weights=[1.0])
    m.set_adapters(["style", "default_0"], weights=[1.0, None])
    m.delete_adapters("style")
    assert m.active_adapters() == ["default_0"] and m.get_list_adapters() == ["default_0"]
    m.disable_lora()
    m.enable_lora()
    # nothing merged on the host: parameters, state_dict and buffers as before, no device touched
    after = m.state_dict()
    assert sorted(after) == sorted(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert all(not p.is_cuda for p in m.parameters())
    m.unload_lora()
    assert m.get_list_adapters() == [] and m.active_adapters() == []


def test_pipelines_carry_the_loader_names():
    from frameino_amd.pipeline_cogvideox_i2v_motion import CogVideoXImageToVideoPipeline as CogS1
    from frameino_amd.pipeline_cogvideox_i2v_motion_frameino import CogVideoXImageToVideoPipeline as Cog
    from frameino_amd.pipeline_wan_i2v_motion import WanImageToVideoPipeline as WanS1
    from frameino_amd.pipeline_wan_i2v_motion_frameino import WanImageToVideoPipeline as Wan
    from frameino_amd.cogvideox_transformer_3d import CogVideoXTransformer3DModel
    names = ("load_lora_weights", "lora_state_dict", "set_adapters", "get_active_adapters", "get_list_adapters",
             "delete_adapters", "disable_lora", "enable_lora", "unload_lora_weights", "fuse_lora", "unfuse_lora")
    for cls in (Wan, WanS1, Cog, CogS1):
        assert all(callable(getattr(cls, n)) for n in names), cls
    for n in ("load_lora_adapter", "set_adapters", "active_adapters", "disable_lora", "enable_lora", "delete_adapters",
              "unload_lora"):
        assert callable(getattr(CogVideoXTransformer3DModel, n))


def test_merge_symbol_is_declared_exported_and_bound():
    import ctypes
    from frameino_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    assert "fino_lora_merge" in _lib.declared_symbols() and "fino_lora_merge" in _lib.SIGNATURES
    assert hasattr(lib, "fino_lora_merge")
    # argument validation happens before any launch (no GPU needed)
    rank, scale = (ctypes.c_int * 1)(0), (ctypes.c_float * 1)(1.0)
    ptr, ld = (ctypes.c_void_p * 1)(16), (ctypes.c_int64 * 1)(64)
    rc = lib.fino_lora_merge(16, 64, 16, 64, 64, 64, 1, ptr, ld, ptr, ld, rank, scale, 0, 0)
    assert rc == -1 and b"rank" in lib.fino_last_error()
    rc = lib.fino_lora_merge(16, 64, 16, 64, 64, 64, 0, None, None, None, None, None, None, 7, 0)
    assert rc == -1 and b"dtype" in lib.fino_last_error()
    rc = lib.fino_lora_merge(16, 32, 16, 64, 64, 64, 0, None, None, None, None, None, None, 0, 0)
    assert rc == -1 and b"leading dimension" in lib.fino_last_error()
    rc = lib.fino_lora_merge(16, 64, 16, 64, 64, 64, 9, ptr, ld, ptr, ld, rank, scale, 0, 0)
    assert rc == -1 and b"n_adapters" in lib.fino_last_error()
