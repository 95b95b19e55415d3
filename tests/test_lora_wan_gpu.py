"""LoRA on the Wan DiT: the mid-size model of test_wan_model_gpu.py::test_midsize_model_vs_oracle with a seeded adapter on one
target family at a time, against oracle.wan_dit.wan_forward on the fp32 state dict with the adapter applied unfused
(W + s * B @ A in fp32); plus the exact-equality properties of the merge (layouts, scale 0, scale vs alpha, unload, MXFP8,
fp16)."""
import pytest
import torch

from oracle import wan_dit as W
from tests.parity import bf16_state_dict, hip_wan_model, rel_rms

pytestmark = pytest.mark.gpu

DEV = "cuda"
CFG = dict(W.WAN22_5B_CFG, num_attention_heads=4, attention_head_dim=128, in_channels=16, out_channels=8, text_dim=256,
           ffn_dim=1024, num_layers=3)
RANK = 8
# family -> (diffusers modules per block or top-level, original Wan-repo names)
FAMILIES = {
    "attn1_qkv": (["attn1.to_q", "attn1.to_k", "attn1.to_v"], ["self_attn.q", "self_attn.k", "self_attn.v"]),
    "attn1_out": (["attn1.to_out.0"], ["self_attn.o"]),
    "attn2_q": (["attn2.to_q"], ["cross_attn.q"]),
    "attn2_kv": (["attn2.to_k", "attn2.to_v"], ["cross_attn.k", "cross_attn.v"]),
    "attn2_out": (["attn2.to_out.0"], ["cross_attn.o"]),
    "ffn_up": (["ffn.net.0.proj"], ["ffn.0"]),
    "ffn_down": (["ffn.net.2"], ["ffn.2"]),
    "condition_embedder": (["@condition_embedder.time_embedder.linear_1", "@condition_embedder.time_proj",
                            "@condition_embedder.text_embedder.linear_2"],
                           ["@time_embedding.0", "@time_projection.1", "@text_embedding.2"]),
    "proj_out": (["@proj_out"], ["@head.head"]),
}
# relative size of the adapter's delta per family (so that each one moves the oracle output by >= 10x the bound)
GAIN = {"attn1_qkv": 2.0, "attn1_out": 2.0, "attn2_q": 3.0}


def _modules(fam):
    mods, orig = FAMILIES[fam]
    out = []
    for m, o in zip(mods, orig):
        if m.startswith("@"):
            out.append((m[1:], o[1:]))
        else:
            out += [(f"blocks.{i}.{m}", f"blocks.{i}.{o}") for i in range(CFG["num_layers"])]
    return out


def make_adapter(sd, fam, seed=11):
    """{(diffusers module, original module): (A, B)} fp32, delta std ~ GAIN x the weight's std"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for mod, orig in _modules(fam):
        w = sd[mod + ".weight"]
        a = torch.randn(RANK, w.shape[1], generator=g) / RANK ** 0.5
        b = torch.randn(w.shape[0], RANK, generator=g) * w.std().item() * GAIN.get(fam, 1.5)
        out[(mod, orig)] = (a, b)
    return out


def diffusers_keys(ad, alpha=None):
    sd = {}
    for (mod, _), (a, b) in ad.items():
        sd[f"transformer.{mod}.lora_A.weight"], sd[f"transformer.{mod}.lora_B.weight"] = a, b
        if alpha is not None:
            sd[f"transformer.{mod}.alpha"] = torch.tensor(float(alpha))
    return sd


def wan_keys(ad, alpha=None):
    sd = {}
    for (_, orig), (a, b) in ad.items():
        sd[f"diffusion_model.{orig}.lora_down.weight"], sd[f"diffusion_model.{orig}.lora_up.weight"] = a, b
        if alpha is not None:
            sd[f"diffusion_model.{orig}.alpha"] = torch.tensor(float(alpha))
    return sd


def merged_sd(sd, ad, s=1.0):
    out = dict(sd)
    for (mod, _), (a, b) in ad.items():
        out[mod + ".weight"] = sd[mod + ".weight"] + s * (b @ a)
    return out


@pytest.fixture(scope="module")
def setup():
    sd = W.wan_random_state_dict(CFG, seed=7, dtype=torch.float32, std=0.04)
    g = torch.Generator().manual_seed(8)
    x = torch.randn(1, 16, 5, 16, 20, generator=g)
    txt = torch.randn(1, 77, 256, generator=g)
    ts = torch.tensor([811.0])
    return sd, x, ts, txt, W.wan_forward(sd, CFG, x, ts, txt)


def run(m, x, ts, txt, dtype=torch.bfloat16, **kw):
    return m(x.to(DEV).to(dtype), ts.to(DEV), txt.to(DEV).to(dtype), return_dict=False, **kw)[0]


@pytest.mark.parametrize("fam", list(FAMILIES))
def test_family_vs_unfused_oracle(setup, fam):
    sd, x, ts, txt, base32 = setup
    ad = make_adapter(sd, fam)
    sdm = merged_sd(sd, ad)
    ref32 = W.wan_forward(sdm, CFG, x, ts, txt)
    refb = W.wan_forward(bf16_state_dict(sdm), CFG, x.bfloat16(), ts, txt.bfloat16()).float()
    moved = rel_rms(ref32, base32)
    m = hip_wan_model(CFG, sd, DEV)
    m.load_lora_adapter(diffusers_keys(ad))
    out = run(m, x, ts, txt)
    r32, rb = rel_rms(out, ref32), rel_rms(out, refb)
    print(f"{fam}: moved {moved:.3f}  hip-vs-fp32 {r32:.4f}  hip-vs-bf16-merged {rb:.4f}")
    assert moved >= 10 * 1.5e-2, f"{fam}: the adapter moves the oracle by only {moved:.4f}"
    assert r32 < 3e-2 and rb < 1.5e-2


def test_layouts_scale_alpha_and_unload_are_exact(setup):
    sd, x, ts, txt, _ = setup
    ad = {}
    for i, fam in enumerate(FAMILIES):
        ad.update(make_adapter(sd, fam, seed=100 + i))
    m = hip_wan_model(CFG, sd, DEV)
    params0 = {k: v.clone() for k, v in m.named_parameters()}
    out0 = run(m, x, ts, txt)
    m.load_lora_adapter(diffusers_keys(ad, alpha=RANK))
    out_d = run(m, x, ts, txt)
    assert not torch.equal(out_d, out0)
    # scale 0 -> the no-adapter output (the merge restores the base bits)
    assert torch.equal(run(m, x, ts, txt, attention_kwargs={"scale": 0.0}), out0)
    out_half = run(m, x, ts, txt, attention_kwargs={"scale": 0.5})
    assert torch.equal(run(m, x, ts, txt), out_d)                       # back to scale 1: no accumulated rounding
    m.unload_lora()
    assert all(torch.equal(p, params0[k]) for k, p in m.named_parameters())
    assert not any(n.rsplit(".", 1)[-1].startswith("_lora_base_") for n, _ in m.named_buffers())
    assert torch.equal(run(m, x, ts, txt), out0)
    # the original Wan-repo layout gives the same output; alpha halved == scale 0.5
    m.load_lora_adapter(wan_keys(ad, alpha=RANK))
    assert torch.equal(run(m, x, ts, txt), out_d)
    m.unload_lora()
    m.load_lora_adapter(wan_keys(ad, alpha=RANK / 2), adapter_name="half")
    assert torch.equal(run(m, x, ts, txt), out_half)
    # state_dict() returns the merged weights, the base copies stay out of it
    sdm = m.state_dict()
    assert sorted(sdm) == sorted(params0)
    assert not torch.equal(sdm["blocks.0.attn1.to_q.weight"], params0["blocks.0.attn1.to_q.weight"])


def test_mxfp8_after_loading_equals_mxfp8_on_merged_parameters(setup):
    sd, x, ts, txt, _ = setup
    ad = {}
    for fam in ("attn1_qkv", "attn2_out", "ffn_up", "ffn_down"):
        ad.update(make_adapter(sd, fam))
    m = hip_wan_model(CFG, sd, DEV)
    m.enable_mxfp8_linears()
    m.load_lora_adapter(diffusers_keys(ad))
    out = run(m, x, ts, txt)
    m2 = hip_wan_model(CFG, sd, DEV)
    m2.load_state_dict(m.state_dict())
    m2.enable_mxfp8_linears()
    assert torch.equal(run(m2, x, ts, txt), out)


def test_fp16(setup):
    sd, x, ts, txt, _ = setup
    ad = make_adapter(sd, "attn1_qkv")
    ad.update(make_adapter(sd, "ffn_down"))
    sdm = merged_sd(sd, ad)
    ref32 = W.wan_forward(sdm, CFG, x, ts, txt)
    m = hip_wan_model(CFG, sd, DEV, dtype=torch.float16)
    out0 = run(m, x, ts, txt, dtype=torch.float16)
    m.load_lora_adapter(diffusers_keys(ad))
    out = run(m, x, ts, txt, dtype=torch.float16)
    assert rel_rms(out, ref32) < 3e-2
    m.unload_lora()
    assert torch.equal(run(m, x, ts, txt, dtype=torch.float16), out0)
