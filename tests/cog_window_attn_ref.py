"""Restatement of the sliding-window self-attention of the CogVideoX DiT (CogVideoXTransformer3DModel.enable_window_attention) for
the tests: the forward recomposed from oracle.cog_dit's functions, run in the dtype of the state dict it is given, with the joint
self-attention of every windowed block restated as SDPA under the boolean block mask expanded from the range table
(frameino_amd/window_attention.py, `prefix_rows` = the text rows).  oracle/ itself is not changed.  Also the tiny geometry the GPU
tests share with their CPU half."""
import torch
import torch.nn.functional as F

from frameino_amd.window_attention import block_mask, frame_window_ranges
from oracle import cog_dit as C
from oracle.wan_dit import linear, timestep_sinusoid

# the tiny DiT of tests/golden/cog_dit_tiny.npz (2 layers, 2 heads x 64, 8 text rows) on 9 latent frames (8 + the ID frame) of a
# 20 x 30 latent, patch 2: 150 tokens per frame, L = 8 + 1350 = 1358 -> 6 q-blocks, 22 key tiles with 14 keys in the last
TINY_CFG = dict(num_attention_heads=2, attention_head_dim=64, in_channels=6, out_channels=2, flip_sin_to_cos=True, freq_shift=0,
                time_embed_dim=32, text_embed_dim=16, num_layers=2, sample_width=30, sample_height=20, sample_frames=29,
                patch_size=2, temporal_compression_ratio=4, max_text_seq_length=8, norm_elementwise_affine=True, norm_eps=1e-5,
                use_rotary_positional_embeddings=True, use_learned_positional_embeddings=True, use_FrameIn=True)
FRAMES, LAT_H, LAT_W, TEXT = 9, 20, 30, 8
TPF = (LAT_H // 2) * (LAT_W // 2)
L = TEXT + FRAMES * TPF
SINKS = (0, FRAMES - 1)                     # config sink (0,) + id_frames = 1


def layer_masks(num_layers, frames, tokens_per_frame, text_rows, window_frames, sinks, skip_layers=(), live_rows=None):
    """{layer: bool [L, L] or None (dense)}: what every block's joint self-attention sees.  Under `live_rows` = (r0, r1) the last
    block's queries are rows [r0, r1) of the joint sequence and its q-blocks are counted from r0 (its other rows are not queries:
    left dense here, their output is never compared)."""
    n = text_rows + frames * tokens_per_frame
    full = block_mask(frame_window_ranges(frames, tokens_per_frame, window_frames, sinks, prefix_rows=text_rows), n, n, text_rows)
    masks = {li: (None if li in skip_layers else full) for li in range(num_layers)}
    last = num_layers - 1
    if live_rows is not None and masks[last] is not None:
        r0, r1 = live_rows
        m = torch.ones(n, n, dtype=torch.bool)
        m[r0:r1] = block_mask(frame_window_ranges(frames, tokens_per_frame, window_frames, sinks, q_rows=(r0, r1),
                                                  prefix_rows=text_rows), r1 - r0, n, text_rows)
        masks[last] = m
    return masks


def masked_attention(sd, p, heads, eps, hidden_states, encoder_hidden_states, rotary, mask):
    """oracle.cog_dit.cog_attention with `mask` (bool [L, L] over the joint [text | video] rows, None: dense) on the logits"""
    lt = encoder_hidden_states.size(1)
    hs = torch.cat([encoder_hidden_states, hidden_states], dim=1)
    b = hs.shape[0]
    q, k, v = (linear(sd, f"{p}.{n}", hs) for n in ("to_q", "to_k", "to_v"))
    dh = q.shape[-1] // heads
    q, k, v = (t.view(b, -1, heads, dh).transpose(1, 2) for t in (q, k, v))
    q = F.layer_norm(q, (dh,), sd[p + ".norm_q.weight"], sd[p + ".norm_q.bias"], eps)
    k = F.layer_norm(k, (dh,), sd[p + ".norm_k.weight"], sd[p + ".norm_k.bias"], eps)
    if rotary is not None:
        q = torch.cat([q[:, :, :lt], C.cog_rope(q[:, :, lt:], *rotary)], dim=2)
        k = torch.cat([k[:, :, :lt], C.cog_rope(k[:, :, lt:], *rotary)], dim=2)
    o = F.scaled_dot_product_attention(q, k, v, attn_mask=None if mask is None else mask.to(q.device))
    o = linear(sd, p + ".to_out.0", o.transpose(1, 2).reshape(b, -1, heads * dh))
    return o[:, lt:], o[:, :lt]


def _block(sd, p, cfg, h, e, temb, rotary, mask):
    """oracle.cog_dit.cog_block with the joint self-attention under `mask`"""
    lt = e.size(1)
    eps = cfg["norm_eps"]
    hn, en, g, eg = C.layer_norm_zero(sd, p + ".norm1", eps, h, e, temb)
    ah, ae = masked_attention(sd, p + ".attn1", cfg["num_attention_heads"], 1e-6, hn, en, rotary, mask)
    h = h + g * ah
    e = e + eg * ae
    hn, en, g, eg = C.layer_norm_zero(sd, p + ".norm2", eps, h, e, temb)
    x = torch.cat([en, hn], dim=1)
    ff = linear(sd, p + ".ff.net.2", F.gelu(linear(sd, p + ".ff.net.0.proj", x), approximate="tanh"))
    return h + g * ff[:, lt:], e + eg * ff[:, :lt]


def window_forward(sd, cfg, hidden_states, encoder_hidden_states, timestep, image_rotary_emb, masks):
    """oracle.cog_dit.cog_forward with `masks`: layer_masks(...) ({} or all None: the dense model)"""
    b, nf, c, hh, ww = hidden_states.shape
    inner = cfg["num_attention_heads"] * cfg["attention_head_dim"]
    ps = cfg["patch_size"]
    t_emb = timestep_sinusoid(timestep, inner, cfg.get("flip_sin_to_cos", True), cfg.get("freq_shift", 0)).to(hidden_states.dtype)
    emb = linear(sd, "time_embedding.linear_2", F.silu(linear(sd, "time_embedding.linear_1", t_emb)))
    txt = linear(sd, "patch_embed.text_proj", encoder_hidden_states)
    lt = txt.shape[1]
    img = F.conv2d(hidden_states.reshape(-1, c, hh, ww), sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=ps)
    img = img.view(b, nf, *img.shape[1:]).flatten(3).transpose(2, 3).flatten(1, 2)
    x = torch.cat([txt, img], dim=1).contiguous()
    x = x + C.cog_pos_embeds(sd, cfg, nf, hh, ww, lt, x.dtype)
    e, h = x[:, :lt], x[:, lt:]
    for i in range(cfg["num_layers"]):
        h, e = _block(sd, f"transformer_blocks.{i}", cfg, h, e, emb, image_rotary_emb, masks.get(i))
    x = torch.cat([e, h], dim=1)
    x = F.layer_norm(x, (inner,), sd.get("norm_final.weight"), sd.get("norm_final.bias"), cfg["norm_eps"])[:, lt:]
    shift, scale = linear(sd, "norm_out.linear", F.silu(emb)).chunk(2, dim=1)
    x = F.layer_norm(x, (inner,), sd.get("norm_out.norm.weight"), sd.get("norm_out.norm.bias"), cfg["norm_eps"])
    x = x * (1 + scale[:, None, :]) + shift[:, None, :]
    x = linear(sd, "proj_out", x)
    return x.reshape(b, nf, hh // ps, ww // ps, -1, ps, ps).permute(0, 1, 4, 2, 5, 3, 6).flatten(5, 6).flatten(3, 4)


def tiny_state_dict(seed, std, v_scale, gate_bias):
    """fp32 random weights of TINY_CFG: N(0, std) (norm weights 1 + N(0, std)), the self-attention's value projection scaled by
    `v_scale` and the attention gate's bias set to `gate_bias` so that the attention output reaches the result"""
    from frameino_amd.cogvideox_transformer_3d import CogVideoXTransformer3DModel
    m = CogVideoXTransformer3DModel(**TINY_CFG)
    g = torch.Generator().manual_seed(seed)
    sd = {}
    inner = TINY_CFG["num_attention_heads"] * TINY_CFG["attention_head_dim"]
    for name, t in list(m.named_parameters()) + list(m.named_buffers()):
        x = std * torch.randn(t.shape, generator=g)
        if name.endswith("norm.weight") or "norm_q.weight" in name or "norm_k.weight" in name or name == "norm_final.weight":
            x = 1.0 + x
        if ".attn1.to_v.weight" in name:
            x = x * v_scale
        if name.endswith(".norm1.linear.bias"):              # chunks (shift, scale, gate, e_shift, e_scale, e_gate)
            x[2 * inner:3 * inner] = gate_bias
            x[5 * inner:] = gate_bias
        sd[name] = x
    return sd


def tiny_inputs(seed=12, batch=1):
    """a latent whose frames differ by an offset (so that which frames a query sees matters), text, timestep, RoPE tables"""
    from frameino_amd.pipeline_cogvideox_i2v_motion_frameino import get_3d_rotary_pos_embed
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(batch, FRAMES, 6, LAT_H, LAT_W, generator=g) + 2.0 * torch.randn(batch, FRAMES, 6, 1, 1, generator=g)
    txt = torch.randn(batch, TEXT, 16, generator=g)
    ts = torch.full((batch,), 811.0)
    gh, gw = LAT_H // 2, LAT_W // 2
    cos, sin = get_3d_rotary_pos_embed(64, ((0, 0), (gh, gw)), (gh, gw), FRAMES - 1)
    n1 = cos.shape[0] // (FRAMES - 1)                       # the FrameIn extension: the ID frame reuses the first frame's rows
    return x, txt, ts, (torch.cat([cos, cos[:n1]]).float(), torch.cat([sin, sin[:n1]]).float())
