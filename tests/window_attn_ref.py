"""Restatement of the sliding-window self-attention (frameino_amd/window_attention.py, WanTransformer3DModel.
enable_window_attention) for the tests: the Wan DiT forward recomposed from oracle.wan_dit pieces the way tests/pab_ref.py does
(embedding and head from tests/step_cache_ref.py), run in the dtype of the state dict it is given, with the self-attention of
every windowed block restated as SDPA under the boolean block mask expanded from the range table.  oracle/ itself is not
changed."""
import torch
import torch.nn.functional as F

from frameino_amd.window_attention import block_mask, frame_window_ranges
from oracle import wan_dit as W
from tests.step_cache_ref import _embed, _head


def layer_masks(num_layers, frames, tokens_per_frame, window_frames, sinks, skip_layers=(), live_rows=None):
    """{layer: bool [L, L] or None (dense)}: what every block's self-attention sees.  Under `live_rows` = (s0, s1) the last
    block's queries are rows [s0, s1) and its q-blocks are counted from s0 (its other rows are not queries: left dense here,
    their output is never compared)."""
    L = frames * tokens_per_frame
    full = block_mask(frame_window_ranges(frames, tokens_per_frame, window_frames, sinks), L, L)
    masks = {li: (None if li in skip_layers else full) for li in range(num_layers)}
    last = num_layers - 1
    if live_rows is not None and masks[last] is not None:
        s0, s1 = live_rows
        m = torch.ones(L, L, dtype=torch.bool)
        m[s0:s1] = block_mask(frame_window_ranges(frames, tokens_per_frame, window_frames, sinks, q_rows=(s0, s1)), s1 - s0, L)
        masks[last] = m
    return masks


def masked_self_attention(sd, prefix, heads, eps, x, rot, mask):
    """oracle.wan_dit.wan_attention for the self-attention, with `mask` (bool [L, L], None: dense) on the logits"""
    q = W.rms_norm(W.linear(sd, prefix + ".to_q", x), sd[prefix + ".norm_q.weight"], eps)
    k = W.rms_norm(W.linear(sd, prefix + ".to_k", x), sd[prefix + ".norm_k.weight"], eps)
    v = W.linear(sd, prefix + ".to_v", x)
    q, k, v = (t.unflatten(2, (heads, -1)).transpose(1, 2) for t in (q, k, v))
    q, k = W.apply_wan_rope(q, *rot), W.apply_wan_rope(k, *rot)
    o = F.scaled_dot_product_attention(q, k, v, attn_mask=None if mask is None else mask.to(q.device))
    return W.linear(sd, prefix + ".to_out.0", o.transpose(1, 2).flatten(2, 3).type_as(q))


def _block(sd, cfg, prefix, x, txt, temb, rot, mask):
    """oracle.wan_dit.wan_block with the self-attention under `mask`"""
    heads, eps = cfg["num_attention_heads"], cfg["eps"]
    table = sd[prefix + ".scale_shift_table"]
    if temb.ndim == 4:
        mods = (table.unsqueeze(0) + temb.float()).chunk(6, dim=2)
        shift_msa, scale_msa, gate_msa, c_shift, c_scale, c_gate = [m.squeeze(2) for m in mods]
    else:
        shift_msa, scale_msa, gate_msa, c_shift, c_scale, c_gate = (table + temb.float()).chunk(6, dim=1)
    n = (W.fp32_layer_norm(x.float(), None, None, eps) * (1 + scale_msa) + shift_msa).type_as(x)
    a = masked_self_attention(sd, prefix + ".attn1", heads, eps, n, rot, mask)
    x = (x.float() + a * gate_msa).type_as(x)
    if cfg.get("cross_attn_norm", True):
        n = W.fp32_layer_norm(x.float(), sd[prefix + ".norm2.weight"], sd[prefix + ".norm2.bias"], eps).type_as(x)
    else:
        n = x.float().type_as(x)
    x = x + W.wan_attention(sd, prefix + ".attn2", heads, eps, n, txt, None)
    n = (W.fp32_layer_norm(x.float(), None, None, eps) * (1 + c_scale) + c_shift).type_as(x)
    f = W.feed_forward(sd, prefix + ".ffn", n)
    return (x.float() + f.float() * c_gate).type_as(x)


def window_forward(sd, cfg, hidden_states, timestep, txt, masks):
    """one forward; `masks`: layer_masks(...) ({} or all None: the dense model)"""
    x, temb, tproj, txt, rot, geo = _embed(sd, cfg, hidden_states, timestep, txt)
    for i in range(cfg["num_layers"]):
        x = _block(sd, cfg, f"blocks.{i}", x, txt, tproj, rot, masks.get(i))
    return _head(sd, cfg, x, temb, geo)
