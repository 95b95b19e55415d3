"""Restatement of Pyramid Attention Broadcast on the CogVideoX DiT (CogVideoXTransformer3DModel.enable_cache with a
PyramidAttentionBroadcastConfig) for the tests: the forward recomposed from oracle.cog_dit's functions as
tests/cog_window_attn_ref.py recomposes it, run in the dtype of the state dict it is given, with the output of every block's joint
attn1 -- the (video, text) pair its out-projection returns, before the gate multiply and the residual add -- carried over between
forwards under diffusers' rule (frameino_amd/step_cache.py: `pab_decide`).  `masks` restates window attention on the branch that is
computed.  oracle/ itself is not changed."""
import torch
import torch.nn.functional as F

from frameino_amd.step_cache import pab_decide
from oracle import cog_dit as C
from oracle.wan_dit import linear, timestep_sinusoid
from tests.cog_window_attn_ref import masked_attention


class CogPyramidAttentionBroadcastRef:
    """ref(context, hidden_states, encoder_hidden_states, timestep, image_rotary_emb) -> the model's output; `.log` holds the
    model's `cache_log` rows.  One decision per forward for the whole batch, one state per context."""

    def __init__(self, sd, cfg, current_timestep, spatial=2, timestep_range=(100, 800), masks=None):
        self.sd, self.cfg, self.now, self.n, self.range, self.masks = sd, cfg, current_timestep, spatial, timestep_range, masks or {}
        self.states, self.log = {}, []

    def _block(self, p, li, h, e, temb, rotary, cache, compute):
        sd, cfg = self.sd, self.cfg
        lt, eps = e.size(1), cfg["norm_eps"]
        hn, en, g, eg = C.layer_norm_zero(sd, p + ".norm1", eps, h, e, temb)
        if compute:
            cache[li] = masked_attention(sd, p + ".attn1", cfg["num_attention_heads"], 1e-6, hn, en, rotary, self.masks.get(li))
        ah, ae = cache[li]
        h = h + g * ah
        e = e + eg * ae
        hn, en, g, eg = C.layer_norm_zero(sd, p + ".norm2", eps, h, e, temb)
        x = torch.cat([en, hn], dim=1)
        ff = linear(sd, p + ".ff.net.2", F.gelu(linear(sd, p + ".ff.net.0.proj", x), approximate="tanh"))
        return h + g * ff[:, lt:], e + eg * ff[:, :lt]

    def __call__(self, context, hidden_states, encoder_hidden_states, timestep, image_rotary_emb):
        sd, cfg = self.sd, self.cfg
        t = float(self.now())
        st = self.states.setdefault(context, {"iteration": 0, "cache": {}})
        compute = pab_decide(st["iteration"], t, bool(st["cache"]), self.n, self.range)
        self.log.append((context, st["iteration"], t, compute, True))
        st["iteration"] += 1
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
            h, e = self._block(f"transformer_blocks.{i}", i, h, e, emb, image_rotary_emb, st["cache"], compute)
        x = torch.cat([e, h], dim=1)
        x = F.layer_norm(x, (inner,), sd.get("norm_final.weight"), sd.get("norm_final.bias"), cfg["norm_eps"])[:, lt:]
        shift, scale = linear(sd, "norm_out.linear", F.silu(emb)).chunk(2, dim=1)
        x = F.layer_norm(x, (inner,), sd.get("norm_out.norm.weight"), sd.get("norm_out.norm.bias"), cfg["norm_eps"])
        x = x * (1 + scale[:, None, :]) + shift[:, None, :]
        x = linear(sd, "proj_out", x)
        return x.reshape(b, nf, hh // ps, ww // ps, -1, ps, ps).permute(0, 1, 4, 2, 5, 3, 6).flatten(5, 6).flatten(3, 4)
