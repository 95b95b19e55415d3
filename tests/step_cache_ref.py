"""Restatement of first-block caching (diffusers' FirstBlockCache, frameino_amd/step_cache.py) for the tests: a Wan DiT forward
composed from oracle.wan_dit pieces (condition embedder, RoPE, blocks, the head as wan_forward writes it), run in the dtype of
the state dict it is given, with the caching rule in plain torch.  oracle/ itself is not changed."""
import torch
import torch.nn.functional as F

from oracle import wan_dit as W


def _embed(sd, cfg, hidden_states, timestep, txt):
    """wan_forward up to the block loop: (h0 [B, L, D], temb, timestep_proj, text, rotary, geometry)"""
    b, _, nf, hh, ww = hidden_states.shape
    pt, ph, pw = cfg["patch_size"]
    geo = (b, nf // pt, hh // ph, ww // pw)
    rotary = W.wan_rope(cfg["attention_head_dim"], cfg["rope_max_seq_len"], *geo[1:], hidden_states.device)
    x = F.conv3d(hidden_states, sd["patch_embedding.weight"], sd["patch_embedding.bias"], stride=(pt, ph, pw))
    x = x.flatten(2).transpose(1, 2)
    ts_len = timestep.shape[1] if timestep.ndim == 2 else None
    temb, tproj, txt = W.wan_condition_embedder(sd, cfg, timestep.flatten() if ts_len else timestep, txt, ts_len)
    tproj = tproj.unflatten(2, (6, -1)) if ts_len is not None else tproj.unflatten(1, (6, -1))
    return x, temb, tproj, txt, rotary, geo


def _head(sd, cfg, x, temb, geo):
    """the output head of wan_forward (norm_out, proj_out, unpatchify)"""
    b, ppf, pph, ppw = geo
    pt, ph, pw = cfg["patch_size"]
    table = sd["scale_shift_table"]
    if temb.ndim == 3:
        shift, scale = (table.unsqueeze(0) + temb.unsqueeze(2)).chunk(2, dim=2)
        shift, scale = shift.squeeze(2), scale.squeeze(2)
    else:
        shift, scale = (table + temb.unsqueeze(1)).chunk(2, dim=1)
    x = (W.fp32_layer_norm(x.float(), None, None, cfg["eps"]) * (1 + scale) + shift).type_as(x)
    x = W.linear(sd, "proj_out", x)
    x = x.reshape(b, ppf, pph, ppw, pt, ph, pw, -1).permute(0, 7, 1, 4, 2, 5, 3, 6)
    return x.flatten(6, 7).flatten(4, 5).flatten(2, 3)


def relative_l1(r, p):
    """diffusers' decision quantity: (r - p).abs().mean() / p.abs().mean(), each tensor op in the dtype of r"""
    return float((r - p).abs().mean() / p.abs().mean())


class FirstBlockCacheRef:
    """`ref(context, hidden_states, timestep, text)`: one forward with first-block caching under `context`.  `log` holds
    (context, step, diff, computed) like WanTransformer3DModel.cache_log; `last` the (h0, h1) of the last call."""

    def __init__(self, sd, cfg, threshold):
        self.sd, self.cfg, self.threshold = sd, cfg, threshold
        self.state, self.log = {}, []

    def reset(self):
        self.state = {}

    def head_residual(self, hidden_states, timestep, txt):
        """r = T(h1 - h0) of one forward, without touching the state"""
        h0, _, tproj, txt, rot, _ = _embed(self.sd, self.cfg, hidden_states, timestep, txt)
        return W.wan_block(self.sd, "blocks.0", self.cfg, h0, txt, tproj, rot) - h0

    def __call__(self, context, hidden_states, timestep, txt):
        sd, cfg = self.sd, self.cfg
        h0, temb, tproj, txt, rot, geo = _embed(sd, cfg, hidden_states, timestep, txt)
        h1 = W.wan_block(sd, "blocks.0", cfg, h0, txt, tproj, rot)
        r = h1 - h0
        st = self.state.setdefault(context, {"head": None, "tail": None, "steps": 0})
        if st["head"] is None:
            diff, compute = None, True
        else:
            diff = relative_l1(r, st["head"])
            compute = diff > self.threshold
        self.log.append((context, st["steps"], diff, compute))
        st["steps"] += 1
        if compute:
            st["head"] = r
            x = h1
            for i in range(1, cfg["num_layers"]):
                x = W.wan_block(sd, f"blocks.{i}", cfg, x, txt, tproj, rot)
            st["tail"] = x - h1
        else:
            x = st["tail"] + h1
        return _head(sd, cfg, x, temb, geo)


def loop_forward(ref, pe, ne):
    """a `forward(x, timestep, text)` for oracle.wan_pipeline.wan_denoise_loop: the context is picked by which text tensor is
    passed (the prompt -> "cond", the negative prompt -> "uncond"), as the reference loop's two cache_context calls do"""
    def forward(x, t, e):
        ctx = "cond" if torch.equal(e, pe.to(e.dtype)) else "uncond" if ne is not None and torch.equal(e, ne.to(e.dtype)) else None
        assert ctx is not None, "text tensor is neither the prompt nor the negative prompt"
        return ref(ctx, x, t, e)
    return forward
