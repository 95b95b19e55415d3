"""Restatement of Pyramid Attention Broadcast (diffusers' hooks/pyramid_attention_broadcast.py, frameino_amd/step_cache.py) for
the tests: the Wan DiT forward recomposed from oracle.wan_dit pieces (fp32_layer_norm, wan_attention, feed_forward, the block's
modulation as wan_block writes it; embedding and head from tests/step_cache_ref.py), run in the dtype of the state dict it is
given, with the rule in plain torch -- every attention module its own `iteration` and `cache` per context, as diffusers keeps
them.  oracle/ itself is not changed."""
from oracle import wan_dit as W
from tests.step_cache_ref import _embed, _head, loop_forward      # noqa: F401  (loop_forward: re-exported for the pipeline test)


class PyramidAttentionBroadcastRef:
    """`ref(context, hidden_states, timestep, text)`: one forward under `context`; `timestep_of()` is the config's
    current_timestep_callback.  `spatial` / `cross`: the block skip ranges (None: the kind is not hooked); `*_range`: the
    timestep skip ranges.  `log` holds (context, iteration, timestep, self computed, cross computed) like
    WanTransformer3DModel.cache_log.  `processors`: {"blocks.i.attn1" / "blocks.i.attn2": callable(module output) -> output}
    stands for a custom attention processor (what the module returns is what is cached)."""

    def __init__(self, sd, cfg, timestep_of, spatial=None, cross=None, spatial_range=(100, 800), cross_range=(100, 800),
                 processors=None):
        self.sd, self.cfg, self.timestep_of = sd, cfg, timestep_of
        self.rule = {"attn1": (spatial, spatial_range), "attn2": (cross, cross_range)}
        self.processors = processors or {}
        self.state, self.log = {}, []

    def reset(self):
        self.state = {}

    def _attention(self, ctx, name, decisions, *args):
        """one attention module's forward under its hook: diffusers' rule, state per (context, module)"""
        kind = name.rsplit(".", 1)[1]
        skip, (lo, hi) = self.rule[kind]
        run = lambda: self.processors.get(name, lambda y: y)(W.wan_attention(self.sd, name, *args))       # noqa: E731
        if skip is None:
            return run()                                   # never hooked
        st = self.state.setdefault((ctx, name), {"iteration": 0, "cache": None})
        t = float(self.timestep_of())
        in_range = lo < t < hi
        compute = st["cache"] is None or st["iteration"] == 0 or not in_range or st["iteration"] % skip == 0
        out = run() if compute else st["cache"]
        st["cache"] = out
        st["iteration"] += 1
        decisions.setdefault(kind, set()).add(compute)
        return out

    def _block(self, ctx, prefix, x, txt, temb, rot, decisions):
        """oracle.wan_dit.wan_block with the two attention calls routed through the hook"""
        sd, cfg = self.sd, self.cfg
        heads, eps = cfg["num_attention_heads"], cfg["eps"]
        table = sd[prefix + ".scale_shift_table"]
        if temb.ndim == 4:
            mods = (table.unsqueeze(0) + temb.float()).chunk(6, dim=2)
            shift_msa, scale_msa, gate_msa, c_shift, c_scale, c_gate = [m.squeeze(2) for m in mods]
        else:
            shift_msa, scale_msa, gate_msa, c_shift, c_scale, c_gate = (table + temb.float()).chunk(6, dim=1)
        n = (W.fp32_layer_norm(x.float(), None, None, eps) * (1 + scale_msa) + shift_msa).type_as(x)
        a = self._attention(ctx, prefix + ".attn1", decisions, heads, eps, n, None, rot)
        x = (x.float() + a * gate_msa).type_as(x)
        if cfg.get("cross_attn_norm", True):
            n = W.fp32_layer_norm(x.float(), sd[prefix + ".norm2.weight"], sd[prefix + ".norm2.bias"], eps).type_as(x)
        else:
            n = x.float().type_as(x)
        a = self._attention(ctx, prefix + ".attn2", decisions, heads, eps, n, txt, None)
        x = x + a
        n = (W.fp32_layer_norm(x.float(), None, None, eps) * (1 + c_scale) + c_shift).type_as(x)
        f = W.feed_forward(sd, prefix + ".ffn", n)
        return (x.float() + f.float() * c_gate).type_as(x)

    def __call__(self, context, hidden_states, timestep, txt):
        sd, cfg = self.sd, self.cfg
        x, temb, tproj, txt, rot, geo = _embed(sd, cfg, hidden_states, timestep, txt)
        steps = self.state.setdefault((context, "forwards"), {"n": 0})
        decisions = {}
        for i in range(cfg["num_layers"]):
            x = self._block(context, f"blocks.{i}", x, txt, tproj, rot, decisions)
        for flags in decisions.values():
            assert len(flags) == 1                         # all modules of a kind decide alike
        self.log.append((context, steps["n"], float(self.timestep_of()), next(iter(decisions.get("attn1", {True}))),
                         next(iter(decisions.get("attn2", {True})))))
        steps["n"] += 1
        return _head(sd, cfg, x, temb, geo)
