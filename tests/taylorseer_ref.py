"""Restatement of TaylorSeer caching (frameino_amd/step_cache.py, include/frameino_hip.h) for the tests.

`update_ref` / `predict_ref`: the factor arithmetic with plain torch fp32 operations on the CPU and `.to(F)` roundings -- one
IEEE operation per subtraction, division, multiplication and addition (the division by a tensor, so that torch cannot turn it
into a multiplication by a reciprocal).  `predict_ref64`: the same prediction in float64, rounded once.

`TaylorSeerRef`: the Wan DiT forward recomposed from oracle.wan_dit pieces as tests/pab_ref.py does, run in the dtype of the
state dict it is given, with the factors held per (context, layer, kind) in default mode and per context in lite mode.
oracle/ itself is not changed."""
import math

import torch

from frameino_amd.step_cache import taylorseer_decide
from oracle import wan_dit as W
from tests.step_cache_ref import _embed, _head, loop_forward      # noqa: F401  (loop_forward: for a pipeline test)


def coefficients(k, n):
    """c_i = float32(k**i / i!), computed in double"""
    return [float(torch.tensor(float(k) ** i / math.factorial(i), dtype=torch.float64).to(torch.float32)) for i in range(n)]


def update_ref(y, factors, n_old, delta, max_order, fdt):
    """-> (the n_new factors after a computing forward that saw y, n_new).  `factors`: the n_old valid ones (dtype `fdt`);
    y in the model dtype; `delta`: forwards since the last computing one."""
    g = [y.float().to(fdt)]
    for i in range(min(n_old, max_order)):
        diff = g[i].float() - factors[i].float()
        g.append((diff / torch.full_like(diff, float(delta))).to(fdt))
    return g, min(n_old + 1, max_order + 1)


def update_planes_ref(y, planes, n_old, delta):
    """the kernel's form: `planes` [P, rows, D] of dtype F with n_old valid ones -> (planes after the update, n_new); planes at
    and beyond n_new keep their values"""
    g, n_new = update_ref(y, [planes[i] for i in range(n_old)], n_old, delta, planes.shape[0] - 1, planes.dtype)
    out = planes.clone()
    for i in range(n_new):
        out[i] = g[i]
    return out, n_new


def predict_f32(factors, n, k):
    """p in fp32: p = f_0; p = p + f_i * c_i, the product and the sum each one fp32 operation"""
    c = coefficients(k, n)
    p = factors[0].float()
    for i in range(1, n):
        p = p + factors[i].float() * torch.full_like(p, c[i])
    return p


def predict_ref(factors, n, k, dtype, x=None):
    """T(p), or T(x + p): every operation a single fp32 rounding that torch repeats"""
    p = predict_f32(factors, n, k)
    return (p if x is None else x.float() + p).to(dtype)


def predict_ref64(factors, n, k, x=None, gate=None):
    """float64: p from the float32 coefficients the kernel is given, then x + p * gate, not rounded"""
    c = coefficients(k, n)
    p = factors[0].double()
    for i in range(1, n):
        p = p + factors[i].double() * c[i]
    if x is None:
        return p
    return x.double() + (p if gate is None else p * gate.double())


class TaylorSeerRef:
    """`ref(context, hidden_states, timestep, text)`: one forward under `context` with the rule of `config` (a
    TaylorSeerCacheConfig).  `log` holds (context, s, computed) like WanTransformer3DModel.cache_log.  `order`: overrides the
    order a PREDICTION uses (0: re-use of the last computed output, what Pyramid Attention Broadcast hands out) without
    changing the schedule or the factors."""

    def __init__(self, sd, cfg, config, order=None):
        self.sd, self.cfg, self.config, self.order = sd, cfg, config, order
        self.state, self.log = {}, []

    def reset(self):
        self.state = {}

    def _factor_dtype(self, y):
        return self.config.taylor_factors_dtype or y.dtype

    def _hooked(self, st, key, compute, k, run):
        """one hooked tensor: computed and folded into the factors, or predicted from them"""
        f = st["factors"].get(key, [])
        if compute:
            y = run()
            st["factors"][key], _ = update_ref(y, f, len(f), k, self.config.max_order, self._factor_dtype(y))
            return y
        n = len(f) if self.order is None else min(len(f), self.order + 1)
        return predict_f32(f, n, k)                    # fp32: the consumer rounds once, as the kernel's epilogue does

    def _block(self, st, compute, k, prefix, x, txt, temb, rot):
        """oracle.wan_dit.wan_block with the two attention outputs routed through the hook"""
        sd, cfg = self.sd, self.cfg
        heads, eps = cfg["num_attention_heads"], cfg["eps"]
        table = sd[prefix + ".scale_shift_table"]
        if temb.ndim == 4:
            mods = (table.unsqueeze(0) + temb.float()).chunk(6, dim=2)
            shift_msa, scale_msa, gate_msa, c_shift, c_scale, c_gate = [m.squeeze(2) for m in mods]
        else:
            shift_msa, scale_msa, gate_msa, c_shift, c_scale, c_gate = (table + temb.float()).chunk(6, dim=1)
        n = (W.fp32_layer_norm(x.float(), None, None, eps) * (1 + scale_msa) + shift_msa).type_as(x)
        a = self._hooked(st, prefix + ".attn1", compute, k, lambda: W.wan_attention(sd, prefix + ".attn1", heads, eps, n, None, rot))
        x = (x.float() + a.float() * gate_msa).type_as(x)
        if cfg.get("cross_attn_norm", True):
            n = W.fp32_layer_norm(x.float(), sd[prefix + ".norm2.weight"], sd[prefix + ".norm2.bias"], eps).type_as(x)
        else:
            n = x.float().type_as(x)
        a = self._hooked(st, prefix + ".attn2", compute, k, lambda: W.wan_attention(sd, prefix + ".attn2", heads, eps, n, txt, None))
        x = (x.float() + a.float()).type_as(x)
        n = (W.fp32_layer_norm(x.float(), None, None, eps) * (1 + c_scale) + c_shift).type_as(x)
        f = W.feed_forward(sd, prefix + ".ffn", n)
        return (x.float() + f.float() * c_gate).type_as(x)

    def __call__(self, context, hidden_states, timestep, txt):
        sd, cfg, config = self.sd, self.cfg, self.config
        st = self.state.setdefault(context, {"s": 0, "n": 0, "s_last": None, "factors": {}})
        s = st["s"]
        compute = bool(taylorseer_decide(s, st["n"], config))
        k = 0 if st["s_last"] is None else s - st["s_last"]
        self.log.append((context, s, compute))
        st["s"] += 1
        if compute:
            st["n"], st["s_last"] = min(st["n"] + 1, config.max_order + 1), s
        pt, ph, pw = cfg["patch_size"]
        b, _, nf, hh, ww = hidden_states.shape
        geo = (b, nf // pt, hh // ph, ww // pw)

        def unpatchify(rows):
            y = rows.reshape(b, geo[1], geo[2], geo[3], pt, ph, pw, -1).permute(0, 7, 1, 4, 2, 5, 3, 6)
            return y.flatten(6, 7).flatten(4, 5).flatten(2, 3)

        def patch_rows(out):
            y = out.reshape(b, -1, geo[1], pt, geo[2], ph, geo[3], pw).permute(0, 2, 4, 6, 3, 5, 7, 1)
            return y.reshape(b, geo[1] * geo[2] * geo[3], -1)

        if config.use_lite_mode and not compute:
            return unpatchify(self._hooked(st, "out", False, k, None).to(hidden_states.dtype))
        x, temb, tproj, txt, rot, geo = _embed(sd, cfg, hidden_states, timestep, txt)
        if config.use_lite_mode:
            for i in range(cfg["num_layers"]):
                x = W.wan_block(sd, f"blocks.{i}", cfg, x, txt, tproj, rot)
            out = _head(sd, cfg, x, temb, geo)
            self._hooked(st, "out", True, k, lambda: patch_rows(out))
            return out
        for i in range(cfg["num_layers"]):
            x = self._block(st, compute, k, f"blocks.{i}", x, txt, tproj, rot)
        return _head(sd, cfg, x, temb, geo)
