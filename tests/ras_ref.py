"""Restatement of region-adaptive sampling (frameino_amd/step_cache.py: RegionAdaptiveSamplingConfig) for the tests: the list
(score and stable selection in float64 / exact order), and a partial forward of the Wan DiT recomposed from oracle.wan_dit pieces
the way tests/window_attn_ref.py does (embedding from tests/step_cache_ref.py) -- given a list and stale per-layer K / V, only the
listed rows run; their k and v replace their rows of K / V before the self-attention of the layer; the other rows keep their
head rows.  Run in the dtype of the state dict it is given; 1-D timesteps ([b] values).  oracle/ itself is not changed."""
import math

import torch

from oracle import wan_dit as W
from tests.step_cache_ref import _embed


# ------------------------------------------------------------------ the list
def score_ref(po, batch=1, counters=None, scale=0.0, eligible=None):
    """po [batch * n, C] -> float64 [n]: the population standard deviation of every row, averaged over the batch elements,
    times exp(scale * counter); eligible 0 -> -inf, 2 -> +inf"""
    n = po.shape[0] // batch
    sd = po.double().view(batch, n, -1).std(dim=-1, unbiased=False).mean(dim=0)
    if counters is not None:
        sd = sd * torch.exp(scale * counters.double())
    if eligible is not None:
        sd = torch.where(eligible == 0, torch.full_like(sd, -math.inf), sd)
        sd = torch.where(eligible == 2, torch.full_like(sd, math.inf), sd)
    return sd


def select_ref(score, k, counters=None):
    """the k largest scores, ties to the lower index, ascending -> (int32 [k], the counters moved on or None): sort by
    (-score, index), take k, sort ascending"""
    order = sorted(range(score.shape[0]), key=lambda i: (-float(score[i]), i))
    idx = torch.tensor(sorted(order[:k]), dtype=torch.int32)
    new = None
    if counters is not None:
        new = counters.clone() + 1
        new[idx.long()] = 0
    return idx, new


def starvation_steps(score_lowest, score_kth, scale):
    """the number of consecutive partial steps a row of score `score_lowest` sits out before exp(scale * k) lifts it above
    a steady `score_kth` (the k-th largest score of rows whose counters stay 0): the smallest k with
    score_lowest * exp(scale * k) > score_kth"""
    return max(0, math.floor(math.log(score_kth / score_lowest) / scale) + 1)


# ------------------------------------------------------------------ the forward
def _mods(sd, prefix, temb):
    return (sd[prefix + ".scale_shift_table"] + temb.float()).chunk(6, dim=1)            # each [b, 1, D]


def _qkv(sd, prefix, heads, eps, n, cos, sin):
    q = W.rms_norm(W.linear(sd, prefix + ".to_q", n), sd[prefix + ".norm_q.weight"], eps)
    k = W.rms_norm(W.linear(sd, prefix + ".to_k", n), sd[prefix + ".norm_k.weight"], eps)
    v = W.linear(sd, prefix + ".to_v", n)
    q, k, v = (t.unflatten(2, (heads, -1)).transpose(1, 2) for t in (q, k, v))
    return W.apply_wan_rope(q, cos, sin), W.apply_wan_rope(k, cos, sin), v


def _block(sd, cfg, prefix, x, txt, temb, rot, idx, kv):
    """oracle.wan_dit.wan_block on the rows `idx` of the sequence (None: all), the self-attention's keys and values from
    `kv` = [K, V] ([b, heads, L, dh], updated in place at the rows that ran)"""
    heads, eps = cfg["num_attention_heads"], cfg["eps"]
    shift_msa, scale_msa, gate_msa, c_shift, c_scale, c_gate = _mods(sd, prefix, temb)
    cos, sin = rot if idx is None else (rot[0][:, :, idx], rot[1][:, :, idx])
    n = (W.fp32_layer_norm(x.float(), None, None, eps) * (1 + scale_msa) + shift_msa).type_as(x)
    q, k, v = _qkv(sd, prefix + ".attn1", heads, eps, n, cos, sin)
    if idx is None:
        kv[0], kv[1] = k, v
    else:
        kv[0][:, :, idx], kv[1][:, :, idx] = k, v
    o = W.sdpa(q, kv[0], kv[1])
    a = W.linear(sd, prefix + ".attn1.to_out.0", o.transpose(1, 2).flatten(2, 3).type_as(q))
    x = (x.float() + a * gate_msa).type_as(x)
    if cfg.get("cross_attn_norm", True):
        n = W.fp32_layer_norm(x.float(), sd[prefix + ".norm2.weight"], sd[prefix + ".norm2.bias"], eps).type_as(x)
    else:
        n = x.float().type_as(x)
    x = x + W.wan_attention(sd, prefix + ".attn2", heads, eps, n, txt, None)
    n = (W.fp32_layer_norm(x.float(), None, None, eps) * (1 + c_scale) + c_shift).type_as(x)
    f = W.feed_forward(sd, prefix + ".ffn", n)
    return (x.float() + f.float() * c_gate).type_as(x)


def _head_rows(sd, cfg, x, temb):
    """norm_out + proj_out of wan_forward on the rows given -> [b, rows, C_out * prod(patch)]"""
    shift, scale = (sd["scale_shift_table"] + temb.unsqueeze(1)).chunk(2, dim=1)
    x = (W.fp32_layer_norm(x.float(), None, None, cfg["eps"]) * (1 + scale) + shift).type_as(x)
    return W.linear(sd, "proj_out", x)


def unpatchify(cfg, po, geo):
    b, ppf, pph, ppw = geo
    pt, ph, pw = cfg["patch_size"]
    x = po.reshape(b, ppf, pph, ppw, pt, ph, pw, -1).permute(0, 7, 1, 4, 2, 5, 3, 6)
    return x.flatten(6, 7).flatten(4, 5).flatten(2, 3)


def ras_forward(sd, cfg, hidden_states, timestep, txt, idx=None, kv=None, po=None):
    """One forward: full (idx None) or over the rows `idx` (an integer tensor) given the stale `kv` (per layer [K, V]) and head
    rows `po` [b, L, C] of earlier forwards -- neither is modified.  -> (prediction [b, C, F, H, W], po, kv)"""
    assert timestep.ndim == 1
    x, temb, tproj, txt, rot, geo = _embed(sd, cfg, hidden_states, timestep, txt)
    if idx is None:
        kv = [[None, None] for _ in range(cfg["num_layers"])]
    else:
        idx = idx.long()
        kv = [[k.clone(), v.clone()] for k, v in kv]
        x = x[:, idx]
    for i in range(cfg["num_layers"]):
        x = _block(sd, cfg, f"blocks.{i}", x, txt, tproj, rot, idx, kv[i])
    rows = _head_rows(sd, cfg, x, temb)
    if idx is None:
        po = rows
    else:
        po = po.clone()
        po[:, idx] = rows
    return unpatchify(cfg, po, geo), po, kv


# ------------------------------------------------------------------ fixtures the CPU and the GPU tests share
LIST_ROWS = 475                 # round(0.4 * 1188): no multiple of 64 or 256


def quantised_scores(n, seed=0, special=True):
    """fp32 [n] scores on 16 levels in [-2, 1.75] (ties everywhere, both signs, both zeros); `special`: a few -inf and +inf
    rows as an eligibility mask leaves them"""
    g = torch.Generator().manual_seed(seed)
    s = torch.randint(0, 16, (n,), generator=g).float() / 4.0 - 2.0
    zeros = (s == 0).nonzero().flatten()
    s[zeros[::2]] = -0.0
    if special and n >= 16:
        s[torch.randperm(n, generator=g)[:max(2, n // 97)]] = -math.inf
        s[torch.randperm(n, generator=g)[:max(1, n // 301)]] = math.inf
    return s


def starved_rows(n=1188, cols=192, seed=3, scale=0.1):
    """(po bf16 [n, cols], counters int32 [n], row): `row` has the smallest standard deviation of all, and a counter that
    alone lifts it onto a list of LIST_ROWS"""
    g = torch.Generator().manual_seed(seed)
    po = (torch.randn(n, cols, generator=g) * (0.5 + torch.rand(n, 1, generator=g))).bfloat16()
    row = 700
    po[row] = po[row] * 0.05
    counters = torch.randint(0, 3, (n,), generator=g, dtype=torch.int32)
    counters[row] = 45          # exp(4.5) = 90: 0.05 * 90 = 4.5 x the typical score
    return po, counters, row
