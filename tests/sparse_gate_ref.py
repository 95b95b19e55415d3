"""CPU restatement, in float64, of the two safeguards of the dynamic block-sparse self-attention (DESIGN.md section 6k;
csrc/fino_attention_plan.hip: fino_attn_tile_plan_gated) and of the calibration's choice (frameino_amd/sparse_calibration.py), for
the tests.  Written from the definitions, sharing nothing with the kernels; the ungated parts are tests/sparse_attn_ref.py's.

similarity: per (b, h), for a block of n rows x_r: u = (1 / n) sum_r x_r / |x_r|_2 (a zero row adds 0), sim = |u|^2 -- the mean
            cosine over all ordered row pairs, self pairs included.  sim_q per 256-row q-block, sim_k per 64-key tile (the ragged
            last tile: its real keys).
gate:       theta > 0.  U = {t : sim_k[t] < theta}.  sim_q[i] < theta: every tile.  Otherwise the tiles of U are kept and take no
            part in the prediction (p_t = 0 there: not in the maximum, not in sum w); the rule of sparse_attn_ref.select_row runs
            over the rest with the forced set F, m_F counting F \\ U; kept = U + F + {p_t >= theta_p}.  sum w = 0 (every tile in
            U): U + F alone.
per head:   head h uses cdf_heads[h]; a value >= 1 keeps every tile of that head.
calibration: err[g] = sum |o_g - o_d| / sum |o_d| per head; the threshold is the smallest grid value g such that g and every
            larger grid value have err <= bound, else 1.0."""
import math

import torch

from tests import sparse_attn_ref as R


def _block_similarity(x):
    """x [B, H, n, dh] float64 -> [B, H]"""
    norm = x.norm(dim=-1, keepdim=True)
    unit = torch.where(norm > 0, x / norm.clamp_min(1e-300), torch.zeros_like(x))
    return unit.mean(2).pow(2).sum(-1)


def similarity(q, k, heads):
    """q [B, Lq, H dh], k [B, Lk, H dh] -> (sim_q [B, H, nqb], sim_k [B, H, nt]) in float64"""
    b, lq, hd = q.shape
    lk, dh = k.shape[1], hd // heads
    q = q.detach().cpu().double().reshape(b, lq, heads, dh).transpose(1, 2)
    k = k.detach().cpu().double().reshape(b, lk, heads, dh).transpose(1, 2)
    sq = torch.stack([_block_similarity(q[:, :, R.Q_BLOCK * i:min(R.Q_BLOCK * (i + 1), lq)]) for i in range(R.nqblocks(lq))], dim=2)
    sk = torch.stack([_block_similarity(k[:, :, R.KEY_TILE * t:min(R.KEY_TILE * (t + 1), lk)]) for t in range(R.ntiles(lk))], dim=2)
    return sq, sk


def gated_probs(q, k, heads, theta, scale=None, folded=False):
    """-> (p [B, H, nqb, nt] float64 with p = 0 on the unpredictable tiles, dense bool [B, H, nqb], unpred bool [B, H, nt]).
    theta None or <= 0: the gate is off, p is sparse_attn_ref.tile_probs.  A (b, h) whose tiles are all unpredictable has p = 0."""
    qbar, kbar, n = R.pool(q, k, heads)
    if theta is None or theta <= 0:
        return (R.tile_probs(q, k, heads, scale, folded), torch.zeros(qbar.shape[:3], dtype=torch.bool),
                torch.zeros(kbar.shape[:3], dtype=torch.bool))
    sq, sk = similarity(q, k, heads)
    dense, unpred = sq < theta, sk < theta
    s = qbar @ kbar.transpose(-1, -2)
    s = s * math.log(2.0) if folded else s * (qbar.shape[-1] ** -0.5 if scale is None else scale)
    s = s.masked_fill(unpred[:, :, None, :], -math.inf)
    mx = s.amax(-1, keepdim=True)
    w = torch.where(unpred[:, :, None, :].expand_as(s), torch.zeros_like(s), n * torch.exp(s - torch.where(mx.isinf(), torch.zeros_like(mx), mx)))
    tot = w.sum(-1, keepdim=True)
    return torch.where(tot > 0, w / tot.clamp_min(1e-300), torch.zeros_like(w)), dense, unpred


def gated_select(p, forced, cdf, dense, unpred, cdf_heads=None):
    """p [B, H, nqb, nt], forced [nqb, nt], dense [B, H, nqb], unpred [B, H, nt] -> bool [B, H, nqb, nt]"""
    out = torch.zeros(p.shape, dtype=torch.bool)
    for b in range(p.shape[0]):
        for h in range(p.shape[1]):
            c = float(cdf if cdf_heads is None else cdf_heads[h])
            for i in range(p.shape[2]):
                if bool(dense[b, h, i]) or (cdf_heads is not None and c >= 1.0):
                    out[b, h, i] = True
                elif float(p[b, h, i].sum()) == 0.0:                              # sum w = 0: U and F alone
                    out[b, h, i] = forced[i] | unpred[b, h]
                else:
                    out[b, h, i] = R.select_row(p[b, h, i], forced[i] | unpred[b, h], c)
    return out


def plan_gated(q, k, heads, cdf, keep_ranges=None, theta=None, cdf_heads=None, scale=None, folded=False):
    """-> (keep bool [B, H, nqb, nt], p, dense, unpred)"""
    p, dense, unpred = gated_probs(q, k, heads, theta, scale, folded)
    forced = R.forced_tiles(keep_ranges, p.shape[2], p.shape[3])
    return gated_select(p, forced, cdf, dense, unpred, cdf_heads), p, dense, unpred


def attention(q, k, v, heads, keep=None, scale=None):
    """float64 SDPA of q [B, Lq, H dh], k / v [B, Lk, H dh] under the tile mask `keep` [B, H, nqb, nt] (None: dense) -> [B, H, Lq, dh]"""
    b, lq, hd = q.shape
    lk, dh = k.shape[1], hd // heads
    q, k, v = (t.detach().cpu().double().reshape(b, t.shape[1], heads, dh).transpose(1, 2) for t in (q, k, v))
    s = q @ k.transpose(-1, -2) * (dh ** -0.5 if scale is None else scale)
    if keep is not None:
        s = s.masked_fill(~R.expand_mask(keep, lq, lk), -math.inf)
    return torch.softmax(s, dim=-1) @ v


def l1_errors(q, k, v, heads, grid, keep_ranges=None, theta=None):
    """-> err [H, len(grid)] float64: sum |o_g - o_d| / sum |o_d| per head over all rows and batch elements"""
    o_d = attention(q, k, v, heads)
    ref = o_d.abs().sum((0, 2, 3))
    cols = []
    for g in grid:
        keep = plan_gated(q, k, heads, g, keep_ranges, theta)[0]
        cols.append((attention(q, k, v, heads, keep) - o_d).abs().sum((0, 2, 3)) / ref)
    return torch.stack(cols, dim=1)


def choose(err, grid, bound):
    """err [..., len(grid)], grid ascending -> the smallest g such that g and every larger grid value have err <= bound, else 1.0"""
    err = torch.as_tensor(err, dtype=torch.float64)
    out = torch.ones(err.shape[:-1], dtype=torch.float64)
    ok = torch.ones(err.shape[:-1], dtype=torch.bool)
    for j in range(len(grid) - 1, -1, -1):
        ok = ok & (err[..., j] <= bound)
        out = torch.where(ok, torch.full_like(out, float(grid[j])), out)
    return out
