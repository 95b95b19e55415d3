"""CPU restatement, in float64, of the dynamic block-sparse self-attention's predictor (csrc/fino_attention_plan.hip,
`ops.attention_tile_plan`) and of the mask layout of `ops.attention_tiles`, for the tests.  Written from
the definition, sharing nothing with the kernels or with frameino_amd/window_attention.py's packing helpers.

pool:    qbar[b, h, i] = mean of q over rows [256 i, min(256 (i + 1), lq)); kbar[b, h, t] = mean of k over the real keys of tile t.
select:  s_t = scale <qbar, kbar_t>, w_t = n_t exp(s_t - max s), p_t = w_t / sum w (n_t: real keys of tile t).  F = the forced
         tiles, m_F their mass.  m_F >= cdf keeps F; else F and every t outside F with p_t >= theta, theta the LARGEST value among
         the p outside F with m_F + sum_{t not in F, p_t >= theta} p_t >= cdf (none: everything).  Ties at theta are all kept."""
import math

import torch

Q_BLOCK, KEY_TILE = 256, 64


def ntiles(lk):
    return -(-int(lk) // KEY_TILE)


def nqblocks(lq):
    return -(-int(lq) // Q_BLOCK)


def pool(q, k, heads):
    """q [B, Lq, H dh], k [B, Lk, H dh] -> (qbar [B, H, nqb, dh], kbar [B, H, nt, dh], n [nt]) in float64"""
    b, lq, hd = q.shape
    lk, dh = k.shape[1], hd // heads
    q = q.detach().cpu().double().reshape(b, lq, heads, dh).transpose(1, 2)
    k = k.detach().cpu().double().reshape(b, lk, heads, dh).transpose(1, 2)
    qbar = torch.stack([q[:, :, Q_BLOCK * i:min(Q_BLOCK * (i + 1), lq)].mean(2) for i in range(nqblocks(lq))], dim=2)
    kbar = torch.stack([k[:, :, KEY_TILE * t:min(KEY_TILE * (t + 1), lk)].mean(2) for t in range(ntiles(lk))], dim=2)
    n = torch.tensor([min(KEY_TILE * (t + 1), lk) - KEY_TILE * t for t in range(ntiles(lk))], dtype=torch.float64)
    return qbar, kbar, n


def tile_probs(q, k, heads, scale=None, folded=False):
    """p [B, H, nqb, nt] float64.  `folded`: q already carries scale * log2(e), the logits are in log2 units"""
    qbar, kbar, n = pool(q, k, heads)
    s = qbar @ kbar.transpose(-1, -2)
    s = s * math.log(2.0) if folded else s * (qbar.shape[-1] ** -0.5 if scale is None else scale)
    w = n * torch.exp(s - s.amax(-1, keepdim=True))
    return w / w.sum(-1, keepdim=True)


def forced_tiles(keep_ranges, nqb, nt):
    """[nqb, 3, 2] table (or None) -> bool [nqb, nt], every range clipped to [0, nt]"""
    f = torch.zeros(nqb, nt, dtype=torch.bool)
    if keep_ranges is not None:
        for i, blk in enumerate(torch.as_tensor(keep_ranges).tolist()):
            for a, b in blk:
                a = min(max(int(a), 0), nt)
                b = min(max(int(b), a), nt)
                f[i, a:b] = True
    return f


def select_row(p, forced, cdf):
    """one row: p [nt] float64, forced bool [nt] -> bool [nt]"""
    m_f = float(p[forced].sum())
    if m_f >= cdf:
        return forced.clone()
    free = ~forced
    for theta in sorted(set(p[free].tolist()), reverse=True):
        if m_f + float(p[free & (p >= theta)].sum()) >= cdf:
            return forced | (free & (p >= theta))
    return torch.ones_like(forced)


def select(p, forced, cdf):
    """p [B, H, nqb, nt], forced [nqb, nt] -> bool [B, H, nqb, nt]"""
    out = torch.zeros(p.shape, dtype=torch.bool)
    for b in range(p.shape[0]):
        for h in range(p.shape[1]):
            for i in range(p.shape[2]):
                out[b, h, i] = select_row(p[b, h, i], forced[i], cdf)
    return out


def plan(q, k, heads, cdf, keep_ranges=None, scale=None, folded=False):
    p = tile_probs(q, k, heads, scale, folded)
    return select(p, forced_tiles(keep_ranges, p.shape[2], p.shape[3]), cdf), p


def pack_mask(keep, words=None):
    """bool [..., nt] -> int32 [..., words]: bit t & 31 of word t >> 5 stands for tile t"""
    nt = keep.shape[-1]
    words = (nt + 31) // 32 if words is None else words
    flat = keep.reshape(-1, nt).tolist()
    out = []
    for row in flat:
        ws = [0] * words
        for t, on in enumerate(row):
            if on:
                ws[t >> 5] |= 1 << (t & 31)
        out.append([w - (1 << 32) if w >= (1 << 31) else w for w in ws])
    return torch.tensor(out, dtype=torch.int32).reshape(keep.shape[:-1] + (words,))


def unpack_mask(mask, nt):
    """int32 / uint32 [..., words] -> bool [..., nt]; bits at or beyond nt are dropped"""
    m = mask.detach().cpu()
    flat = m.reshape(-1, m.shape[-1]).tolist()
    out = [[bool(((row[t >> 5] & 0xffffffff) >> (t & 31)) & 1) for t in range(nt)] for row in flat]
    return torch.tensor(out, dtype=torch.bool).reshape(m.shape[:-1] + (nt,))


def expand_mask(keep, lq, lk):
    """bool [B, H, nqb, nt] (size-1 dims stay) -> bool [B, H, lq, lk]: what `ops.attention_tiles` computes under it"""
    return keep.repeat_interleave(Q_BLOCK, dim=2)[:, :, :lq].repeat_interleave(KEY_TILE, dim=3)[..., :lk]
