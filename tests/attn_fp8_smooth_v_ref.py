"""Torch restatement of the fp8 attention's quantisation with smooth K and smooth V (fino_attn_fwd_fp8_smoothed,
csrc/fino_attention_fp8.hip): tests/attn_fp8_ref.py::emulated extended with `smooth_v` (the mean of V over the keys leaves V
before it is quantised and joins the normalised output again), an optional key mask (the range walk), and the one rounding to the
storage dtype the kernel ends with.  Plus the seeded inputs, the ulp helper and the tail-split plan the smooth-V tests share between
their CPU and GPU halves.  Runs on any device."""
import math

import torch
import torch.nn.functional as F

from tests.attn_fp8_ref import LOG2E, OFFSET_SHAPES, mxq, sdpa  # noqa: F401  (re-exported for the tests)

OFFSET_C = 8.0
# what the offset must cost the plain emulation on the seeded inputs, per storage dtype: in bf16 the rounding of an output of
# magnitude ~8 (2^-8 relative) is a floor both share
CONDITION = {torch.float16: 3.0, torch.bfloat16: 1.45}


def emulated(q, k, v, heads, p_mode="exp2", smooth_k=False, smooth_v=False, mask=None):
    """the kernel's quantisation in plain torch (fp32 everywhere else, exact running maximum), rounded to q's dtype at the end and
    returned as fp32.  smooth_k / smooth_v: the mean over ALL keys, per (batch element, head, channel), leaves K / V before the
    quantiser; V's joins the normalised output again.  mask: bool [lq, lk], the keys each query row walks (a row without keys: 0)."""
    b, lq, hd = q.shape
    dh = hd // heads
    lk = k.shape[1]
    qh, kh, vh = (t.float().view(b, -1, heads, dh).transpose(1, 2) for t in (q, k, v))
    if smooth_k:
        kh = kh - kh.mean(2, keepdim=True)
    mu = vh.mean(2, keepdim=True) if smooth_v else torch.zeros_like(vh[:, :, :1])
    vh = vh - mu
    q8 = mxq(qh * (dh ** -0.5 * LOG2E))
    k8 = mxq(kh)
    v8 = mxq(F.pad(vh, (0, 0, 0, (-lk) % 32)), dim=2)[:, :, :lk]
    s = q8 @ k8.transpose(2, 3)
    if mask is not None:
        s = s.masked_fill(~mask, float("-inf"))
    top = s.amax(-1, keepdim=True)
    top = torch.where(torch.isfinite(top), top, torch.zeros_like(top))
    if p_mode == "ramp":
        m = torch.round(top - 6)
        p8 = torch.round(8 * (s - m) + 55.5).clamp(0, 126).to(torch.uint8).view(torch.float8_e4m3fn).float()
    else:
        p8 = (torch.exp2(s - top) * 64).to(torch.float8_e4m3fn).float() / 64
    l = p8.sum(-1, keepdim=True)
    o = torch.where(l > 0, (p8 @ v8) / l.clamp_min(1e-30) + mu, torch.zeros_like(mu))
    return o.transpose(1, 2).reshape(b, lq, hd).to(q.dtype).float()


def sdpa_masked(q, k, v, heads, mask):
    """fp32 SDPA under a bool [lq, lk] key mask; a query row without keys gives 0"""
    b, lq, hd = q.shape
    dh = hd // heads
    qh, kh, vh = (t.float().view(b, -1, heads, dh).transpose(1, 2) for t in (q, k, v))
    s = (qh @ kh.transpose(2, 3) * dh ** -0.5).masked_fill(~mask, float("-inf"))
    p = torch.nan_to_num(torch.softmax(s, dim=-1), nan=0.0)
    return (p @ vh).transpose(1, 2).reshape(b, lq, hd)


def offset_v_inputs(b, heads, lq, lk, dh, dtype, device="cpu", c=OFFSET_C):
    """q, k = N(0, 1); V = N(0, 1) + c * N(0, 1) per (batch element, channel), the offset shared by every key.  Generated on the
    CPU from a seed (the same numbers wherever the test runs); k | v are row-strided views of one buffer."""
    d = heads * dh
    g = torch.Generator().manual_seed(3000 * dh + lq + lk + heads)
    q = torch.randn(b, lq, d, generator=g).to(dtype)
    kv = torch.randn(b, lk, 2 * d + 64, generator=g)
    kv[:, :, d:2 * d] += c * torch.randn(b, 1, d, generator=g)
    kv = kv.to(dtype).to(device)
    return q.to(device), kv[:, :, :d], kv[:, :, d:2 * d]


def constant_c(b, d):
    """odd integers in [33, 63], one per (batch element, channel): exact in bf16 / fp16 (6 significant bits), not in e4m3 (4).
    Different per batch element, per channel and per 64-channel sub-head: c[bi, ch] = 33 + 2 ((7 ch + 5 bi + 3 (ch // 64)) % 16)"""
    ch = torch.arange(d)
    bi = torch.arange(b)[:, None]
    return (33 + 2 * ((7 * ch[None] + 5 * bi + 3 * (ch[None] // 64)) % 16)).float()


def ulp(x, dtype):
    """one unit in the last place of |x| in `dtype` (bf16: 8 significant bits, fp16: 11; fp16 subnormals below 2^-14)"""
    bits = 8 if dtype == torch.bfloat16 else 11
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -14 if dtype == torch.float16 else 2.0 ** -126)))
    return torch.exp2(e - (bits - 1))


def plan_split(batch, heads, nqb, nt, cus):
    """csrc/fino_attention.hip::plan_split restated: (full_x, rem_x, nwg, per) of the head_dim 128 tail split on a device of `cus`
    compute units; rem_x = 0: every block runs whole.  (fino_attn_fwd_fp8 also needs nwg <= 32 to split.)"""
    cus_x = max(cus // 8, 1)
    hb = batch * heads
    vsplit = 8 // math.gcd(hb, 8)
    if vsplit > nqb:
        vsplit = 1
    nqb_v = -(-nqb // vsplit)
    nblk_x = -(-hb * vsplit // 8) * nqb_v
    rem = nblk_x % cus_x
    whole = (nblk_x, 0, 0, 1)
    if rem == 0:
        return whole
    total = rem * nt
    nwg = min(cus_x, total // 8)
    if nwg <= rem:
        return whole
    per = -(-total // nwg)
    if per >= nt:
        return whole
    return nblk_x - rem, rem, -(-total // per), per


def table_mask(table, lq, lk, device="cpu"):
    """int32 [ceil(lq / 256), 3, 2] table of 64-key tile ranges -> bool [lq, lk], clipped as the kernel clips"""
    nt = -(-lk // 64)
    mask = torch.zeros(lq, lk, dtype=torch.bool, device=device)
    for i, blk in enumerate(table.tolist()):
        for s, e in blk:
            s = min(max(int(s), 0), nt)
            e = min(max(int(e), s), nt)
            mask[256 * i:256 * i + 256, 64 * s:min(64 * e, lk)] = True
    return mask
