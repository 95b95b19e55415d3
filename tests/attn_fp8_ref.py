"""Torch restatement of the quantisation of fino_attn_fwd_fp8 / fino_attn_fwd_fp8_smooth (csrc/fino_attention_fp8.hip): the
`_mxq` / `_sdpa` / `_emulated` of tests/test_attention_fp8_gpu.py with a `smooth_k` argument, plus the seeded inputs the smooth-K
tests share between their CPU and GPU halves.  Runs on any device (the CPU test checks the inputs' condition without a GPU)."""
import torch

LOG2E = 1.4426950408889634
# (b, heads, lq, lk) of the offset-key test: a full tile, a ragged last tile (key tile = 64), several 256-key chunks of the mean,
# batch / head strides; the heads are halved at head_dim 128
OFFSET_SHAPES = [(1, 2, 256, 320), (2, 3, 300, 1000), (1, 1, 33, 65)]
OFFSET_C = 8.0


def mxq(x, dim=-1, block=32):
    """block-scaled e4m3: one power-of-two scale per `block` elements along `dim`, amax / scale in (224, 448]"""
    x = x.transpose(dim, -1)
    shp = x.shape
    xb = x.reshape(*shp[:-1], shp[-1] // block, block)
    amax = xb.abs().amax(-1, keepdim=True).clamp_min(1e-30)
    s = torch.exp2(torch.ceil(torch.log2(amax / 448.0)))
    q = (xb / s).to(torch.float8_e4m3fn).float() * s
    return q.reshape(shp).transpose(dim, -1)


def sdpa(q, k, v, heads):
    """fp32 softmax(q k^T / sqrt(dh)) v on [b, l, heads * dh] operands"""
    b, lq, hd = q.shape
    dh = hd // heads
    qh, kh, vh = (t.float().view(b, -1, heads, dh).transpose(1, 2) for t in (q, k, v))
    p = torch.softmax(qh @ kh.transpose(2, 3) * dh ** -0.5, dim=-1)
    return (p @ vh).transpose(1, 2).reshape(b, lq, hd)


def emulated(q, k, v, heads, p_mode="exp2", smooth_k=False):
    """the kernel's quantisation in plain torch (fp32 everywhere else, exact running maximum); smooth_k: the mean of K over the
    keys, per (batch element, head, channel), leaves K before it is quantised"""
    b, lq, hd = q.shape
    dh = hd // heads
    lk = k.shape[1]
    pad = (-lk) % 32
    qh, kh, vh = (t.float().view(b, -1, heads, dh).transpose(1, 2) for t in (q, k, v))
    if smooth_k:
        kh = kh - kh.mean(2, keepdim=True)
    q8 = mxq(qh * (dh ** -0.5 * LOG2E))
    k8 = mxq(kh)
    vp = torch.nn.functional.pad(vh, (0, 0, 0, pad))
    v8 = mxq(vp, dim=2)[:, :, :lk]
    s = q8 @ k8.transpose(2, 3)
    if p_mode == "ramp":
        # the byte IS rne(8 (s - m) + 55.5) with m a whole number of octaves (the maximum lands near 2^6); 0 below, <= 0x7e above
        m = torch.round(s.amax(-1, keepdim=True) - 6)
        byte = torch.round(8 * (s - m) + 55.5).clamp(0, 126).to(torch.uint8)
        p8 = byte.view(torch.float8_e4m3fn).float()
    else:
        p = torch.exp2(s - s.amax(-1, keepdim=True))
        p8 = (p * 64).to(torch.float8_e4m3fn).float() / 64
    return ((p8 @ v8) / p8.sum(-1, keepdim=True)).transpose(1, 2).reshape(b, lq, hd)


def offset_inputs(b, heads, lq, lk, dh, dtype, device="cpu"):
    """q, v = N(0, 1); K = N(0, 1) + OFFSET_C * N(0, 1) per (head, channel), the offset shared by every key and batch element.
    Generated on the CPU from a seed (the same numbers wherever the test runs); k | v are row-strided views of one buffer."""
    d = heads * dh
    g = torch.Generator().manual_seed(1000 * dh + lq + lk + heads)
    q = torch.randn(b, lq, d, generator=g).to(dtype)
    kv = torch.randn(b, lk, 2 * d + 64, generator=g)
    kv[:, :, :d] += OFFSET_C * torch.randn(d, generator=g)
    kv = kv.to(dtype).to(device)
    return q.to(device), kv[:, :, :d], kv[:, :, d:2 * d]
