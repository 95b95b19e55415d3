"""Torch restatement of the fp8 attention's quantisation with smooth Q (fino_attn_fwd_fp8_smooth_q, csrc/fino_attention_fp8.hip):
tests/attn_fp8_smooth_v_ref.py::emulated extended with `smooth_q` -- the mean of q over each block of 256 consecutive query rows
(per batch element, head and channel; a ragged last block averages over the rows it has) leaves q before it is quantised, and
qbar . k_key, from the unquantised (smoothed, with smooth_k) keys and rounded to the kernel's hi | lo pair of the storage dtype,
joins the logits.  Plus the seeded inputs and shapes the smooth-Q tests share between their CPU and GPU halves.  Runs on any
device."""
import torch
import torch.nn.functional as F

from tests.attn_fp8_ref import LOG2E, mxq, sdpa  # noqa: F401  (re-exported for the tests)

Q_BLOCK = 256
OFFSET_C = 8.0
# (b, heads, lq, lk); heads halved at head_dim 128.  A full block; a second, ragged block of 44 rows, a ragged last key tile, batch
# and head strides; a block of 33 rows with a nearly one-hot softmax (closeness only: excluded from the condition's ratio)
SHAPES = [(1, 2, 256, 320), (2, 3, 300, 1000), (1, 1, 33, 65)]
CONDITION_SHAPES = SHAPES[:2]
CONDITION = 2.0           # the plain emulation's rel-RMS against fp32 SDPA is at least this many times the smoothed emulation's


def heads_at(heads, dh):
    return heads if dh == 64 else max(1, heads // 2)


def block_mean(x, block=Q_BLOCK):
    """x [..., rows, channels] -> the mean over each block of `block` consecutive rows, repeated over the block's rows"""
    rows = x.shape[-2]
    out = torch.empty_like(x)
    for r0 in range(0, rows, block):
        out[..., r0:r0 + block, :] = x[..., r0:r0 + block, :].mean(-2, keepdim=True)
    return out


def pair(x, dtype):
    """the kernel's table entry: hi = T(x), lo = T(x - hi), read back as hi + lo"""
    hi = x.to(dtype).float()
    return hi + (x - hi).to(dtype).float()


def emulated(q, k, v, heads, p_mode="exp2", smooth_k=False, smooth_v=False, smooth_q=False):
    """the kernel's quantisation in plain torch (fp32 everywhere else, exact running maximum), rounded to q's dtype at the end and
    returned as fp32"""
    b, lq, hd = q.shape
    dh = hd // heads
    lk = k.shape[1]
    qh, kh, vh = (t.float().view(b, -1, heads, dh).transpose(1, 2) for t in (q, k, v))
    if smooth_k:
        kh = kh - kh.mean(2, keepdim=True)
    mu = vh.mean(2, keepdim=True) if smooth_v else torch.zeros_like(vh[:, :, :1])
    vh = vh - mu
    pre = dh ** -0.5 * LOG2E
    bias = 0.0
    if smooth_q:
        qbar = block_mean(qh)
        bias = pair(pre * (qbar @ kh.transpose(2, 3)), q.dtype)
        qh = qh - qbar
    q8 = mxq(qh * pre)
    k8 = mxq(kh)
    v8 = mxq(F.pad(vh, (0, 0, 0, (-lk) % 32)), dim=2)[:, :, :lk]
    s = q8 @ k8.transpose(2, 3) + bias
    top = s.amax(-1, keepdim=True)
    if p_mode == "ramp":
        m = torch.round(top - 6)
        p8 = torch.round(8 * (s - m) + 55.5).clamp(0, 126).to(torch.uint8).view(torch.float8_e4m3fn).float()
    else:
        p8 = (torch.exp2(s - top) * 64).to(torch.float8_e4m3fn).float() / 64
    o = (p8 @ v8) / p8.sum(-1, keepdim=True) + mu
    return o.transpose(1, 2).reshape(b, lq, hd).to(q.dtype).float()


def offset_q_inputs(b, heads, lq, lk, dh, dtype, device="cpu", c=OFFSET_C):
    """q, k, v = N(0, 1); q gets an offset c * N(0, 1) per (256-row block, head, channel), shared by the batch.  Generated on the CPU
    from a seed (the same numbers wherever the test runs); k | v are row-strided views of one buffer."""
    d = heads * dh
    g = torch.Generator().manual_seed(7000 * dh + lq + lk + heads)
    q = torch.randn(b, lq, d, generator=g)
    off = c * torch.randn(-(-lq // Q_BLOCK), d, generator=g)
    q = (q + off.repeat_interleave(Q_BLOCK, 0)[:lq]).to(dtype)
    kv = torch.randn(b, lk, 2 * d + 64, generator=g).to(dtype).to(device)
    return q.to(device), kv[:, :, :d], kv[:, :, d:2 * d]


def block_constant_inputs(b, heads, lq, lk, dh, dtype, device="cpu"):
    """within each 256-row block every query row is the same N(0, 1) row (another one per batch element, block and head channel):
    q - qbar = 0 up to the mean's rounding, so every logit comes from the bias table.  k, v = N(0, 1)."""
    d = heads * dh
    g = torch.Generator().manual_seed(9000 * dh + lq + lk + heads)
    rows = torch.randn(b, -(-lq // Q_BLOCK), d, generator=g)
    q = rows.repeat_interleave(Q_BLOCK, 1)[:, :lq].to(dtype)
    kv = torch.randn(b, lk, 2 * d + 64, generator=g).to(dtype).to(device)
    return q.contiguous().to(device), kv[:, :, :d], kv[:, :, d:2 * d]
