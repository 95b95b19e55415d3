"""Torch-tensor front end of the C ABI (include/frameino_hip.h).

PyTorch is plumbing here: it owns device memory and the HIP stream; every op below forwards raw
pointers + strides to libframeino_hip.so on torch's *current* stream (so the calls are capturable in a
torch.cuda.CUDAGraph == hipGraph).  No op has a torch/CPU fallback.
"""
import math
import os

import torch

from . import _lib

BF16, F16 = 0, 1
EPI_NONE, EPI_GELU_TANH, EPI_RESIDUAL, EPI_GATED_RESIDUAL, EPI_GATED_RESIDUAL_STAGED = 0, 1, 2, 3, 4
EPI_F32, EPI_F32_RESIDUAL = 5, 6           # fp32 output of a split-bf16 product (gemm_f32)


class KernelTimer:
    """HIP-event timing of named kernel launches on the stream they are launched on (used by bench.py for the
    live `roofline.achieved` figure).  `with KernelTimer({"attn_self"}) as kt: ...; kt.summary()`."""

    active = None

    def __init__(self, names):
        self.names = set(names)
        self.events = {n: [] for n in self.names}
        self.flops = {}
        self.bytes = {}

    def __enter__(self):
        KernelTimer.active = self
        return self

    def __exit__(self, *exc):
        KernelTimer.active = None

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for n, evs in self.events.items():
            ms = [s.elapsed_time(e) for s, e in evs]
            if ms:
                out[n] = {"launches": len(ms), "avg_us": 1e3 * sum(ms) / len(ms), "total_ms": sum(ms)}
        return out


def _timed(name):
    kt = KernelTimer.active
    if kt is None or name not in kt.names:
        return None
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kt.events[name].append((s, e))
    s.record()
    return e


def _timed_gemm(epilogue, flops, nbytes=0.0):
    """a GEMM launch under KernelTimer: counted under "gemm_epi<epilogue>" (bench.py's roofline.secondary rows: one per epilogue
    class of the block GEMMs) when that name is asked for, else under "gemm"; `epilogue` None (the MX GEMMs, the two-output
    split, the blocked-A GEMM): always under "gemm".  Returns a closure to call after the launch."""
    kt = KernelTimer.active
    if kt is None:
        return None
    name = "gemm" if epilogue is None else f"gemm_epi{int(epilogue)}"
    if name not in kt.names:
        name = "gemm"
        if name not in kt.names:
            return None
    ev = _timed(name)

    def done():
        ev.record()
        kt.flops[name] = kt.flops.get(name, 0.0) + flops
        kt.bytes[name] = kt.bytes.get(name, 0.0) + nbytes
    return done


def _dt(t):
    if t.dtype == torch.bfloat16:
        return BF16
    if t.dtype == torch.float16:
        return F16
    raise TypeError(f"frameino_amd: activations must be bf16 or fp16, got {t.dtype}")


F32 = 2          # FINO_F32: fp32 STORAGE (the Wan VAE's rearrangement kernels in its fp32-faithful mode); never an MFMA operand type


def _dt3(t):
    return F32 if t.dtype == torch.float32 else _dt(t)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return 0 if t is None else t.data_ptr()


def _rows2d(t):
    """View [..., D] with contiguous last dim and uniform row stride as (rows, D, ld)."""
    if not t.is_cuda:
        raise RuntimeError("frameino_amd ops need CUDA(HIP) tensors; there is no CPU path")
    if t.stride(-1) != 1:
        raise ValueError("last dimension must be contiguous")
    t2 = t if t.dim() == 2 else t.reshape(-1, t.shape[-1]) if t.is_contiguous() else None
    if t2 is None:
        if t.dim() == 3 and t.shape[0] == 1:
            t2 = t[0]
        else:
            raise ValueError("need a 2-D row-strided view")
    return t2, t2.shape[0], t2.shape[1], t2.stride(0)


def _epi_operands(residual, gate):
    """(residual as 2-D rows or None, its leading dimension, the gate's row stride) as the GEMM entry points take them"""
    r2, ldr = (None, 0)
    if residual is not None:
        r2, _, _, ldr = _rows2d(residual)
    return r2, ldr, gate.stride(0) if (gate is not None and gate.dim() == 2) else 0


def _mx_pair(shape, scale_bytes, device, out):
    """the (q, scales) pair an MX producer writes: `out`, or fresh element bytes + zeroed scale bytes"""
    if out is not None:
        return out
    return (torch.empty(shape, dtype=torch.uint8, device=device), torch.zeros(scale_bytes, dtype=torch.uint8, device=device))


def adaln_modulate(x, shift, scale, sel=None, eps=1e-6, out=None):
    """y = T(LN(x)*(1+scale[sel])+shift[sel]).  shift/scale: fp32 [R, D] views of one table (same row stride)."""
    x2, rows, dim, ldx = _rows2d(x)
    out = torch.empty_like(x2) if out is None else out
    o2, _, _, ldy = _rows2d(out)
    assert shift.dtype == torch.float32 and scale.dtype == torch.float32
    ms = shift.stride(0) if shift.dim() == 2 else 0
    if scale.dim() == 2:
        assert scale.stride(0) == ms
    _lib.check(_lib.lib().fino_adaln_modulate(_p(x2), _p(o2), rows, dim, ldx, ldy, _p(shift), _p(scale), ms, _p(sel),
                                             eps, _dt(x), _stream()), "fino_adaln_modulate")
    return out.view(x.shape) if out.shape != x.shape and out.numel() == x.numel() else out


def layernorm(x, weight=None, bias=None, eps=1e-5, out=None):
    x2, rows, dim, ldx = _rows2d(x)
    out = torch.empty_like(x2) if out is None else out
    o2, _, _, ldy = _rows2d(out)
    for t in (weight, bias):
        assert t is None or t.dtype == torch.float32
    _lib.check(_lib.lib().fino_layernorm(_p(x2), _p(o2), rows, dim, ldx, ldy, _p(weight), _p(bias), eps, _dt(x),
                                        _stream()), "fino_layernorm")
    return out.view(x.shape) if out.shape != x.shape and out.numel() == x.numel() else out


def layernorm_zero(x, weight, bias, shift, scale, sel=None, eps=1e-5, out=None):
    """y = T(T(T(LN(x)*w+b) * T(1+scale[sel])) + shift[sel]) -- CogVideoXLayerNormZero / AdaLayerNorm in T."""
    x2, rows, dim, ldx = _rows2d(x)
    out = torch.empty_like(x2) if out is None else out
    o2, _, _, ldy = _rows2d(out)
    for t in (weight, bias, shift, scale):
        assert t is None or t.dtype == torch.float32
    ms = shift.stride(0) if shift.dim() == 2 else 0
    _lib.check(_lib.lib().fino_layernorm_zero(_p(x2), _p(o2), rows, dim, ldx, ldy, _p(weight), _p(bias), _p(shift),
                                             _p(scale), ms, _p(sel), eps, _dt(x), _stream()), "fino_layernorm_zero")
    return out.view(x.shape) if out.shape != x.shape and out.numel() == x.numel() else out


def gated_residual(x, y, gate=None, sel=None, out=None, staged=False):
    """out = T(float(x) + float(y)*gate[sel]) (gate None => T(x+y)); staged: T(x + T(y*gate))."""
    x2, rows, dim, ldx = _rows2d(x)
    y2, _, _, ldy = _rows2d(y)
    out = torch.empty_like(x2) if out is None else out
    o2, _, _, ldo = _rows2d(out)
    ms = gate.stride(0) if (gate is not None and gate.dim() == 2) else 0
    fn = _lib.lib().fino_gated_residual_staged if staged else _lib.lib().fino_gated_residual
    _lib.check(fn(_p(x2), _p(y2), _p(o2), rows, dim, ldx, ldy, ldo, _p(gate), ms, _p(sel), _dt(x), _stream()),
               "fino_gated_residual")
    return out.view(x.shape) if out.shape != x.shape and out.numel() == x.numel() else out


SCALE_FOLDED = -1.0     # FINO_ATTN_SCALE_FOLDED: q already carries softmax_scale * log2(e) (rmsnorm_rope_(out_scale=...))
LOG2E = 1.4426950408889634


def rmsnorm_rope_(x, weight, eps, cos=None, sin=None, head_dim=0, out_scale=1.0):
    """In place on the row-strided view x [rows, D] (e.g. the q or k column block of a fused QKV buffer).
    out_scale: multiplies the fp32 result before its one rounding (q for attention(scale=SCALE_FOLDED))."""
    x2, rows, dim, ldx = _rows2d(x)
    if cos is not None:
        assert cos.dtype == torch.float32 and cos.is_contiguous() and cos.shape == (rows, head_dim // 2)
        assert sin.dtype == torch.float32 and sin.is_contiguous() and sin.shape == cos.shape
    _lib.check(_lib.lib().fino_rmsnorm_rope_scaled(_p(x2), rows, dim, ldx, _p(weight), eps, _p(cos), _p(sin), head_dim,
                                                  float(out_scale), _dt(x), _stream()), "fino_rmsnorm_rope")
    return x


def qkv_rmsnorm_rope_(qkv, dim, q_weight, q_eps, k_weight, k_eps, cos, sin, head_dim, q_out_scale=1.0, out=None,
                      head_off=None, head_ld=None):
    """q (columns [0, dim)) and k ([dim, 2 dim)) of the fused projection qkv [rows, 3 dim] in ONE launch: the arithmetic of
    rmsnorm_rope_(q, ..., out_scale=q_out_scale) and rmsnorm_rope_(k, ...).  With `out` (flat buffer) + head_off [3 heads]
    + head_ld [heads] (int64 device tables) nothing changes in place and q, k and v are scattered by head (see
    rmsnorm_rope_scatter)."""
    x2, rows, width, ldx = _rows2d(qkv)
    assert width == 3 * dim
    assert cos.dtype == torch.float32 and cos.is_contiguous() and cos.shape == (rows, head_dim // 2) and sin.shape == cos.shape
    if out is not None:
        assert head_off.dtype == torch.int64 and head_off.numel() == 3 * (dim // head_dim) and head_off.is_contiguous()
        assert head_ld.dtype == torch.int64 and head_ld.numel() == dim // head_dim and out.is_contiguous()
    _lib.check(_lib.lib().fino_qkv_rmsnorm_rope(_p(x2), rows, dim, ldx, _p(q_weight), q_eps, _p(k_weight), k_eps, _p(cos),
                                                _p(sin), head_dim, float(q_out_scale), _p(out), _p(head_off), _p(head_ld),
                                                _dt(qkv), _stream()), "fino_qkv_rmsnorm_rope")
    return qkv if out is None else out


def rmsnorm_rope_scatter(x, weight, eps, cos, sin, head_dim, out, head_off, head_ld, out_scale=1.0):
    """rmsnorm_rope_ out of place: head hd of row r of x [rows, D] (row-strided view) is written to the flat buffer `out`
    at element head_off[hd] + r * head_ld[hd] (int64 device tables).  weight = cos = None: a scattering copy."""
    x2, rows, dim, ldx = _rows2d(x)
    assert head_off.dtype == torch.int64 and head_ld.dtype == torch.int64 and head_off.is_cuda and head_ld.is_cuda
    assert head_off.numel() == dim // head_dim == head_ld.numel() and out.is_contiguous() and out.dtype == x.dtype
    if cos is not None:
        assert cos.dtype == torch.float32 and cos.is_contiguous() and cos.shape == (rows, head_dim // 2)
        assert sin.dtype == torch.float32 and sin.is_contiguous() and sin.shape == cos.shape
    _lib.check(_lib.lib().fino_rmsnorm_rope_scatter(_p(x2), rows, dim, ldx, _p(weight), eps, _p(cos), _p(sin), head_dim,
                                                    float(out_scale), _p(out), _p(head_off), _p(head_ld), _dt(x),
                                                    _stream()), "fino_rmsnorm_rope_scatter")
    return out


def headnorm_rope_(x, heads, head_dim, weight, bias, eps, cos=None, sin=None, rope_row0=0, out_scale=1.0):
    """In place on x [B, rows, heads*head_dim] (row-strided): per-head LayerNorm + RoPE on rows >= rope_row0.
    out_scale: multiplies the result before it is stored (q for attention(scale=SCALE_FOLDED))."""
    assert x.dim() == 3 and x.stride(2) == 1
    b, rows, _ = x.shape
    _lib.check(_lib.lib().fino_headnorm_rope_scaled(_p(x), b, rows, heads, head_dim, x.stride(1), x.stride(0), _p(weight),
                                                   _p(bias), eps, _p(cos), _p(sin), rope_row0, float(out_scale), _dt(x),
                                                   _stream()), "fino_headnorm_rope")
    return x


SPLIT_ATTENTION_TAIL = os.environ.get("FINO_ATTN_SPLIT", "1") != "0"      # A/B knob; the split is the default
_attn_ws = {}      # device index -> fp32 workspace of the attention tail split (caller-owned per the C ABI; grown on demand)


def _attention_workspace(b, heads, lq, lk, dh, device):
    need = _lib.lib().fino_attn_workspace_bytes(b, heads, lq, lk, dh)
    if need <= 0:
        return None, 0
    key = (device.index, torch.cuda.current_stream().cuda_stream)       # concurrent streams must not share partials
    ws = _attn_ws.get(key)
    if ws is None or ws.numel() * 4 < need:
        ws = _attn_ws[key] = torch.empty(need // 4, dtype=torch.float32, device=device)
    return ws, need


def _attn_args(q, k, v, heads, out, scale, make_out=True):
    """what the attention front ends share before the launch: q [B, Lq, H*Dh], k / v [B, Lk, H*Dh] (row-strided views) checked,
    `out` (unless the front end makes its own) and `scale` defaulted -> (b, lq, lk, hd, dh, out, scale)"""
    assert q.dim() == 3 and k.dim() == 3 and v.dim() == 3
    b, lq, hd = q.shape
    lk = k.shape[1]
    dh = hd // heads
    for t in (q, k, v):
        assert t.stride(2) == 1 and t.is_cuda
    if out is None and make_out:
        out = torch.empty((b, lq, hd), dtype=q.dtype, device=q.device)
    scale = dh ** -0.5 if scale is None else scale
    return b, lq, lk, hd, dh, out, scale


def _attn_lead(q, k, v, out, b, heads, lq, lk, dh, scale):
    """fino_attn_fwd's arguments up to dtype, which its siblings repeat (head stride dh: a row holds its heads side by side)"""
    return (_p(q), _p(k), _p(v), _p(out), b, heads, lq, lk, dh, q.stride(0), q.stride(1), dh, k.stride(0), k.stride(1), dh,
            v.stride(0), v.stride(1), dh, out.stride(0), out.stride(1), dh, float(scale), _dt(q))


def _attn_fp8_lead(q, k, v, out, b, heads, lq, lk, dh, scale, p_mode, ws, need):
    """fino_attn_fwd_fp8's arguments up to kv_workspace_bytes, which its siblings repeat"""
    return (_p(q), _p(k), _p(v), _p(out), b, heads, lq, lk, dh, q.stride(0), q.stride(1), k.stride(0), k.stride(1),
            v.stride(0), v.stride(1), out.stride(0), out.stride(1), float(scale), _dt(q), int(p_mode), _p(ws), need)


def _check_ranges(ranges, lq):
    nqb = (lq + 255) // 256
    assert ranges.dtype == torch.int32 and ranges.is_cuda and ranges.is_contiguous() and tuple(ranges.shape) == (nqb, 3, 2), \
        f"ranges: an int32 device tensor [{nqb}, 3, 2] is needed, got {ranges.dtype} {tuple(ranges.shape)} on {ranges.device}"


def _timed_attn(b, lq, lk, hd, ranges=None, nbytes=False):
    """an attention launch under KernelTimer: "attn_self" / "attn_cross" by the rule of the kernel symbols (VAR 0 / 1; a range
    walk is always "attn_self"), 4.Lq.Lk.(H.Dh) FLOPs per batch element -- a range walk: from the tiles walked, the table's host
    copy read only here, under the timer (one sync per launch) -- and, `nbytes`, the algorithmic bytes: Q read + O written (Lq
    rows), K and V read (Lk rows), 2 bytes per element.  Returns a closure to call after the launch, or None."""
    name = "attn_self" if ranges is not None or lk > 1024 else "attn_cross"
    ev = _timed(name)
    if ev is None:
        return None

    def done():
        ev.record()
        kt_ = KernelTimer.active
        pairs = lq * lk if ranges is None else _ranges_pairs(ranges, lq, lk)
        kt_.flops[name] = kt_.flops.get(name, 0.0) + 4.0 * b * pairs * hd
        if nbytes:
            kt_.bytes[name] = kt_.bytes.get(name, 0.0) + 2.0 * b * hd * (2 * lq + 2 * lk)
    return done


def attention(q, k, v, heads, out=None, scale=None):
    """q [B, Lq, H*Dh] (row-strided view), k/v [B, Lk, H*Dh] -> o [B, Lq, H*Dh].  Non-causal SDPA."""
    b, lq, lk, hd, dh, out, scale = _attn_args(q, k, v, heads, out, scale)
    done = _timed_attn(b, lq, lk, hd, nbytes=True)
    ws, ws_bytes = _attention_workspace(b, heads, lq, lk, dh, q.device) if SPLIT_ATTENTION_TAIL else (None, 0)
    _lib.check(_lib.lib().fino_attn_fwd_ws(*_attn_lead(q, k, v, out, b, heads, lq, lk, dh, scale), _p(ws), ws_bytes, _stream()),
               "fino_attn_fwd_ws")
    if done is not None:
        done()
    return out


def _ranges_pairs(ranges, lq, lk):
    """(query row, key) pairs of one head that a ranges launch walks"""
    nta = (lk + 63) // 64
    pairs = 0.0
    for i, blk in enumerate(ranges.clamp(0, nta).tolist()):
        keys = sum(max(0, min(e * 64, lk) - s * 64) for s, e in blk)
        pairs += float(min(256, lq - 256 * i)) * keys
    return pairs


def attention_ranges_supported(b, heads, lq, lk, dh):
    return bool(_lib.lib().fino_attn_ranges_supported(int(b), int(heads), int(lq), int(lk), int(dh)))


def attention_ranges(q, k, v, heads, ranges, out=None, scale=None):
    """attention() over a subset of the key tiles, chosen per 256-row q-block: `ranges` is an int32 DEVICE tensor
    [ceil(Lq / 256), 3, 2] of up to three ascending, disjoint [begin, end) ranges of 64-key tiles per q-block ((0, 0): unused),
    shared by all heads and batch elements (fino_attn_fwd_ranges; frameino_amd/window_attention.py builds the tables of the
    sliding window over frames).  A q-block without tiles gets zeros."""
    b, lq, lk, hd, dh, out, scale = _attn_args(q, k, v, heads, out, scale)
    _check_ranges(ranges, lq)
    done = _timed_attn(b, lq, lk, hd, ranges, nbytes=True)
    _lib.check(_lib.lib().fino_attn_fwd_ranges(*_attn_lead(q, k, v, out, b, heads, lq, lk, dh, scale), _p(ranges), _stream()),
               "fino_attn_fwd_ranges")
    if done is not None:
        done()
    return out


def attention_tiles_supported(b, heads, lq, lk, dh):
    return bool(_lib.lib().fino_attn_tiles_supported(int(b), int(heads), int(lq), int(lk), int(dh)))


_MASK_DTYPES = tuple(d for d in (torch.int32, getattr(torch, "uint32", None)) if d is not None)


def _check_tile_mask(mask, b, heads, lq, lk):
    """a tile mask [B | 1, heads | 1, nqb, words] -> (words, batch stride, head stride) in words; size-1 dims share their rows"""
    nqb, nta = (lq + 255) // 256, (lk + 63) // 64
    ok = (isinstance(mask, torch.Tensor) and mask.dtype in _MASK_DTYPES and mask.is_cuda and mask.dim() == 4
          and mask.is_contiguous() and mask.shape[0] in (1, b) and mask.shape[1] in (1, heads) and mask.shape[2] == nqb
          and mask.shape[3] * 32 >= nta)
    if not ok:
        got = f"{mask.dtype} {tuple(mask.shape)} on {mask.device}" if isinstance(mask, torch.Tensor) else type(mask)
        raise ValueError(f"mask: a contiguous int32 / uint32 device tensor [{b} | 1, {heads} | 1, {nqb}, >= {(nta + 31) // 32}] is "
                         f"needed, got {got}")
    words = mask.shape[3]
    return words, (mask.shape[1] * nqb * words if mask.shape[0] == b and b > 1 else 0), (nqb * words if mask.shape[1] == heads and heads > 1 else 0)


def _tile_mask_bits(mask, lk):
    """host copy of a tile mask as bool [..., nqb, ceil(lk / 64)] (a host read: diagnostics only)"""
    from .window_attention import unpack_tile_mask          # (the one unpacking of the layout; that module is pure torch)
    return unpack_tile_mask(mask, lk)


def tile_mask_density(mask, lk):
    """fraction of the (q-block, key tile) pairs a tile mask keeps, over all its batch elements and heads.  A HOST read of the
    mask (one sync): diagnostics only, never on the step's path."""
    return float(_tile_mask_bits(mask, lk).float().mean())


def attention_tile_plan_bytes(b, heads, lq, lk, dh):
    """bytes of the fp32 workspace attention_tile_plan needs (0: shape not supported)"""
    return int(_lib.lib().fino_attn_tile_plan_bytes(int(b), int(heads), int(lq), int(lk), int(dh)))


_plan_ws = {}      # (device index, stream) -> fp32 workspace of attention_tile_plan (pooled q and k; grown on demand)


def attention_tile_plan_gated_bytes(b, heads, lq, lk, dh):
    """bytes of the fp32 workspace attention_tile_plan needs with `similarity_threshold`: the pooled means, then sim_q
    [b, heads, nqb] and sim_k [b, heads, ntall] (0: shape not supported)"""
    return int(_lib.lib().fino_attn_tile_plan_gated_bytes(int(b), int(heads), int(lq), int(lk), int(dh)))


def attention_tile_plan(q, k, heads, cdf, keep_ranges=None, scale=None, out=None, workspace=None, cdf_heads=None,
                        similarity_threshold=None, return_similarity=False):
    """The tile mask of attention_tiles, predicted on the device from q [B, Lq, H*Dh] and k [B, Lk, H*Dh] as the attention call
    gets them (fino_attn_tile_plan: mean-pooled q-blocks and key tiles, a softmax over the tiles, the smallest set of tiles by
    descending mass that reaches `cdf` together with the always-kept tiles of `keep_ranges`, an int32 device table
    [ceil(Lq / 256), 3, 2] in the format of attention_ranges, or None) -> int32 device tensor [B, heads, nqb, words].  `scale`
    as attention(): SCALE_FOLDED when q carries it.  `out` / `workspace` (fp32, >= fino_attn_tile_plan_bytes): caller-owned
    buffers, for a step that is captured.  No host read; deterministic.
    `cdf_heads` (fp32 device tensor [heads]): head h uses cdf_heads[h] instead of `cdf`, >= 1 keeps every tile of that head.
    `similarity_threshold` (theta in (0, 1]): q-blocks whose rows do not resemble each other (mean pairwise cosine < theta) keep
    every tile, such key tiles are always kept and take no part in the prediction (fino_attn_tile_plan_gated; the workspace is
    then >= fino_attn_tile_plan_gated_bytes).  With both None the ungated entry is called, as ever.  `return_similarity` (needs
    the threshold): -> (mask, (sim_q [B, heads, nqb], sim_k [B, heads, ntall])), copies of the workspace's tail."""
    assert q.dim() == 3 and k.dim() == 3 and q.shape[0] == k.shape[0] and q.shape[2] == k.shape[2]
    for t in (q, k):
        assert t.stride(2) == 1 and t.is_cuda
    b, lq, hd = q.shape
    lk = k.shape[1]
    dh = hd // heads
    nqb, words = (lq + 255) // 256, ((lk + 63) // 64 + 31) // 32
    if keep_ranges is not None:
        _check_ranges(keep_ranges, lq)
    if cdf_heads is not None:
        assert isinstance(cdf_heads, torch.Tensor) and cdf_heads.dtype == torch.float32 and cdf_heads.is_cuda and \
            cdf_heads.is_contiguous() and tuple(cdf_heads.shape) == (heads,), \
            f"cdf_heads: a contiguous fp32 device tensor [{heads}] is needed, got {getattr(cdf_heads, 'dtype', type(cdf_heads))} " \
            f"{tuple(getattr(cdf_heads, 'shape', ()))}"
    gate = similarity_threshold is not None
    if gate:
        theta = float(similarity_threshold)
        assert 0.0 < theta <= 1.0, f"similarity_threshold = {similarity_threshold!r}: a number in (0, 1] is needed"
    assert gate or not return_similarity, "return_similarity needs similarity_threshold: the similarities are computed under the gate only"
    if out is None:
        out = torch.empty((b, heads, nqb, words), dtype=torch.int32, device=q.device)
    assert out.dtype in _MASK_DTYPES and out.is_cuda and out.is_contiguous() and \
        tuple(out.shape[:3]) == (b, heads, nqb) and out.dim() == 4 and out.shape[3] * 32 >= (lk + 63) // 64, \
        f"out: a contiguous int32 device tensor [{b}, {heads}, {nqb}, >= {words}] is needed, got {out.dtype} {tuple(out.shape)}"
    plain = _lib.lib().fino_attn_tile_plan_bytes(b, heads, lq, lk, dh)
    need = _lib.lib().fino_attn_tile_plan_gated_bytes(b, heads, lq, lk, dh) if gate else plain
    if need <= 0:
        raise NotImplementedError(f"attention_tile_plan: B={b} H={heads} Lq={lq} Lk={lk} head_dim={dh} is not supported "
                                  f"(head_dim 64 | 128, at most 65536 keys)")
    if workspace is None:
        key = (q.device.index, torch.cuda.current_stream().cuda_stream)
        workspace = _plan_ws.get(key)
        if workspace is None or workspace.numel() * 4 < need:
            workspace = _plan_ws[key] = torch.empty(need // 4, dtype=torch.float32, device=q.device)
    assert workspace.dtype == torch.float32 and workspace.is_cuda and workspace.is_contiguous() and workspace.numel() * 4 >= need
    scale = dh ** -0.5 if scale is None else scale
    ev = _timed("attn_tile_plan")
    if cdf_heads is None and not gate:
        _lib.check(_lib.lib().fino_attn_tile_plan(_p(q), _p(k), b, heads, lq, lk, dh, q.stride(0), q.stride(1), dh,
                                                 k.stride(0), k.stride(1), dh, float(scale), _dt(q), float(cdf),
                                                 _p(keep_ranges), _p(out), out.shape[3], _p(workspace), workspace.numel() * 4,
                                                 _stream()), "fino_attn_tile_plan")
    else:
        _lib.check(_lib.lib().fino_attn_tile_plan_gated(_p(q), _p(k), b, heads, lq, lk, dh, q.stride(0), q.stride(1), dh,
                                                       k.stride(0), k.stride(1), dh, float(scale), _dt(q), float(cdf),
                                                       _p(cdf_heads), theta if gate else 0.0, _p(keep_ranges), _p(out),
                                                       out.shape[3], _p(workspace), workspace.numel() * 4, _stream()),
                   "fino_attn_tile_plan_gated")
    if ev is not None:
        ev.record()
    if return_similarity:
        nt = (lk + 63) // 64
        tail = workspace[plain // 4:plain // 4 + b * heads * (nqb + nt)]
        return out, (tail[:b * heads * nqb].view(b, heads, nqb).clone(), tail[b * heads * nqb:].view(b, heads, nt).clone())
    return out


def _timed_tiles_done(ev, mask, b, heads, lq, lk, hd, dh):
    """close the "attn_self" timing of a tile walk: FLOPs from the tiles walked -- the mask's host copy is read only here, under
    the timer (one sync per launch)"""
    ev.record()
    kt_ = KernelTimer.active
    bits = _tile_mask_bits(mask, lk).expand(b, heads, -1, -1).to(torch.float64)
    keys = torch.full((bits.shape[-1],), 64.0, dtype=torch.float64)
    keys[-1] = lk - 64 * (bits.shape[-1] - 1)
    rows = torch.tensor([min(256, lq - 256 * i) for i in range(bits.shape[2])], dtype=torch.float64)
    pairs = float(((bits * keys).sum(-1) * rows).sum())
    kt_.flops["attn_self"] = kt_.flops.get("attn_self", 0.0) + 4.0 * pairs * dh
    kt_.bytes["attn_self"] = kt_.bytes.get("attn_self", 0.0) + 2.0 * b * hd * (2 * lq + 2 * lk)


def attention_tiles(q, k, v, heads, mask, out=None, scale=None):
    """attention() over a subset of the key tiles, chosen per (batch element, head, 256-row q-block): `mask` is an int32 / uint32
    DEVICE tensor [B | 1, heads | 1, ceil(Lq / 256), words], bit t & 31 of word t >> 5 of a row stands for the 64-key tile t; a
    size-1 dimension shares its rows (fino_attn_fwd_tiles; attention_tile_plan predicts such a mask).  Bits at or beyond
    ceil(Lk / 64) are ignored; an empty row gives zeros."""
    b, lq, lk, hd, dh, out, scale = _attn_args(q, k, v, heads, out, scale)
    words, mask_bs, mask_hs = _check_tile_mask(mask, b, heads, lq, lk)
    ev = _timed("attn_self")
    _lib.check(_lib.lib().fino_attn_fwd_tiles(*_attn_lead(q, k, v, out, b, heads, lq, lk, dh, scale), _p(mask), mask_bs, mask_hs,
                                             words, _stream()), "fino_attn_fwd_tiles")
    if ev is not None:
        _timed_tiles_done(ev, mask, b, heads, lq, lk, hd, dh)
    return out


def attention_tail_supported(b, heads, lq, lk, dh):
    return bool(_lib.lib().fino_attn_tail_supported(int(b), int(heads), int(lq), int(lk), int(dh)))


def attention_tail(q, k, v, heads, lk_b, tail_mult, out=None, scale=None):
    """attention() over key sequences whose tail is ONE row repeated (a zero-padded prompt): batch element i attends to its first
    lk_b[i] rows of k / v [B, Lk, H*Dh]; the last of them stands for tail_mult[i] identical keys (its logit gets + ln mult), rows
    from lk_b[i] on are ignored.  Equals attention() on the expanded sequences up to the rounding of one weight
    (fino_attn_fwd_tail: the walking kernel; head_dim 128, B <= 4, Lk > 64 -- attention_tail_supported)."""
    import ctypes
    b, lq, lk, hd, dh, out, scale = _attn_args(q, k, v, heads, out, scale)
    assert len(lk_b) == b and len(tail_mult) == b
    lk_arr = (ctypes.c_int * b)(*[int(x) for x in lk_b])
    mult_arr = (ctypes.c_float * b)(*[float(x) for x in tail_mult])
    ev = _timed("attn_cross")
    _lib.check(_lib.lib().fino_attn_fwd_tail(*_attn_lead(q, k, v, out, b, heads, lq, lk, dh, scale),
                                            ctypes.cast(lk_arr, ctypes.c_void_p), ctypes.cast(mult_arr, ctypes.c_void_p), _stream()),
               "fino_attn_fwd_tail")
    if ev is not None:
        ev.record()
        kt_ = KernelTimer.active
        kt_.flops["attn_cross"] = kt_.flops.get("attn_cross", 0.0) + 4.0 * lq * hd * sum(int(x) for x in lk_b)
    return out


def attention_probs_supported(b, heads, lq, lk, dh):
    return bool(_lib.lib().fino_attn_probs_supported(int(b), int(heads), int(lq), int(lk), int(dh)))


def row_rrms(x, eps, out=None):
    """rrms[row] = 1 / sqrt(mean(x[row]^2) + eps), fp32 [rows]: the statistic of rmsnorm_rope_ alone, bit for bit (fino_row_rrms)"""
    x2, rows, dim, ldx = _rows2d(x)
    if out is None:
        out = torch.empty(rows, dtype=torch.float32, device=x.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= rows
    _lib.check(_lib.lib().fino_row_rrms(_p(x2), rows, dim, ldx, float(eps), _p(out), _dt(x), _stream()), "fino_row_rrms")
    return out


def attention_probs(q, k, heads, lk_b, tail_mult, kp, out=None, scale=None, q_rrms=None, q_weight=None):
    """P = softmax(scale q.K^T) per head over a short key sequence: q [B, Lq, H*128], k [B, Lk <= 128, H*128] (row-strided views)
    -> p [B, Lq, H*kp] (kp a multiple of 8 >= every lk_b; columns from lk_b[i] on are zeros).  lk_b / tail_mult as attention_tail.
    The A operand of the re-associated out-projection P.(V W_o^T) (fino_attn_probs).  q_rrms [B, Lq] fp32 + q_weight [H*128]: q is
    the RAW projection, RMS-normalised while it is loaded (rmsnorm_rope_'s arithmetic and rounding points, without its pass)."""
    import ctypes
    assert q.dim() == 3 and k.dim() == 3
    b, lq, hd = q.shape
    lk = k.shape[1]
    dh = hd // heads
    for t in (q, k):
        assert t.stride(2) == 1 and t.is_cuda
    if out is None:
        out = torch.empty((b, lq, heads * kp), dtype=q.dtype, device=q.device)
    assert out.shape == (b, lq, heads * kp) and out.stride(2) == 1
    scale = dh ** -0.5 if scale is None else scale
    lk_arr = (ctypes.c_int * b)(*[int(x) for x in lk_b])
    mult_arr = (ctypes.c_float * b)(*[float(x) for x in tail_mult])
    ev = _timed("attn_cross")
    _lib.check(_lib.lib().fino_attn_probs(_p(q), _p(k), _p(out), b, heads, lq, lk, dh, q.stride(0), q.stride(1), dh,
                                         k.stride(0), k.stride(1), dh, int(kp), out.stride(0), out.stride(1), float(scale),
                                         _dt(q), ctypes.cast(lk_arr, ctypes.c_void_p), ctypes.cast(mult_arr, ctypes.c_void_p),
                                         _p(q_rrms), q_rrms.stride(0) if q_rrms is not None else 0, _p(q_weight), _stream()),
               "fino_attn_probs")
    if ev is not None:
        ev.record()
        kt_ = KernelTimer.active
        kt_.flops["attn_cross"] = kt_.flops.get("attn_cross", 0.0) + 2.0 * lq * hd * sum(int(x) for x in lk_b)
    return out


_attn_fp8_ws = {}     # (device index, stream) -> byte workspace of the quantised K / V images of attention_fp8


# how a softmax weight becomes its e4m3 operand byte (include/frameino_hip.h: FINO_FP8_P_*): exp2 + rounding on the
# transcendental / conversion units, or the byte written directly as rne(8 (s - m) + 55.5) -- exp2 with a piecewise-linear
# mantissa, a third of the vector-instruction time of a kernel that is bound by exactly those instructions
FP8_P_EXP2, FP8_P_RAMP = 0, 1
FP8_P_MODES = {"exp2": FP8_P_EXP2, "ramp": FP8_P_RAMP}
_p_env = os.environ.get("FINO_FP8_P_MODE", "ramp")
if _p_env not in FP8_P_MODES:
    raise ValueError(f"FINO_FP8_P_MODE={_p_env!r}: expected one of {' | '.join(FP8_P_MODES)} (how the opt-in fp8 attention turns a "
                     f"softmax weight into its e4m3 byte; 'ramp' -- a piecewise-linear exp2, the default since round 4 -- adds "
                     f"~0.3e-2 to the 5.5e-2 rel-RMS of the fp8 operands, 'exp2' is the exact form)")
FP8_P_DEFAULT = FP8_P_MODES[_p_env]


def _attn_fp8_workspace(need, device):
    """the byte workspace of the quantised K / V images, one per (device, stream), grown on demand"""
    key = (device.index, torch.cuda.current_stream().cuda_stream)
    ws = _attn_fp8_ws.get(key)
    if ws is None or ws.numel() < need:
        ws = _attn_fp8_ws[key] = torch.empty(need, dtype=torch.uint8, device=device)
    return ws


def _fp8_smooth_flags(smooth_k, smooth_v):
    # include/frameino_hip.h: FINO_FP8_SMOOTH_K = 1, FINO_FP8_SMOOTH_V = 2
    return (1 if smooth_k else 0) | (2 if smooth_v else 0)


def _attn_fp8_prepare(p_mode, smooth_k, smooth_v, b, heads, lk, dh, device):
    """what the fp8 front ends share before the launch -> (p_mode as its FP8_P_* integer, the smooth flag word, bytes of the
    quantised K / V images for these flags -- <= 0: no kernel for this head_dim --, their workspace)"""
    p_mode = FP8_P_DEFAULT if p_mode is None else FP8_P_MODES.get(p_mode, p_mode)
    flags = _fp8_smooth_flags(smooth_k, smooth_v)
    need = _lib.lib().fino_attn_fp8_smoothed_kv_bytes(b, heads, lk, dh, flags)      # flags 0 / 1: the plain / smooth-K sizes
    return p_mode, flags, need, _attn_fp8_workspace(max(need, 0), device)


def attention_fp8(q, k, v, heads, out=None, scale=None, p_mode=None, smooth_k=False, smooth_v=False, smooth_q=False):
    """attention() with fp8 (e4m3) matrix operands, head_dim 64 or 128: K / V quantised per call (block-scaled, V transposed), Q
    and P in registers, both products on the block-scaled fp8 MFMA, softmax and accumulation in fp32 (fino_attn_fwd_fp8).
    p_mode: "exp2" | "ramp" (or the FP8_P_* integers); None = FP8_P_DEFAULT.
    smooth_k: subtract the mean of K over the keys (per batch element, head and channel) before K is quantised
    (fino_attn_fwd_fp8_smooth): the softmax cannot see it, and a channel offset all keys share stops costing mantissa bits.
    smooth_v: subtract the mean of V over the keys before V is quantised and add it back to the normalised output in fp32
    (fino_attn_fwd_fp8_smoothed): exact, because the softmax weights sum to one; V has one scale per (channel, 32 keys), so an
    offset all keys of a channel share (a to_v bias, a DC component) stops costing mantissa bits.
    smooth_q: subtract from every block of 256 consecutive query rows its mean (per batch element, head and channel) before q is
    quantised, and add what the mean contributed to the logits -- qbar . k_key, one fp32 per (q-block, key), from the unquantised
    keys -- back on the matrix pipe (fino_attn_fwd_fp8_smooth_q): exact, and an offset neighbouring query rows share (norm_q
    weights, low-frequency RoPE channels) stops costing mantissa bits.  Three more small launches and a table of
    B * heads * ceil(Lq / 256) * Lk words per call; the dense call only.  With smooth_q=False the call is what it was."""
    b, lq, lk, hd, dh, out, scale = _attn_args(q, k, v, heads, out, scale)
    if smooth_q:
        return _attention_fp8_smooth_q(q, k, v, out, b, heads, lq, lk, hd, dh, scale, p_mode, smooth_k, smooth_v)
    p_mode, flags, need, ws = _attn_fp8_prepare(p_mode, smooth_k, smooth_v, b, heads, lk, dh, q.device)
    if need <= 0:
        raise RuntimeError(f"attention_fp8: head_dim {dh} is not supported (64 or 128)")
    fwd = "fino_attn_fwd_fp8_smoothed" if smooth_v else ("fino_attn_fwd_fp8_smooth" if smooth_k else "fino_attn_fwd_fp8")
    done = _timed_attn(b, lq, lk, hd)
    _lib.check(getattr(_lib.lib(), fwd)(*_attn_fp8_lead(q, k, v, out, b, heads, lq, lk, dh, scale, p_mode, ws, need), _stream(),
                                        *((flags,) if smooth_v else ())), fwd)
    if done is not None:
        done()
    return out


def _attention_fp8_smooth_q(q, k, v, out, b, heads, lq, lk, hd, dh, scale, p_mode, smooth_k, smooth_v):
    """attention_fp8(smooth_q=True): the flag word with FINO_FP8_SMOOTH_Q = 4 and the workspace that holds the means and the table"""
    p_mode = FP8_P_DEFAULT if p_mode is None else FP8_P_MODES.get(p_mode, p_mode)
    flags = _fp8_smooth_flags(smooth_k, smooth_v) | 4
    need = _lib.lib().fino_attn_fp8_smooth_q_kv_bytes(b, heads, lq, lk, dh, flags)
    if need <= 0:
        raise RuntimeError(f"attention_fp8: head_dim {dh} is not supported (64 or 128)")
    ws = _attn_fp8_workspace(need, q.device)
    done = _timed_attn(b, lq, lk, hd)
    _lib.check(_lib.lib().fino_attn_fwd_fp8_smooth_q(*_attn_fp8_lead(q, k, v, out, b, heads, lq, lk, dh, scale, p_mode, ws, need),
                                                    _stream(), flags), "fino_attn_fwd_fp8_smooth_q")
    if done is not None:
        done()
    return out


def attention_fp8_ranges_supported(b, heads, lq, lk, dh):
    return bool(_lib.lib().fino_attn_fp8_ranges_supported(int(b), int(heads), int(lq), int(lk), int(dh)))


def attention_fp8_ranges(q, k, v, heads, ranges, out=None, scale=None, p_mode=None, smooth_k=False, smooth_v=False):
    """attention_fp8() over the subset of key tiles attention_ranges() walks: the same int32 DEVICE table [ceil(Lq / 256), 3, 2]
    per 256 query rows (fino_attn_fwd_fp8_ranges; head_dim 64 only).  K / V are quantised whole, and `smooth_k` subtracts the mean
    over ALL keys: the softmax over any subset of them cannot see it either.  `smooth_v` likewise subtracts (and adds back) the
    mean of V over ALL keys: the weights of any subset still sum to one.  A q-block without tiles gets zeros, not that mean."""
    b, lq, lk, hd, dh, out, scale = _attn_args(q, k, v, heads, out, scale)
    _check_ranges(ranges, lq)
    if dh != 64:
        raise RuntimeError(f"attention_fp8_ranges: head_dim {dh} is not supported (64 only)")
    p_mode, flags, need, ws = _attn_fp8_prepare(p_mode, smooth_k, smooth_v, b, heads, lk, dh, q.device)
    done = _timed_attn(b, lq, lk, hd, ranges)
    _lib.check(_lib.lib().fino_attn_fwd_fp8_ranges(*_attn_fp8_lead(q, k, v, out, b, heads, lq, lk, dh, scale, p_mode, ws, need),
                                                  flags, _p(ranges), _stream()), "fino_attn_fwd_fp8_ranges")
    if done is not None:
        done()
    return out


def attention_fp8_tiles_supported(b, heads, lq, lk, dh):
    return bool(_lib.lib().fino_attn_fp8_tiles_supported(int(b), int(heads), int(lq), int(lk), int(dh)))


def attention_fp8_tiles(q, k, v, heads, mask, out=None, scale=None, p_mode=None, smooth_k=False, smooth_v=False):
    """attention_fp8() over the subset of key tiles attention_tiles() walks: the same int32 / uint32 DEVICE mask [B | 1, heads | 1,
    ceil(Lq / 256), words] (fino_attn_fwd_fp8_tiles; head_dim 128 only, at most 1024 key tiles).  K / V are quantised whole, and
    `smooth_k` / `smooth_v` take their means over ALL keys: exact for any subset (every logit of a query moves by the same amount;
    the weights of the walked tiles sum to one).  Bits at or beyond ceil(Lk / 64) are ignored; an empty row gives zeros, not the
    value mean."""
    b, lq, lk, hd, dh, out, scale = _attn_args(q, k, v, heads, out, scale)
    words, mask_bs, mask_hs = _check_tile_mask(mask, b, heads, lq, lk)
    if dh != 128:
        raise RuntimeError(f"attention_fp8_tiles: head_dim {dh} is not supported (the fp8 tile walk exists for head_dim 128 only)")
    p_mode, flags, need, ws = _attn_fp8_prepare(p_mode, smooth_k, smooth_v, b, heads, lk, dh, q.device)
    ev = _timed("attn_self")
    _lib.check(_lib.lib().fino_attn_fwd_fp8_tiles(*_attn_fp8_lead(q, k, v, out, b, heads, lq, lk, dh, scale, p_mode, ws, need),
                                                 flags, _p(mask), mask_bs, mask_hs, words, _stream()), "fino_attn_fwd_fp8_tiles")
    if ev is not None:
        _timed_tiles_done(ev, mask, b, heads, lq, lk, hd, dh)
    return out


def attention_partial_floats(batch, heads, lq, head_dim):
    return _lib.lib().fino_attn_partial_bytes(batch, heads, lq, head_dim) // 4


def attention_partial(q, k, v, heads, out=None, scale=None):
    """Attention of q [B, Lq, H*Dh] over ONE key range k/v [B, Lk, H*Dh]: -> fp32 partial buffer (unnormalised O, m, l per
    (head, q-block)) for `attention_merge`."""
    b, lq, lk, hd, dh, out, scale = _attn_args(q, k, v, heads, out, scale, make_out=False)
    need = _lib.lib().fino_attn_partial_bytes(b, heads, lq, dh)
    if out is None or out.numel() * 4 < need:
        out = torch.empty(need // 4, dtype=torch.float32, device=q.device)
    _lib.check(_lib.lib().fino_attn_partial(_p(q), _p(k), _p(v), b, heads, lq, lk, dh, q.stride(0), q.stride(1), dh,
                                           k.stride(0), k.stride(1), dh, v.stride(0), v.stride(1), dh, float(scale),
                                           _dt(q), _p(out), need, _stream()), "fino_attn_partial")
    return out


def attention_merge(parts, batch, lq, heads, head_dim, dtype, out=None):
    """1..3 partials of `attention_partial` (same queries, disjoint key ranges) -> o [B, Lq, H*Dh]."""
    assert 1 <= len(parts) <= 3
    if out is None:
        out = torch.empty((batch, lq, heads * head_dim), dtype=dtype, device=parts[0].device)
    ps = list(parts) + [None] * (3 - len(parts))
    _lib.check(_lib.lib().fino_attn_merge(_p(out), batch, heads, lq, head_dim, out.stride(0), out.stride(1), head_dim,
                                         _p(ps[0]), _p(ps[1]), _p(ps[2]), _dt(out), _stream()), "fino_attn_merge")
    return out


def gemm_plan(m, n):
    """(rows run as 256-row tiles, tile height of the remaining rows or 0) -- fino_gemm's tiling on this device"""
    import ctypes
    r, t = ctypes.c_int64(), ctypes.c_int()
    _lib.check(_lib.lib().fino_gemm_plan(m, n, ctypes.byref(r), ctypes.byref(t)), "fino_gemm_plan")
    return r.value, t.value


def gemm(a, w, bias=None, epilogue=EPI_NONE, residual=None, gate=None, sel=None, out=None, out2=None, split=0, tile_m=0,
         keep=None):
    """C = epilogue(A.W^T + bias).  a [M, K] row-strided, w [N, K] (nn.Linear weight).
    `out2`, `split`: columns [split, N) of the product go to out2 [M, N - split], columns [0, split) to out [M, split]
    (fino_gemm_split_n: the fused q | k | v projection of a token shard, k | v landing in the all-gather's send buffer).
    `tile_m`: this call's tile height (0 = planned, 8 = 256-row tiles only, 2 .. 7 = 32 x tile_m rows); results do not
    depend on it.
    `keep` [M, N] row-strided (residual epilogues only; fino_gemm_keep): also receives y = T(A.W^T + bias), the value before
    the gate multiply and the residual add -- what EPI_NONE would return; `out` is what the call without it returns."""
    a2, m, k, lda = _rows2d(a)
    assert w.dim() == 2 and w.stride(1) == 1 and w.shape[1] == k and w.dtype == a.dtype
    n = w.shape[0]
    if out is None:
        out = torch.empty((m, split or n), dtype=a.dtype, device=a.device)
    o2, _, _, ldc = _rows2d(out)
    if out2 is not None:
        if keep is not None:
            raise ValueError("gemm: keep= goes with a residual epilogue, out2= / split= with none: they do not combine")
        assert 0 < split < n and residual is None
        c2, _, _, ldc2 = _rows2d(out2)
        done = _timed_gemm(None, 2.0 * m * n * k)
        _lib.check(_lib.lib().fino_gemm_split_n(_p(a2), _p(w), _p(bias), _p(o2), m, n, k, lda, w.stride(0), ldc, epilogue,
                                               0, 0, 0, 0, 0, _dt(a), _p(c2), ldc2, split, tile_m, _stream()),
                   "fino_gemm_split_n")
        if done is not None:
            done()
        return out, out2
    r2, ldr, ms = _epi_operands(residual, gate)
    if bias is not None:
        assert bias.dtype == a.dtype and bias.is_contiguous()
    # algorithmic bytes: A [M, K] and W [N, K] read, C [M, N] written (+ the residual read), 2 bytes per element
    done = _timed_gemm(epilogue, 2.0 * m * n * k, 2.0 * (m * k + n * k + m * n * (2 if residual is not None else 1)))
    if keep is not None:
        k2, km, kn, ldk = _rows2d(keep)
        assert (km, kn) == (m, n) and keep.dtype == a.dtype and keep.is_cuda
        _lib.check(_lib.lib().fino_gemm_keep(_p(a2), _p(w), _p(bias), _p(o2), m, n, k, lda, w.stride(0), ldc, epilogue,
                                            _p(r2), ldr, _p(gate), ms, _p(sel), _dt(a), _p(k2), ldk, tile_m, _stream()),
                   "fino_gemm_keep")
    elif tile_m:
        _lib.check(_lib.lib().fino_gemm_split_n(_p(a2), _p(w), _p(bias), _p(o2), m, n, k, lda, w.stride(0), ldc, epilogue,
                                               _p(r2), ldr, _p(gate), ms, _p(sel), _dt(a), None, 0, 0, tile_m, _stream()),
                   "fino_gemm_split_n")
    else:
        _lib.check(_lib.lib().fino_gemm(_p(a2), _p(w), _p(bias), _p(o2), m, n, k, lda, w.stride(0), ldc, epilogue, _p(r2),
                                       ldr, _p(gate), ms, _p(sel), _dt(a), _stream()), "fino_gemm")
    if done is not None:
        done()
    return out


def gemm_blocked_a(a_blocks, rows, w, bias, residual, gate, sel, out, tile_m=0):
    """out = residual + gate[sel] * (A.W^T + bias) with A given as K blocks: a_blocks [nblk, rows_pad, blk_k], or
    [groups, peers, rows_pad, blk_k] with K block j * groups + g at a_blocks[g, j] (last dims row-strided):
    A[i, b * blk_k + c] = block b [i, c] for i < rows.  fino_gemm_blocked_a: the out-projection reading the heads exchange's
    return buffers as they arrived."""
    if a_blocks.dim() == 3:
        a_blocks = a_blocks[None]
    assert a_blocks.dim() == 4 and a_blocks.stride(3) == 1 and w.dtype == a_blocks.dtype and w.stride(1) == 1
    groups, peers, _, bk = a_blocks.shape
    n, k = w.shape
    assert k == groups * peers * bk and residual.shape == (rows, n) and out.shape == (rows, n)
    r2, _, _, ldr = _rows2d(residual)
    o2, _, _, ldc = _rows2d(out)
    ms = gate.stride(0) if gate.dim() == 2 else 0
    done = _timed_gemm(None, 2.0 * rows * n * k)
    _lib.check(_lib.lib().fino_gemm_blocked_a(_p(a_blocks), _p(w), _p(bias), _p(o2), rows, n, k, bk, a_blocks.stride(1),
                                              groups, a_blocks.stride(0), a_blocks.stride(2), w.stride(0), ldc, _p(r2),
                                              ldr, _p(gate), ms, _p(sel), _dt(a_blocks), tile_m, _stream()),
               "fino_gemm_blocked_a")
    if done is not None:
        done()
    return out


def quantize_mxfp8(x, out=None):
    """x [rows, cols] bf16|fp16 (cols % 128 == 0) -> (q uint8 [rows, cols], scales uint8 [...]) in the layout
    fino_gemm_mxfp8 consumes (OCP e4m3 elements, one e8m0 scale per 32 K-elements)."""
    x2, rows, cols, ldx = _rows2d(x)
    nbytes = _lib.lib().fino_mxfp8_scale_bytes(rows, cols)
    if nbytes <= 0:
        raise ValueError(f"quantize_mxfp8: cols={cols} must be a positive multiple of 128")
    q, s = _mx_pair((rows, cols), nbytes, x.device, out)
    _lib.check(_lib.lib().fino_quantize_mxfp8(_p(x2), _p(q), _p(s), rows, cols, ldx, _dt(x), _stream()),
               "fino_quantize_mxfp8")
    return q, s


def ln_mxfp8(mode, x, weight=None, bias=None, shift=None, scale=None, sel=None, eps=1e-6, out=None):
    """adaln_modulate (mode 0) / layernorm (1) / layernorm_zero (2) with the result as MXFP8 activations: -> (q, scales) as
    quantize_mxfp8 would make them from the T-rounded output, in one pass (fino_ln_mxfp8)."""
    x2, rows, dim, ldx = _rows2d(x)
    nbytes = _lib.lib().fino_mxfp8_scale_bytes(rows, dim)
    if nbytes <= 0:
        raise ValueError(f"ln_mxfp8: dim={dim} must be a positive multiple of 128")
    q, s = _mx_pair((rows, dim), nbytes, x.device, out)
    for t in (weight, bias, shift, scale):
        assert t is None or t.dtype == torch.float32
    ms = shift.stride(0) if (shift is not None and shift.dim() == 2) else 0
    _lib.check(_lib.lib().fino_ln_mxfp8(mode, _p(x2), _p(q), _p(s), rows, dim, ldx, _p(weight), _p(bias), _p(shift),
                                       _p(scale), ms, _p(sel), eps, _dt(x), _stream()), "fino_ln_mxfp8")
    return q, s


def _mx_gemm(entry, aq, a_scales, wq, w_scales, bias, epilogue, residual, gate, sel, out, out_dtype, m, n, k, keep=None):
    """what gemm_mxfp8 and gemm_mxfp6 share once the operands are checked: `entry` names the library's entry point (with
    `keep`, its `_keep` form)"""
    if out is None:
        out = torch.empty((m, n), dtype=out_dtype, device=aq.device)
    o2, _, _, ldc = _rows2d(out)
    r2, ldr, ms = _epi_operands(residual, gate)
    done = _timed_gemm(None, 2.0 * m * n * k)
    if keep is not None:
        k2, km, kn, ldk = _rows2d(keep)
        assert (km, kn) == (m, n) and keep.dtype == out.dtype and keep.is_cuda
        entry += "_keep"
        _lib.check(getattr(_lib.lib(), entry)(_p(aq), _p(a_scales), _p(wq), _p(w_scales), _p(bias), _p(o2), m, n, k, ldc,
                                              epilogue, _p(r2), ldr, _p(gate), ms, _p(sel), _dt(out), _p(k2), ldk, _stream()),
                   entry)
    else:
        _lib.check(getattr(_lib.lib(), entry)(_p(aq), _p(a_scales), _p(wq), _p(w_scales), _p(bias), _p(o2), m, n, k, ldc,
                                              epilogue, _p(r2), ldr, _p(gate), ms, _p(sel), _dt(out), _stream()), entry)
    if done is not None:
        done()
    return out


def gemm_mxfp8(aq, a_scales, wq, w_scales, bias=None, epilogue=EPI_NONE, residual=None, gate=None, sel=None, out=None,
               out_dtype=torch.bfloat16, keep=None):
    """C = epilogue(dequant(aq).dequant(wq)^T + bias): aq [M, K], wq [N, K] uint8 (e4m3) + their MX scales.
    `keep` [M, N] row-strided (residual epilogues only; fino_gemm_mxfp8_keep): as in `gemm` -- also receives y = T(acc + bias),
    what EPI_NONE would return; `out` is what the call without it returns."""
    m, k = aq.shape
    n = wq.shape[0]
    assert wq.shape[1] == k and aq.dtype == torch.uint8 and wq.dtype == torch.uint8 and aq.is_contiguous() \
        and wq.is_contiguous()
    return _mx_gemm("fino_gemm_mxfp8", aq, a_scales, wq, w_scales, bias, epilogue, residual, gate, sel, out, out_dtype, m, n, k,
                    keep)


def gemm_mxfp8_q(aq, a_scales, wq, w_scales, bias, epilogue=EPI_NONE, out=None):
    """MXFP8 GEMM whose result leaves quantised: -> (q uint8 [M, N], scales) ready to be the next MXFP8 GEMM's A."""
    m, k = aq.shape
    n = wq.shape[0]
    assert bias is not None and wq.shape[1] == k
    q, s = _mx_pair((m, n), _lib.lib().fino_mxfp8_scale_bytes(m, n), aq.device, out)
    done = _timed_gemm(None, 2.0 * m * n * k)
    _lib.check(_lib.lib().fino_gemm_mxfp8_q(_p(aq), _p(a_scales), _p(wq), _p(w_scales), _p(bias), _p(q), _p(s), m, n, k,
                                           epilogue, _dt(bias), _stream()), "fino_gemm_mxfp8_q")
    if done is not None:
        done()
    return q, s


MX_ROTATE = {"act": 1, "weight": 2}        # FINO_MX_ROT_ACT, FINO_MX_ROT_WEIGHT


def quantize_mxfp6(x, out=None, rotate=None):
    """x [rows, cols] bf16|fp16 (cols % 128 == 0) -> (q uint8 [fino_mxfp6_bytes], scales uint8 [...]): OCP e2m3 elements packed
    as the 16-row x 128-column fragments fino_gemm_mxfp6 reads (include/frameino_hip.h), one e8m0 scale per 32 K-elements.
    rotate: None, or "act" | "weight" (fino_quantize_mxfp6_rot): every 32-element block is rotated by the Walsh-Hadamard
    matrix before the rule, which spreads a block's outliers; "weight" also folds the 1/32 into its scales, so gemm_mxfp6 of an
    "act" image and a "weight" image is the product of the unrotated operands, up to quantisation."""
    if rotate is not None and rotate not in MX_ROTATE:
        raise ValueError(f"quantize_mxfp6: rotate={rotate!r} must be None, 'act' or 'weight'")
    x2, rows, cols, ldx = _rows2d(x)
    nbytes = _lib.lib().fino_mxfp6_scale_bytes(rows, cols)
    if nbytes <= 0:
        raise ValueError(f"quantize_mxfp6: cols={cols} must be a positive multiple of 128")
    q, s = _mx_pair(_lib.lib().fino_mxfp6_bytes(rows, cols), nbytes, x.device, out)
    if rotate is None:
        _lib.check(_lib.lib().fino_quantize_mxfp6(_p(x2), _p(q), _p(s), rows, cols, ldx, _dt(x), _stream()),
                   "fino_quantize_mxfp6")
    else:
        _lib.check(_lib.lib().fino_quantize_mxfp6_rot(_p(x2), _p(q), _p(s), rows, cols, ldx, _dt(x), MX_ROTATE[rotate],
                                                     _stream()), "fino_quantize_mxfp6_rot")
    q.mx_shape = (rows, cols)
    return q, s


def gemm_mxfp6(aq, a_scales, wq, w_scales, bias=None, epilogue=EPI_NONE, residual=None, gate=None, sel=None, out=None,
               out_dtype=torch.bfloat16, m=None, n=None, k=None, keep=None):
    """C = epilogue(dequant(aq).dequant(wq)^T + bias): aq / wq the packed images quantize_mxfp6 made of [M, K] / [N, K].  The
    images are flat byte tensors; quantize_mxfp6 notes the matrix shape on them (`q.mx_shape`), and `m` / `n` / `k` say it for
    images that came another way (a view, a copy).  `keep`: as in `gemm_mxfp8` (fino_gemm_mxfp6_keep)."""
    assert aq.dtype == torch.uint8 and wq.dtype == torch.uint8 and aq.is_contiguous() and wq.is_contiguous()
    sa_, sw_ = getattr(aq, "mx_shape", None), getattr(wq, "mx_shape", None)
    m = m if m is not None else (sa_[0] if sa_ else None)
    n = n if n is not None else (sw_[0] if sw_ else None)
    k = k if k is not None else (sa_[1] if sa_ else (sw_[1] if sw_ else None))
    if m is None or n is None or k is None:
        raise ValueError("gemm_mxfp6: operands without mx_shape need m / n / k")
    if sw_ and sw_[1] != k:
        raise ValueError(f"gemm_mxfp6: K of A ({k}) and of W ({sw_[1]}) differ")
    lib = _lib.lib()
    if aq.numel() != lib.fino_mxfp6_bytes(m, k) or wq.numel() != lib.fino_mxfp6_bytes(n, k):
        raise ValueError(f"gemm_mxfp6: operand sizes {aq.numel()} / {wq.numel()} do not match M={m} N={n} K={k}")
    return _mx_gemm("fino_gemm_mxfp6", aq, a_scales, wq, w_scales, bias, epilogue, residual, gate, sel, out, out_dtype, m, n, k,
                    keep)


def skinny_linear(x, w, b=None, silu_input=False):
    """fp32 y = W.(silu?)(x) + b for M <= 16 rows; w fp32 or bf16/fp16."""
    assert x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous() and w.is_contiguous()
    m, k = x.shape
    n = w.shape[0]
    wd = -1 if w.dtype == torch.float32 else _dt(w)
    if b is not None:
        assert b.dtype == w.dtype
    y = torch.empty((m, n), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().fino_skinny_linear(_p(x), _p(w), _p(b), _p(y), m, n, k, wd, int(silu_input), _stream()),
               "fino_skinny_linear")
    return y


def patchify(x, patch, out=None):
    """x [C, F, H, W] -> a [L, C*pt*ph*pw]"""
    assert x.dim() == 4 and x.is_contiguous()
    c, f, h, w = x.shape
    pt, ph, pw = patch
    L = (f // pt) * (h // ph) * (w // pw)
    if out is None:
        out = torch.empty((L, c * pt * ph * pw), dtype=x.dtype, device=x.device)
    _lib.check(_lib.lib().fino_patchify(_p(x), _p(out), c, f, h, w, pt, ph, pw, out.stride(0), _dt(x), _stream()),
               "fino_patchify")
    return out


def unpatchify(y, cout, frames, height, width, patch, out=None):
    """y [L, pt*ph*pw*cout] -> [cout, F, H, W]"""
    pt, ph, pw = patch
    if out is None:
        out = torch.empty((cout, frames, height, width), dtype=y.dtype, device=y.device)
    _lib.check(_lib.lib().fino_unpatchify(_p(y), _p(out), cout, frames, height, width, pt, ph, pw, y.stride(0), _dt(y),
                                         _stream()), "fino_unpatchify")
    return out


def wan_model_input(lat, cond, id_lat, traj, dtype, out=None):
    """lat [C,Fg,H,W], cond [C,1,H,W], id_lat [C,n_id,H,W]|None, traj [C,Fg+n_id,H,W] (fp32) -> [2C,Fg+n_id,H,W]."""
    c, fg, h, w = lat.shape
    nid = 0 if id_lat is None else id_lat.shape[1]
    for t in (lat, cond, id_lat, traj):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous())
    assert traj.shape == (c, fg + nid, h, w) and cond.shape == (c, 1, h, w)
    if out is None:
        out = torch.empty((2 * c, fg + nid, h, w), dtype=dtype, device=lat.device)
    _lib.check(_lib.lib().fino_wan_model_input(_p(lat), _p(cond), _p(id_lat), _p(traj), _p(out), c, fg, nid, h, w,
                                              _dt(out), _stream()), "fino_wan_model_input")
    return out


def cfg_euler_step_(lat, cond_pred, uncond_pred, guidance, dt_dev, round_out=True):
    """In place on lat [C,Fg,H,W] fp32; preds [C,Ft,H,W] of the model dtype; dt_dev: 1-element fp32 device tensor."""
    c, fg, h, w = lat.shape
    ft = cond_pred.shape[1]
    assert lat.dtype == torch.float32 and lat.is_contiguous() and cond_pred.is_contiguous()
    assert dt_dev.dtype == torch.float32 and dt_dev.is_cuda
    _lib.check(_lib.lib().fino_cfg_euler_step(_p(cond_pred), _p(uncond_pred), _p(lat), c, fg, ft, h, w, float(guidance),
                                             _p(dt_dev), int(round_out), _dt(cond_pred), _stream()),
               "fino_cfg_euler_step")
    return lat


def cfg_unipc_step_(x, last, m0, m1, cond_pred, uncond_pred, coef_dev):
    """UniPC multistep update fused with CFG; x/last/m0/m1 fp32 [C,Fg,H,W] in place, coef_dev fp32[10] (device)."""
    c, fg, h, w = x.shape
    ft = cond_pred.shape[1]
    for t in (x, last, m0, m1):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.shape == x.shape
    assert coef_dev.dtype == torch.float32 and coef_dev.numel() >= 10 and cond_pred.is_contiguous()
    _lib.check(_lib.lib().fino_cfg_unipc_step(_p(cond_pred), _p(uncond_pred), _p(x), _p(last), _p(m0), _p(m1), c, fg,
                                             ft, h, w, _p(coef_dev), _dt(cond_pred), _stream()), "fino_cfg_unipc_step")
    return x


def cfg_vpred_step_(lat, pred, coef_dev, has_uncond=True):
    """lat [Fg, C, H, W] of T in place; pred [2|1, Ft, C, H, W] of T; coef_dev fp32[5] = {sa, sb, ca, cb, g}."""
    assert lat.is_contiguous() and pred.is_contiguous() and coef_dev.dtype == torch.float32 and lat.dtype == pred.dtype
    _lib.check(_lib.lib().fino_cfg_vpred_step(_p(pred), _p(lat), lat.numel(), pred[0].numel(), _p(coef_dev),
                                             int(has_uncond), _dt(lat), _stream()), "fino_cfg_vpred_step")
    return lat


def cfg_dpm_step_(lat, pred, x0_old, noise, coef_dev, has_uncond=True):
    """CogVideoXDPMScheduler step + CFG: lat [Fg, C, H, W] of T in place, pred [2|1, Ft, C, H, W] of T, x0_old fp32 like
    lat (in/out), noise of T like lat, coef_dev fp32[9] = {sa, sb, m1, m2, m3, m4, mn, g, use_old}."""
    assert lat.is_contiguous() and pred.is_contiguous() and noise.is_contiguous() and x0_old.is_contiguous()
    assert coef_dev.dtype == torch.float32 and coef_dev.numel() >= 9 and lat.dtype == pred.dtype == noise.dtype
    assert x0_old.dtype == torch.float32 and x0_old.numel() == lat.numel() == noise.numel()
    _lib.check(_lib.lib().fino_cfg_dpm_step(_p(pred), _p(lat), _p(x0_old), _p(noise), lat.numel(), pred[0].numel(),
                                           _p(coef_dev), int(has_uncond), _dt(lat), _stream()), "fino_cfg_dpm_step")
    return lat


# ---- guiders (frameino_amd/guiders.py): {A, B} of v = A c + B u on the device, and the guided siblings of the four steps
def guider_workspace_bytes(n):
    """bytes of the caller-owned workspace of guider_coefs over a sample of n elements"""
    return int(_lib.lib().fino_guider_workspace_bytes(int(n)))


def _guider_launch(cond, uncond, rows, row_len, row_stride, args, g_dev, zero_dev, workspace, ab):
    kind, norm_threshold, eta, rescale = args
    assert ab.dtype == torch.float32 and ab.numel() >= 2 and ab.is_contiguous() and workspace.is_contiguous()
    assert g_dev.dtype == torch.float32 and g_dev.numel() >= 1 and (zero_dev is None or zero_dev.dtype == torch.float32)
    assert g_dev.device == ab.device == workspace.device == cond.device
    _lib.check(_lib.lib().fino_guider_coefs(_p(cond), _p(uncond), rows, row_len, row_stride, int(kind), float(norm_threshold),
                                           float(eta), float(rescale), _p(g_dev), _p(zero_dev), _p(workspace),
                                           workspace.numel() * workspace.element_size(), _p(ab), _dt(cond), _stream()),
               "fino_guider_coefs")
    return ab


def guider_coefs(cond_pred, uncond_pred, gen_frames, args, g_dev, zero_dev, workspace, ab):
    """Wan layout: preds [C, Ft, H, W] of T, the first gen_frames frames of every channel are the sample (ID frames excluded).
    args = guiders.kernel_args(config); g_dev / zero_dev: one fp32 each on the device (zero_dev may be None); writes ab[0:2]."""
    c, ft, h, w = cond_pred.shape
    assert cond_pred.is_contiguous() and uncond_pred.is_contiguous() and uncond_pred.shape == cond_pred.shape
    assert cond_pred.dtype == uncond_pred.dtype and 1 <= gen_frames <= ft
    return _guider_launch(cond_pred, uncond_pred, c, gen_frames * h * w, ft * h * w, args, g_dev, zero_dev, workspace, ab)


def guider_coefs_rows(pred, n_lat, args, g_dev, zero_dev, workspace, ab):
    """CogVideoX layout: pred [2, ...] of T (uncond, cond), the first n_lat elements of each row are the sample."""
    assert pred.is_contiguous() and pred.shape[0] == 2 and 1 <= n_lat <= pred[0].numel()
    return _guider_launch(pred[1], pred[0], 1, int(n_lat), pred[0].numel(), args, g_dev, zero_dev, workspace, ab)


def guided_euler_step_(lat, cond_pred, uncond_pred, ab, dt_dev, round_out=True):
    """cfg_euler_step_ with v = T(A c + B u) from ab = {A, B} (device fp32[2])."""
    c, fg, h, w = lat.shape
    ft = cond_pred.shape[1]
    assert lat.dtype == torch.float32 and lat.is_contiguous() and cond_pred.is_contiguous() and uncond_pred.is_contiguous()
    assert cond_pred.shape == uncond_pred.shape == (c, ft, h, w) and ft >= fg
    assert dt_dev.dtype == torch.float32 and dt_dev.is_cuda and ab.dtype == torch.float32 and ab.numel() >= 2
    _lib.check(_lib.lib().fino_guided_euler_step(_p(cond_pred), _p(uncond_pred), _p(lat), c, fg, ft, h, w, _p(ab), _p(dt_dev),
                                                int(round_out), _dt(cond_pred), _stream()), "fino_guided_euler_step")
    return lat


def guided_unipc_step_(x, last, m0, m1, cond_pred, uncond_pred, coef_dev, ab):
    """cfg_unipc_step_ with v = T(A c + B u) from ab = {A, B} (device fp32[2]); coef_dev[0] (g) is not read."""
    c, fg, h, w = x.shape
    ft = cond_pred.shape[1]
    for t in (x, last, m0, m1):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.shape == x.shape
    assert coef_dev.dtype == torch.float32 and coef_dev.numel() >= 10 and cond_pred.is_contiguous()
    assert uncond_pred.is_contiguous() and cond_pred.shape == uncond_pred.shape == (c, ft, h, w) and ft >= fg
    assert ab.dtype == torch.float32 and ab.numel() >= 2
    _lib.check(_lib.lib().fino_guided_unipc_step(_p(cond_pred), _p(uncond_pred), _p(x), _p(last), _p(m0), _p(m1), c, fg, ft, h,
                                                w, _p(coef_dev), _p(ab), _dt(cond_pred), _stream()), "fino_guided_unipc_step")
    return x


def guided_vpred_step_(lat, pred, coef_dev, ab):
    """cfg_vpred_step_ with v = A c + B u (fp32) from ab = {A, B} (device fp32[2]); coef_dev[4] (g) is not read."""
    assert lat.is_contiguous() and pred.is_contiguous() and coef_dev.dtype == torch.float32 and lat.dtype == pred.dtype
    assert pred.shape[0] == 2 and pred[0].numel() >= lat.numel() and coef_dev.numel() >= 4
    assert ab.dtype == torch.float32 and ab.numel() >= 2
    _lib.check(_lib.lib().fino_guided_vpred_step(_p(pred), _p(lat), lat.numel(), pred[0].numel(), _p(coef_dev), _p(ab),
                                                _dt(lat), _stream()), "fino_guided_vpred_step")
    return lat


def guided_dpm_step_(lat, pred, x0_old, noise, coef_dev, ab):
    """cfg_dpm_step_ with v = A c + B u (fp32) from ab = {A, B} (device fp32[2]); coef_dev[7] (g) is not read."""
    assert lat.is_contiguous() and pred.is_contiguous() and noise.is_contiguous() and x0_old.is_contiguous()
    assert coef_dev.dtype == torch.float32 and coef_dev.numel() >= 9 and lat.dtype == pred.dtype == noise.dtype
    assert x0_old.dtype == torch.float32 and x0_old.numel() == lat.numel() == noise.numel()
    assert pred.shape[0] == 2 and pred[0].numel() >= lat.numel() and ab.dtype == torch.float32 and ab.numel() >= 2
    _lib.check(_lib.lib().fino_guided_dpm_step(_p(pred), _p(lat), _p(x0_old), _p(noise), lat.numel(), pred[0].numel(),
                                              _p(coef_dev), _p(ab), _dt(lat), _stream()), "fino_guided_dpm_step")
    return lat


# ------------------------------------------------------------------------------------------------ Wan VAE (channels-last)
_ZERO_PAGE = {}


def zero_page(device):
    z = _ZERO_PAGE.get(str(device))
    if z is None:
        z = _ZERO_PAGE[str(device)] = torch.zeros(256, dtype=torch.uint8, device=device)
    return z


def conv3d_cl(x, w2, bias, kernel, stride=(1, 1, 1), pad=(0, 0, 0), out_thw=None, upsample2x=False, residual=None,
              out=None):
    """x [T,H,W,Cin_pad] channels-last; w2 [Cout_pad, kt*kh*kw*Cin_pad] (tap-major); pad = FRONT pads (t,h,w)."""
    assert x.dim() == 4 and x.is_contiguous() and w2.is_contiguous()
    t, h, w, cin = x.shape
    kt, kh, kw = kernel
    cout = w2.shape[0]
    assert w2.shape[1] == kt * kh * kw * cin, (w2.shape, kernel, cin)
    if out_thw is None:
        up = 2 if upsample2x else 1
        out_thw = ((t + pad[0] - kt) // stride[0] + 1, (h * up + 2 * pad[1] - kh) // stride[1] + 1,
                   (w * up + 2 * pad[2] - kw) // stride[2] + 1)
    to, ho, wo = out_thw
    if out is None:
        out = torch.empty((to, ho, wo, cout), dtype=x.dtype, device=x.device)
    ev = _timed("conv3d")
    _lib.check(_lib.lib().fino_conv3d(_p(x), _p(w2), _p(bias), _p(out), t, h, w, cin, to, ho, wo, cout, kt, kh, kw,
                                     stride[0], stride[1], stride[2], pad[0], pad[1], pad[2], int(upsample2x),
                                     EPI_RESIDUAL if residual is not None else EPI_NONE, _p(residual),
                                     _p(zero_page(x.device)), _dt(x), _stream()), "fino_conv3d")
    if ev is not None:
        ev.record()
        kt_ = KernelTimer.active
        kt_.flops["conv3d"] = kt_.flops.get("conv3d", 0.0) + 2.0 * to * ho * wo * cout * w2.shape[1]
    return out


def rmsnorm_silu_cl(x, gamma, c_valid, silu=True, out=None):
    assert x.is_contiguous() and gamma.dtype == torch.float32
    cpad = x.shape[-1]
    rows = x.numel() // cpad
    out = torch.empty_like(x) if out is None else out
    _lib.check(_lib.lib().fino_rmsnorm_silu_cl(_p(x), _p(out), rows, c_valid, cpad, _p(gamma), int(silu), _dt(x),
                                              _stream()), "fino_rmsnorm_silu_cl")
    return out


def softmax_rows_(s, n, scale):
    assert s.dim() == 2 and s.stride(1) == 1
    _lib.check(_lib.lib().fino_softmax_rows(_p(s), s.shape[0], n, s.stride(0), float(scale), _dt3(s), _stream()),
               "fino_softmax_rows")
    return s


def dup_up3d_add(main, x, c_in, c_out, factor_t, factor_s):
    t, h, w, cin_pad = x.shape
    out = torch.empty_like(main)
    assert main.shape == (1 + (t - 1) * factor_t, h * factor_s, w * factor_s, main.shape[3])
    _lib.check(_lib.lib().fino_dup_up3d_add(_p(main), _p(x), _p(out), t, h, w, c_in, cin_pad, c_out, main.shape[3],
                                           factor_t, factor_s, _dt3(x), _stream()), "fino_dup_up3d_add")
    return out


def avg_down3d_add(main, x, c_in, c_out, factor_t, factor_s):
    t, h, w, cin_pad = x.shape
    out = torch.empty_like(main)
    _lib.check(_lib.lib().fino_avg_down3d_add(_p(main), _p(x), _p(out), t, h, w, c_in, cin_pad, c_out, main.shape[3],
                                             factor_t, factor_s, _dt3(x), _stream()), "fino_avg_down3d_add")
    return out


def vae_unpatchify_clamp(y, channels, patch):
    t, h, w, cpad = y.shape
    out = torch.empty((channels, t, h * patch, w * patch), dtype=torch.float32, device=y.device)
    _lib.check(_lib.lib().fino_vae_unpatchify_clamp(_p(y), _p(out), t, h, w, cpad, channels, patch, _dt3(y), _stream()),
               "fino_vae_unpatchify_clamp")
    return out


def vae_patchify(x, c_pad, patch, dtype):
    c, t, hp, wp = x.shape
    assert x.dtype == torch.float32 and x.is_contiguous()
    y = torch.empty((t, hp // patch, wp // patch, c_pad), dtype=dtype, device=x.device)
    _lib.check(_lib.lib().fino_vae_patchify(_p(x), _p(y), t, hp // patch, wp // patch, c_pad, c, patch, _dt3(y),
                                           _stream()), "fino_vae_patchify")
    return y


# ---- the Wan VAE computing like fp32 on the bf16 matrix pipe: split-bf16 products (include/frameino_hip.h, FINO_VERSION 103) ----
# an fp32 value = hi + mid + lo (three bf16 planes); a product keeps the terms >= 2^-16 relative
SPLIT_PRODUCTS = {2: ((0, 0), (0, 1), (1, 0)),                                    # (A plane, W plane) per product, in K order
                  3: ((0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (2, 0))}


def _pack_planes(planes):
    v = 0
    for i, q in enumerate(planes):
        v |= int(q) << (2 * i)
    return v


def split_bf16(x, layout, nplanes=3, out=None):
    """x fp32 [..., C] (C % 8 == 0) -> bf16 [..., nseg * C] of split planes:
      layout "planes": the planes side by side (the A operand of conv3d_split_cl), "A" / "W": one plane per product of
      SPLIT_PRODUCTS[nplanes] -- the operands of gemm(..., EPI_F32) -- A side / W side."""
    assert x.dtype == torch.float32 and x.stride(-1) == 1
    x2 = x if x.dim() == 2 else x.reshape(-1, x.shape[-1])
    rows, cols = x2.shape
    prod = SPLIT_PRODUCTS[nplanes]
    planes = tuple(range(nplanes)) if layout == "planes" else tuple(p[0 if layout == "A" else 1] for p in prod)
    nseg = len(planes)
    if out is None:
        out = torch.empty(tuple(x.shape[:-1]) + (nseg * cols,), dtype=torch.bfloat16, device=x.device)
    assert out.is_contiguous() and out.numel() == rows * nseg * cols
    _lib.check(_lib.lib().fino_split_bf16(_p(x2), _p(out), rows, cols, x2.stride(0), nseg * cols, nseg, _pack_planes(planes),
                                         _stream()), "fino_split_bf16")
    return out


def rmsnorm_silu_cl_f32(x, gamma, c_valid, silu=True, split=None, nplanes=3):
    """WanRMS_norm [+ SiLU] on fp32 channels-last activations, in fp32; split=None -> fp32 out, "planes" | "A" | "W" -> the split
    planes of split_bf16 in the same pass"""
    assert x.is_contiguous() and x.dtype == torch.float32 and gamma.dtype == torch.float32
    cpad = x.shape[-1]
    rows = x.numel() // cpad
    if split is None:
        planes, out = (), torch.empty_like(x)
    else:
        prod = SPLIT_PRODUCTS[nplanes]
        planes = tuple(range(nplanes)) if split == "planes" else tuple(p[0 if split == "A" else 1] for p in prod)
        out = torch.empty(tuple(x.shape[:-1]) + (len(planes) * cpad,), dtype=torch.bfloat16, device=x.device)
    _lib.check(_lib.lib().fino_rmsnorm_silu_cl_f32(_p(x), _p(out), rows, c_valid, cpad, _p(gamma), int(silu), len(planes),
                                                  _pack_planes(planes), _stream()), "fino_rmsnorm_silu_cl_f32")
    return out


def conv3d_split_cl(xp, w6, bias, kernel, nplanes, stride=(1, 1, 1), pad=(0, 0, 0), out_thw=None, upsample2x=False,
                    residual=None, out=None):
    """conv3d_cl on split operands: xp bf16 [T, H, W, nplanes * Cin_pad] (split_bf16 layout "planes"), w6 bf16 [Cout_pad,
    taps * products * Cin_pad] (W planes of the products per tap), bias fp32 [Cout_pad], residual fp32 -> fp32 [To, Ho, Wo, Cout_pad]
    (into `out` if given: contiguous fp32 of that shape)"""
    assert xp.dim() == 4 and xp.is_contiguous() and w6.is_contiguous() and xp.dtype == torch.bfloat16 and w6.dtype == torch.bfloat16
    t, h, w, cw = xp.shape
    cin = cw // nplanes
    kt, kh, kw = kernel
    cout = w6.shape[0]
    nprod = len(SPLIT_PRODUCTS[nplanes])
    assert cin * nplanes == cw and w6.shape[1] == kt * kh * kw * nprod * cin, (xp.shape, w6.shape, kernel)
    assert bias is None or bias.dtype == torch.float32
    if out_thw is None:
        up = 2 if upsample2x else 1
        out_thw = ((t + pad[0] - kt) // stride[0] + 1, (h * up + 2 * pad[1] - kh) // stride[1] + 1,
                   (w * up + 2 * pad[2] - kw) // stride[2] + 1)
    to, ho, wo = out_thw
    if out is None:
        out = torch.empty((to, ho, wo, cout), dtype=torch.float32, device=xp.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (to, ho, wo, cout)
    if residual is not None:
        assert residual.dtype == torch.float32 and residual.is_contiguous() and residual.shape == out.shape
    ev = _timed("conv3d")
    _lib.check(_lib.lib().fino_conv3d_split(_p(xp), _p(w6), _p(bias), _p(out), t, h, w, cin, nplanes, to, ho, wo, cout, kt, kh, kw,
                                           stride[0], stride[1], stride[2], pad[0], pad[1], pad[2], int(upsample2x),
                                           EPI_RESIDUAL if residual is not None else EPI_NONE, _p(residual),
                                           _p(zero_page(xp.device)), _stream()), "fino_conv3d_split")
    if ev is not None:
        ev.record()
        kt_ = KernelTimer.active
        kt_.flops["conv3d"] = kt_.flops.get("conv3d", 0.0) + 2.0 * to * ho * wo * cout * w6.shape[1]
    return out


def gemm_f32(a_split, w_split, bias=None, residual=None, out=None):
    """fp32 C = A.W^T + bias [+ R] from operands already expanded by split_bf16 ("A" / "W" layouts: one plane per product):
    a_split [M, products * K], w_split [N, products * K] bf16; bias fp32 [N], residual / out fp32 [M, N]"""
    a2, m, k, lda = _rows2d(a_split)
    assert w_split.dim() == 2 and w_split.stride(1) == 1 and w_split.shape[1] == k and a_split.dtype == w_split.dtype == torch.bfloat16
    n = w_split.shape[0]
    if out is None:
        out = torch.empty((m, n), dtype=torch.float32, device=a_split.device)
    assert out.dtype == torch.float32 and out.stride(-1) == 1
    o2 = out if out.dim() == 2 else out.view(-1, out.shape[-1])
    r2, ldr = None, 0
    if residual is not None:
        assert residual.dtype == torch.float32 and residual.stride(-1) == 1
        r2 = residual if residual.dim() == 2 else residual.view(-1, residual.shape[-1])
        ldr = r2.stride(0)
    assert bias is None or (bias.dtype == torch.float32 and bias.is_contiguous())
    _lib.check(_lib.lib().fino_gemm(_p(a2), _p(w_split), _p(bias), _p(o2), m, n, k, lda, w_split.stride(0), o2.stride(0),
                                   EPI_F32_RESIDUAL if residual is not None else EPI_F32, _p(r2), ldr, None, 0, None, BF16,
                                   _stream()), "fino_gemm")
    return out


# ------------------------------------------------------------------------------------------------ CogVideoX VAE
def vae_blend_tiles_(a, b, extent, axis):
    """diffusers' blend_v (axis 0) / blend_h (axis 1) in place on the channels-last tile b [T, Hb, Wb, Cpad] from its upper / left
    neighbour a (fino_vae_blend_tiles)"""
    assert a.dim() == 4 and b.dim() == 4 and a.is_contiguous() and b.is_contiguous() and a.dtype == b.dtype
    assert a.shape[0] == b.shape[0] and a.shape[3] == b.shape[3]
    _lib.check(_lib.lib().fino_vae_blend_tiles(_p(a), _p(b), a.shape[0], a.shape[1], a.shape[2], b.shape[1], b.shape[2],
                                              a.shape[3], int(extent), int(axis), _dt(a), _stream()), "fino_vae_blend_tiles")
    return b


_GN_WS = {}


def groupnorm_cl(x, c_valid, groups, gamma, beta, eps=1e-6, mod=None, silu=False, out=None):
    """x [T, H, W, Cpad] channels-last -> T(GroupNorm(x)) [ * scale[z] + shift[z] ] [ -> silu ].  mod = (scale, shift),
    each [Tz, hz, wz, Cpad] of x's dtype (CogVideoXSpatialNorm3D's conv_y / conv_b at latent resolution)."""
    assert x.dim() == 4 and x.is_contiguous() and gamma.dtype == torch.float32 and beta.dtype == torch.float32
    t, h, w, cp = x.shape
    out = torch.empty_like(x) if out is None else out
    need = _lib.lib().fino_groupnorm_workspace_bytes(cp)
    key = (x.device.index, torch.cuda.current_stream().cuda_stream, cp)
    ws = _GN_WS.get(key)
    if ws is None:
        ws = _GN_WS[key] = torch.empty(need // 4, dtype=torch.float32, device=x.device)
    ms = mh = None
    tz = hz = wz = 0
    if mod is not None:
        ms, mh = mod
        assert ms.shape == mh.shape and ms.shape[3] == cp and ms.is_contiguous() and mh.is_contiguous() \
            and ms.dtype == x.dtype
        tz, hz, wz = ms.shape[:3]
    _lib.check(_lib.lib().fino_groupnorm_cl(_p(x), _p(out), t, h, w, c_valid, cp, groups, _p(gamma), _p(beta), eps,
                                           _p(ms), _p(mh), tz, hz, wz, int(silu), _p(ws), need, _dt(x), _stream()),
               "fino_groupnorm_cl")
    return out


def avg_pool_time2(x):
    t, h, w, cp = x.shape
    assert x.is_contiguous() and t > 1
    out = torch.empty(((t & 1) + (t - (t & 1)) // 2, h, w, cp), dtype=x.dtype, device=x.device)
    _lib.check(_lib.lib().fino_avg_pool_time2(_p(x), _p(out), t, h, w, cp, _dt(x), _stream()), "fino_avg_pool_time2")
    return out


LORA_MAX_ADAPTERS = 8                      # FINO_LORA_MAX_ADAPTERS


def lora_merge_(w_base, adapters, out=None):
    """LoRA merge on the GPU (fino_lora_merge): out = T( float(w_base) + sum_a s_a * B_a.float() @ A_a.float() ), the rank
    products accumulated in fp32 and ONE rounding at the end.  `adapters`: (A [r, K], B [N, r], s) triples, A / B in the
    weight's dtype (bf16 / fp16 / fp32), row-strided with a contiguous last dimension.  out=None merges in place; otherwise
    `out` is a [N, K] row-strided buffer of the same dtype that does not overlap w_base.  Returns the written tensor."""
    out = w_base if out is None else out
    if not (w_base.is_cuda and out.is_cuda):
        raise RuntimeError("frameino_amd ops need CUDA(HIP) tensors; there is no CPU path")
    if w_base.dim() != 2 or out.shape != w_base.shape or out.dtype != w_base.dtype:
        raise ValueError(f"lora_merge_: weight {tuple(w_base.shape)} {w_base.dtype} / out {tuple(out.shape)} {out.dtype}")
    if w_base.stride(1) != 1 or out.stride(1) != 1:
        raise ValueError("lora_merge_: the weight's last dimension must be contiguous")
    if len(adapters) > LORA_MAX_ADAPTERS:
        raise ValueError(f"lora_merge_: {len(adapters)} adapters in one call (at most {LORA_MAX_ADAPTERS})")
    n, k = w_base.shape
    na = len(adapters)
    ptr_a, ptr_b = (_lib.c_void_p * max(na, 1))(), (_lib.c_void_p * max(na, 1))()
    lda, ldb = (_lib.c_i64 * max(na, 1))(), (_lib.c_i64 * max(na, 1))()
    rank, scale = (_lib.c_int * max(na, 1))(), (_lib.c_float * max(na, 1))()
    for i, (a, b, s) in enumerate(adapters):
        r = a.shape[0]
        if a.dim() != 2 or b.dim() != 2 or a.shape[1] != k or b.shape != (n, r):
            raise ValueError(f"lora_merge_: adapter {i}: A {tuple(a.shape)} / B {tuple(b.shape)} for a weight {tuple(w_base.shape)}")
        if a.dtype != w_base.dtype or b.dtype != w_base.dtype or not (a.is_cuda and b.is_cuda):
            raise ValueError(f"lora_merge_: adapter {i}: factors must be {w_base.dtype} device tensors")
        if a.stride(1) != 1 or b.stride(1) != 1:
            raise ValueError(f"lora_merge_: adapter {i}: factors need a contiguous last dimension")
        ptr_a[i], ptr_b[i] = a.data_ptr(), b.data_ptr()
        lda[i], ldb[i], rank[i], scale[i] = a.stride(0), b.stride(0), r, float(s)
    _lib.check(_lib.lib().fino_lora_merge(_p(w_base), w_base.stride(0), _p(out), out.stride(0), n, k, na, ptr_a, lda, ptr_b,
                                          ldb, rank, scale, _dt3(w_base), _stream()), "fino_lora_merge")
    return out


STEP_CACHE_MAX_SEGMENTS = 4                # FINO_STEP_CACHE_MAX_SEGMENTS
_STEP_CACHE_WS = {}                        # (device, stream) -> (sums [MAX, 2], partial workspace) fp32


def _rows_of(t, dtype, what):
    if not t.is_cuda:
        raise RuntimeError("frameino_amd ops need CUDA(HIP) tensors; there is no CPU path")
    if t.dim() != 2 or t.stride(1) != 1 or t.dtype != dtype:
        raise ValueError(f"{what}: need a row-strided [rows, D] {dtype} tensor, got {tuple(t.shape)} {t.dtype} strides {t.stride()}")
    return t


def step_cache_probe(h0, h1, p, r, h1_copy=None):
    """First-block-cache probe (fino_step_cache_probe) over S segments: r = T(h1 - h0) (and h1_copy = h1), and the fp32 sums
    (sum |T(r - p)|, sum |p|) of every segment -- a device [S, 2] tensor (valid until the next probe on this device and stream: the host
    reads it right away).  Every argument is a list of S row-strided [rows_s, D] tensors (or one tensor for S = 1); p[s] may be None
    (read as zeros), h1_copy None or a list with None entries (no copy).  The sums are deterministic bit for bit."""
    one = not isinstance(h0, (list, tuple))
    h0, h1, p, r = ([t] for t in (h0, h1, p, r)) if one else (h0, h1, p, r)
    n = len(h0)
    h1_copy = ([h1_copy] if one else h1_copy) if h1_copy is not None else [None] * n
    if not (1 <= n <= STEP_CACHE_MAX_SEGMENTS) or not (len(h1) == len(p) == len(r) == len(h1_copy) == n):
        raise ValueError(f"step_cache_probe: {n} segments (1 .. {STEP_CACHE_MAX_SEGMENTS}), one entry per operand each")
    dt, d, dev = h0[0].dtype, h0[0].shape[-1], h0[0].device
    segs = (_lib.StepCacheSegment * n)()
    for s in range(n):
        rows = h0[s].shape[0]
        for t, what in ((h0[s], "h0"), (h1[s], "h1"), (p[s], "p"), (r[s], "r"), (h1_copy[s], "h1_copy")):
            if t is not None and (_rows_of(t, dt, f"step_cache_probe {what}").shape != (rows, d) or t.device != dev):
                raise ValueError(f"step_cache_probe: segment {s}: {what} is {tuple(t.shape)} on {t.device}, want {(rows, d)} on {dev}")
        g = segs[s]
        g.h0, g.h1, g.p, g.r, g.h1_copy = _p(h0[s]), _p(h1[s]), _p(p[s]), _p(r[s]), _p(h1_copy[s])
        g.rows, g.ld_h0, g.ld_h1, g.ld_r = rows, h0[s].stride(0), h1[s].stride(0), r[s].stride(0)
        g.ld_p = p[s].stride(0) if p[s] is not None else 0
        g.ld_h1_copy = h1_copy[s].stride(0) if h1_copy[s] is not None else 0
    key = (str(dev), _stream())             # two CFG branches on two streams never share the sums
    if key not in _STEP_CACHE_WS:
        _STEP_CACHE_WS[key] = (torch.zeros((STEP_CACHE_MAX_SEGMENTS, 2), dtype=torch.float32, device=dev),
                               torch.empty(2 * STEP_CACHE_MAX_SEGMENTS * 1024, dtype=torch.float32, device=dev))
    sums, ws = _STEP_CACHE_WS[key]
    _lib.check(_lib.lib().fino_step_cache_probe(segs, n, d, _p(sums), _p(ws), _dt3(h0[0]), _stream()), "fino_step_cache_probe")
    return sums[:n]


def step_cache_residual(a, b, out=None, subtract=True):
    """out = T(a - b) (subtract) or T(a + b): torch's `a - b` / `a + b` in the storage dtype, bit for bit
    (fino_step_cache_residual; bf16 / fp16 / fp32, row-strided [rows, D]; out may alias a or b)."""
    _rows_of(a, a.dtype, "step_cache_residual a")
    _rows_of(b, a.dtype, "step_cache_residual b")
    out = torch.empty_like(a) if out is None else _rows_of(out, a.dtype, "step_cache_residual out")
    if a.shape != b.shape or out.shape != a.shape:
        raise ValueError(f"step_cache_residual: shapes {tuple(a.shape)} / {tuple(b.shape)} / {tuple(out.shape)}")
    rows, d = a.shape
    _lib.check(_lib.lib().fino_step_cache_residual(_p(a), a.stride(0), _p(b), b.stride(0), _p(out), out.stride(0), rows, d,
                                                   int(bool(subtract)), _dt3(a), _stream()), "fino_step_cache_residual")
    return out


_MAGCACHE_WS = {}                          # (device, stream) -> the partials' workspace (bytes)


def magcache_calibrate(x_out, x_in, r_prev, r_new, stats):
    """MagCache's calibration pass (fino_magcache_calibrate): r_new = T(x_out - x_in), bit for bit `step_cache_residual`'s, and in
    the same pass stats[0] = mean over rows of ||r_new|| / (||r_prev|| + 1e-8), stats[1] = mean over rows of the cosine distance
    1 - <r_new, r_prev> / max(||r_new|| ||r_prev||, 1e-8) -- norms over the rounded values in fp32, means in fp64.  Row-strided
    [rows, D] bf16 / fp16 / fp32 operands; r_new may be r_prev; `stats` a caller-owned fp64 device tensor [2].  Nothing is read
    back: the call adds no host sync.  Deterministic bit for bit.  -> r_new"""
    dt = x_out.dtype
    _rows_of(x_out, dt, "magcache_calibrate x_out")
    for t, what in ((x_in, "x_in"), (r_prev, "r_prev"), (r_new, "r_new")):
        if _rows_of(t, dt, f"magcache_calibrate {what}").shape != x_out.shape or t.device != x_out.device:
            raise ValueError(f"magcache_calibrate: {what} is {tuple(t.shape)} on {t.device}, want {tuple(x_out.shape)} on "
                             f"{x_out.device}")
    if (not stats.is_cuda or stats.dtype != torch.float64 or tuple(stats.shape) != (2,) or stats.stride(0) != 1
            or stats.device != x_out.device):
        raise ValueError(f"magcache_calibrate: stats must be a contiguous fp64 [2] tensor on {x_out.device}, got "
                         f"{tuple(stats.shape)} {stats.dtype} on {stats.device}")
    rows, d = x_out.shape
    if rows < 1:
        raise ValueError("magcache_calibrate: no rows")
    need = _lib.lib().fino_magcache_workspace_bytes(rows)
    key = (str(x_out.device), _stream())    # two CFG branches on two streams never share the partials
    ws = _MAGCACHE_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = _MAGCACHE_WS[key] = torch.empty(need, dtype=torch.uint8, device=x_out.device)
    _lib.check(_lib.lib().fino_magcache_calibrate(_p(x_out), x_out.stride(0), _p(x_in), x_in.stride(0), _p(r_prev),
                                                  r_prev.stride(0), _p(r_new), r_new.stride(0), rows, d, _dt3(x_out), _p(stats),
                                                  _p(ws), ws.numel(), _stream()), "fino_magcache_calibrate")
    return r_new


_TEACACHE_WS = {}                          # (device, stream) -> the partials' workspace (bytes)


def teacache_probe(x, plane, stats, shift=None, scale=None, sel=None, eps=1e-6, compare=True):
    """TeaCache's probe (fino_teacache_probe): m = T(LN(x) * (1 + scale[sel]) + shift[sel]), bit for bit `adaln_modulate`'s
    (shift and scale None: the plain mode, m = x); with `compare` stats[0] = sum |m - p| and stats[1] = sum |p| against the
    p that `plane` held -- row sums over the rounded values in fp32, sums over rows in fp64 --, without it (0, 0) and the plane is
    not read; then plane = m, in place.  Row-strided [rows, D] bf16 / fp16 operands; shift / scale fp32 [R, D] views of one
    table, as `adaln_modulate` takes them; `stats` a caller-owned fp64 device tensor [2].  Nothing is read back: the call adds
    no host sync.  Deterministic bit for bit.  -> plane"""
    dt = x.dtype
    _dt(x)
    _rows_of(x, dt, "teacache_probe x")
    if _rows_of(plane, dt, "teacache_probe plane").shape != x.shape or plane.device != x.device:
        raise ValueError(f"teacache_probe: plane is {tuple(plane.shape)} on {plane.device}, want {tuple(x.shape)} on {x.device}")
    if (not stats.is_cuda or stats.dtype != torch.float64 or tuple(stats.shape) != (2,) or stats.stride(0) != 1
            or stats.device != x.device):
        raise ValueError(f"teacache_probe: stats must be a contiguous fp64 [2] tensor on {x.device}, got "
                         f"{tuple(stats.shape)} {stats.dtype} on {stats.device}")
    if (shift is None) != (scale is None):
        raise ValueError("teacache_probe: shift and scale come together (both None: the plain mode)")
    if shift is None and sel is not None:
        raise ValueError("teacache_probe: a selector needs shift and scale")
    rows, d = x.shape
    if rows < 1:
        raise ValueError("teacache_probe: no rows")
    ms = 0
    if shift is not None:
        for t, what in ((shift, "shift"), (scale, "scale")):
            if t.dtype != torch.float32 or t.device != x.device or t.shape[-1] != d or t.stride(-1) != 1 or t.dim() > 2:
                raise ValueError(f"teacache_probe: {what} must be fp32 [R, {d}] rows on {x.device}, got {tuple(t.shape)} {t.dtype} "
                                 f"on {t.device}")
        ms = shift.stride(0) if shift.dim() == 2 else 0
        if scale.dim() == 2 and scale.stride(0) != ms:
            raise ValueError("teacache_probe: shift and scale must be views of one table (the same row stride)")
        if sel is not None and (sel.dtype != torch.int32 or sel.dim() != 1 or sel.shape[0] != rows or sel.stride(0) != 1
                                or sel.device != x.device):
            raise ValueError(f"teacache_probe: sel must be a contiguous int32 [{rows}] tensor on {x.device}")
    need = _lib.lib().fino_teacache_workspace_bytes(rows)
    key = (str(x.device), _stream())        # two CFG branches on two streams never share the partials
    ws = _TEACACHE_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = _TEACACHE_WS[key] = torch.empty(need, dtype=torch.uint8, device=x.device)
    _lib.check(_lib.lib().fino_teacache_probe(_p(x), x.stride(0), _p(plane), plane.stride(0), rows, d, _p(shift), _p(scale), ms,
                                              _p(sel), eps, int(bool(compare)), _dt(x), _p(stats), _p(ws), ws.numel(), _stream()),
               "fino_teacache_probe")
    return plane


def pab_broadcast(x, y, gate=None, sel=None, out=None):
    """out = T(fma(float(y), gate[sel], float(x))) (gate None: T(x + y)): the gated-residual epilogue of `gemm` applied to a
    cached y, bit for bit what the GEMM that produced y wrote (fino_pab_broadcast; `gated_residual` rounds y * gate first).
    Row-strided [rows, D] bf16 / fp16; out may alias x."""
    _rows_of(x, x.dtype, "pab_broadcast x")
    _rows_of(y, x.dtype, "pab_broadcast y")
    out = torch.empty_like(x) if out is None else _rows_of(out, x.dtype, "pab_broadcast out")
    if x.shape != y.shape or out.shape != x.shape:
        raise ValueError(f"pab_broadcast: shapes {tuple(x.shape)} / {tuple(y.shape)} / {tuple(out.shape)}")
    if gate is not None:
        assert gate.dtype == torch.float32 and gate.stride(-1) == 1 and gate.shape[-1] == x.shape[1]
    rows, d = x.shape
    ms = gate.stride(0) if (gate is not None and gate.dim() == 2) else 0
    _lib.check(_lib.lib().fino_pab_broadcast(_p(x), x.stride(0), _p(y), y.stride(0), _p(out), out.stride(0), rows, d, _p(gate),
                                             ms, _p(sel), _dt(x), _stream()), "fino_pab_broadcast")
    return out


TAYLOR_MAX_PLANES = 4                      # FINO_TAYLOR_MAX_PLANES
_TAYLOR_FACTOR_DTYPES = (torch.bfloat16, torch.float16, torch.float32)


def _taylor_planes(factors, rows, d, what):
    """the factor planes of a TaylorSeer buffer: [planes, rows, D] bf16 / fp16 / fp32 with a contiguous last dimension"""
    if not factors.is_cuda:
        raise RuntimeError("frameino_amd ops need CUDA(HIP) tensors; there is no CPU path")
    if factors.dim() != 3 or factors.stride(2) != 1 or factors.dtype not in _TAYLOR_FACTOR_DTYPES:
        raise ValueError(f"{what}: factors must be a [planes, rows, D] bf16 / fp16 / fp32 tensor with a contiguous last "
                         f"dimension, got {tuple(factors.shape)} {factors.dtype} strides {factors.stride()}")
    if tuple(factors.shape[1:]) != (rows, d):
        raise ValueError(f"{what}: factor planes are {tuple(factors.shape[1:])}, want {(rows, d)}")
    return factors


def taylor_coefficients(k, n):
    """c_i = float32(k**i / i!) for i < n, computed in double: the weights of a TaylorSeer prediction k steps after the last
    computed step"""
    return [_lib.c_float(float(k) ** i / math.factorial(i)).value for i in range(n)]      # (c_float rounds to nearest even)


def _taylor_bytes(name, ev, nbytes):
    if ev is not None:
        ev.record()
        kt_ = KernelTimer.active
        kt_.bytes[name] = kt_.bytes.get(name, 0.0) + nbytes


def taylor_update(y, factors, n_old, delta, n_new=None):
    """TaylorSeer factor update on a step that computed y (fino_taylor_update), in place: g_0 = F(y),
    g_{i+1} = F((g_i - f_i) / delta) for i + 1 < n_new, then f = g; every operation one fp32 operation, every factor rounded to
    F once.  y row-strided [rows, D] bf16 / fp16; factors [planes, rows, D] of dtype F (bf16 / fp16 / fp32), of which the first
    `n_old` are valid; `n_new` defaults to min(n_old + 1, planes).  Planes at and beyond n_new are not touched.  -> n_new"""
    _rows_of(y, y.dtype, "taylor_update y")
    rows, d = y.shape
    _taylor_planes(factors, rows, d, "taylor_update")
    planes = factors.shape[0]
    n_old, delta = int(n_old), int(delta)
    n_new = min(n_old + 1, planes) if n_new is None else int(n_new)
    if not (0 <= n_old <= planes <= TAYLOR_MAX_PLANES and 1 <= n_new <= min(n_old + 1, planes)):
        raise ValueError(f"taylor_update: n_old={n_old} n_new={n_new} with {planes} planes (at most {TAYLOR_MAX_PLANES}; "
                         f"n_new in 1 .. min(n_old + 1, planes))")
    if delta < 1 and n_new > 1:
        raise ValueError(f"taylor_update: delta={delta} must be at least 1")
    if factors.device != y.device:
        raise ValueError(f"taylor_update: y on {y.device}, factors on {factors.device}")
    ev = _timed("taylor_update")
    _lib.check(_lib.lib().fino_taylor_update(_p(y), y.stride(0), _p(factors), factors.stride(0), factors.stride(1), rows, d, n_old,
                                             n_new, delta, _dt(y), _dt3(factors), _stream()), "fino_taylor_update")
    _taylor_bytes("taylor_update", ev, rows * d * (y.element_size() + (2 * n_new - 1) * factors.element_size()))
    return n_new


def taylor_predict(factors, n, k, x=None, gate=None, sel=None, out=None, dtype=None, coef=None):
    """TaylorSeer prediction k steps after the last update from the first n factor planes (fino_taylor_predict):
    p = f_0 + sum_{i=1}^{n-1} f_i * float32(k**i / i!) in fp32 (the product and the sum each rounded, in that order), then
    out = T(p) (x None), T(x + p) (gate None) or T(fma(p, gate[sel], x)) -- the last two are `pab_broadcast` on y = p.
    factors [planes, rows, D] bf16 / fp16 / fp32; x / out row-strided [rows, D] bf16 / fp16 (`dtype` names T when neither is
    given); out may alias x.  `coef` (at least n host floats, coef[0] is not used) replaces the weights float32(k**i / i!) --
    FasterCache's self-attention extrapolation passes [1, w]."""
    if factors.dim() != 3:
        raise ValueError(f"taylor_predict: factors must be [planes, rows, D], got {tuple(factors.shape)}")
    rows, d = factors.shape[1:]
    _taylor_planes(factors, rows, d, "taylor_predict")
    n = int(n)
    if not (1 <= n <= factors.shape[0] <= TAYLOR_MAX_PLANES):
        raise ValueError(f"taylor_predict: n={n} of {factors.shape[0]} planes (1 .. planes, at most {TAYLOR_MAX_PLANES})")
    t = x.dtype if x is not None else out.dtype if out is not None else dtype
    if t not in (torch.bfloat16, torch.float16):
        raise TypeError(f"taylor_predict: the output dtype must be bf16 or fp16, got {t}")
    if x is not None:
        _rows_of(x, t, "taylor_predict x")
    elif gate is not None or sel is not None:
        raise ValueError("taylor_predict: a gate needs x")
    out = torch.empty((rows, d), dtype=t, device=factors.device) if out is None else _rows_of(out, t, "taylor_predict out")
    if tuple(out.shape) != (rows, d) or (x is not None and tuple(x.shape) != (rows, d)):
        raise ValueError(f"taylor_predict: factor planes {(rows, d)} / x {None if x is None else tuple(x.shape)} / out "
                         f"{tuple(out.shape)}")
    if out.device != factors.device or (x is not None and x.device != factors.device):
        raise ValueError("taylor_predict: operands on different devices")
    if gate is not None:
        assert gate.dtype == torch.float32 and gate.stride(-1) == 1 and gate.shape[-1] == d
    ms = gate.stride(0) if (gate is not None and gate.dim() == 2) else 0
    if coef is not None and len(coef) < n:
        raise ValueError(f"taylor_predict: {len(coef)} coefficients for n={n} planes")
    coef = (_lib.c_float * TAYLOR_MAX_PLANES)(*(taylor_coefficients(k, n) if coef is None else [float(v) for v in coef[:n]]))
    ev = _timed("taylor_predict")
    _lib.check(_lib.lib().fino_taylor_predict(_p(factors), factors.stride(0), factors.stride(1), n, coef, _p(x),
                                              0 if x is None else x.stride(0), _p(out), out.stride(0), rows, d, _p(gate), ms,
                                              _p(sel), _dt(out), _dt3(factors), _stream()), "fino_taylor_predict")
    _taylor_bytes("taylor_predict", ev, rows * d * (n * factors.element_size() + (2 if x is not None else 1) * out.element_size()))
    return out


FASTERCACHE_MAX_PLANE = 16384              # FINO_FASTERCACHE_MAX_PLANE


def fastercache_supported(planes, height, width):
    """whether `fastercache_delta` takes [planes, height, width] (fino_fastercache_supported): every size at least 1 and one
    fp32 plane within 64 KiB of LDS (height * width <= 16384)"""
    return bool(_lib.lib().fino_fastercache_supported(int(planes), int(height), int(width)))


def _fastercache_planes(t, what):
    if not t.is_cuda:
        raise RuntimeError("frameino_amd ops need CUDA(HIP) tensors; there is no CPU path")
    if t.dim() < 2 or not t.is_contiguous():
        raise ValueError(f"{what}: need a contiguous [..., H, W] tensor, got {tuple(t.shape)} strides {t.stride()}")
    return t


def fastercache_delta(uncond, cond, d_low=None, d_high=None):
    """FasterCache's frequency-split difference of the two CFG predictions of one step (fino_fastercache_delta):
    D = float(uncond) - float(cond), d_low = LP(D) and d_high = D - d_low in fp32, LP the radial low-pass of every [H, W] plane
    (the DFT bins with fy^2 + fx^2 <= (min(H, W) // 5)^2 kept).  uncond / cond: contiguous [..., H, W] bf16 / fp16 of one
    shape; d_low / d_high: fp32 of that shape (allocated when None).  Deterministic bit for bit.  -> (d_low, d_high)"""
    _fastercache_planes(uncond, "fastercache_delta uncond")
    _fastercache_planes(cond, "fastercache_delta cond")
    if uncond.dtype not in (torch.bfloat16, torch.float16) or cond.dtype != uncond.dtype or cond.shape != uncond.shape \
            or cond.device != uncond.device:
        raise ValueError(f"fastercache_delta: uncond {tuple(uncond.shape)} {uncond.dtype} on {uncond.device} / cond "
                         f"{tuple(cond.shape)} {cond.dtype} on {cond.device}: need one bf16 / fp16 shape on one device")
    h, w = uncond.shape[-2:]
    planes = uncond.numel() // max(h * w, 1)
    if not fastercache_supported(planes, h, w):
        raise ValueError(f"fastercache_delta: {planes} planes of {h} x {w} are not supported (every size at least 1, "
                         f"H * W at most {FASTERCACHE_MAX_PLANE})")
    d_low = torch.empty(uncond.shape, dtype=torch.float32, device=uncond.device) if d_low is None else d_low
    d_high = torch.empty(uncond.shape, dtype=torch.float32, device=uncond.device) if d_high is None else d_high
    for t, what in ((d_low, "d_low"), (d_high, "d_high")):
        _fastercache_planes(t, f"fastercache_delta {what}")
        if t.dtype != torch.float32 or t.shape != uncond.shape or t.device != uncond.device:
            raise ValueError(f"fastercache_delta: {what} must be fp32 {tuple(uncond.shape)} on {uncond.device}, got "
                             f"{tuple(t.shape)} {t.dtype} on {t.device}")
    ev = _timed("fastercache_delta")
    _lib.check(_lib.lib().fino_fastercache_delta(_p(uncond), _p(cond), _p(d_low), _p(d_high), planes, h, w, _dt(uncond), _stream()),
               "fino_fastercache_delta")
    _taylor_bytes("fastercache_delta", ev, uncond.numel() * (2 * uncond.element_size() + 8))
    return d_low, d_high


def fastercache_apply(cond, d_low, d_high, a_low, a_high, out=None):
    """FasterCache's rebuilt unconditional prediction (fino_fastercache_apply): out = T((float(cond) + a_low * d_low) +
    a_high * d_high), every multiply and add one fp32 operation, one rounding to T.  cond / out contiguous bf16 / fp16, d_low /
    d_high contiguous fp32 of the same number of elements; a_low / a_high host floats (rounded to fp32).  out may be cond."""
    for t, what in ((cond, "cond"), (d_low, "d_low"), (d_high, "d_high")):
        if not t.is_cuda:
            raise RuntimeError("frameino_amd ops need CUDA(HIP) tensors; there is no CPU path")
        if not t.is_contiguous():
            raise ValueError(f"fastercache_apply: {what} must be contiguous, got strides {t.stride()}")
    if cond.dtype not in (torch.bfloat16, torch.float16) or d_low.dtype != torch.float32 or d_high.dtype != torch.float32:
        raise ValueError(f"fastercache_apply: cond {cond.dtype} (bf16 / fp16), d_low {d_low.dtype} / d_high {d_high.dtype} (fp32)")
    n = cond.numel()
    if n < 1 or d_low.numel() != n or d_high.numel() != n:
        raise ValueError(f"fastercache_apply: {n} / {d_low.numel()} / {d_high.numel()} elements (one count, at least 1)")
    out = torch.empty_like(cond) if out is None else out
    if out.dtype != cond.dtype or out.numel() != n or not out.is_contiguous() or not out.is_cuda:
        raise ValueError(f"fastercache_apply: out must be a contiguous {cond.dtype} device tensor of {n} elements")
    if not (out.device == cond.device == d_low.device == d_high.device):
        raise ValueError("fastercache_apply: operands on different devices")
    ev = _timed("fastercache_apply")
    _lib.check(_lib.lib().fino_fastercache_apply(_p(cond), _p(d_low), _p(d_high), float(a_low), float(a_high), _p(out), n,
                                                 _dt(cond), _stream()), "fino_fastercache_apply")
    _taylor_bytes("fastercache_apply", ev, n * (2 * cond.element_size() + 8))
    return out


# ---------------------------------------------------------------------- region-adaptive sampling (fino_token_select.hip)
TOKEN_SELECT_MAX = 65536                   # FINO_TOKEN_SELECT_MAX


def _index_list(idx, what):
    if not idx.is_cuda or idx.dtype != torch.int32 or idx.dim() != 1 or not idx.is_contiguous():
        raise ValueError(f"{what}: the list must be a contiguous int32 [k] device tensor, got {tuple(idx.shape)} {idx.dtype} on "
                         f"{idx.device}")
    return idx


def token_score(po, batch=1, counters=None, starvation_scale=0.0, eligible=None, out=None):
    """The score of every token row of a kept prediction (fino_token_score): po row-strided [batch * rows, cols] bf16 / fp16
    (the batch elements stacked) -> fp32 [rows], the population standard deviation of the row's `cols` values averaged over
    the batch elements, times exp(starvation_scale * counters[row]) (int32 [rows]; None: no factor).  `eligible` (uint8 [rows]):
    0 scores -inf, 2 scores +inf.  Deterministic bit for bit."""
    _rows_of(po, po.dtype, "token_score po")
    batch = int(batch)
    if batch < 1 or po.shape[0] % batch or po.shape[0] < batch:
        raise ValueError(f"token_score: {po.shape[0]} rows for a batch of {batch}")
    rows, cols = po.shape[0] // batch, po.shape[1]
    for t, dt, what in ((counters, torch.int32, "counters"), (eligible, torch.uint8, "eligible")):
        if t is not None and (t.dtype != dt or tuple(t.shape) != (rows,) or not t.is_contiguous() or t.device != po.device):
            raise ValueError(f"token_score: {what} must be a contiguous {dt} [{rows}] tensor on {po.device}")
    out = torch.empty(rows, dtype=torch.float32, device=po.device) if out is None else out
    if out.dtype != torch.float32 or tuple(out.shape) != (rows,) or not out.is_contiguous() or out.device != po.device:
        raise ValueError(f"token_score: out must be a contiguous fp32 [{rows}] tensor on {po.device}")
    _lib.check(_lib.lib().fino_token_score(_p(po), rows, cols, po.stride(0), batch, _p(counters), float(starvation_scale),
                                           _p(eligible), _p(out), _dt(po), _stream()), "fino_token_score")
    return out


def token_select(score, k, counters=None, out=None):
    """The k rows of the largest scores (fino_token_select): fp32 [n] -> int32 [k] in ascending index order, ties to the lower
    index; `counters` (int32 [n]) are set to 0 for the selected rows and incremented for the others.  n <= TOKEN_SELECT_MAX."""
    if not score.is_cuda or score.dtype != torch.float32 or score.dim() != 1 or not score.is_contiguous():
        raise ValueError(f"token_select: score must be a contiguous fp32 [n] device tensor, got {tuple(score.shape)} {score.dtype}")
    n, k = score.shape[0], int(k)
    if counters is not None and (counters.dtype != torch.int32 or tuple(counters.shape) != (n,) or not counters.is_contiguous()
                                 or counters.device != score.device):
        raise ValueError(f"token_select: counters must be a contiguous int32 [{n}] tensor on {score.device}")
    out = torch.empty(max(k, 0), dtype=torch.int32, device=score.device) if out is None else _index_list(out, "token_select out")
    if out.shape[0] != k or out.device != score.device:
        raise ValueError(f"token_select: out holds {out.shape[0]} entries on {out.device}, want {k} on {score.device}")
    _lib.check(_lib.lib().fino_token_select(_p(score), n, k, _p(out), _p(counters), _stream()), "fino_token_select")
    return out


def _row_bytes(t, what):
    if not t.is_cuda:
        raise RuntimeError("frameino_amd ops need CUDA(HIP) tensors; there is no CPU path")
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{what}: need a row-strided [rows, width] tensor, got {tuple(t.shape)} strides {t.stride()}")
    return t.shape[1] * t.element_size(), t.stride(0) * t.element_size()


def gather_rows(src, idx, out=None):
    """out[r] = src[idx[r]] (fino_gather_rows): whole rows of a row-strided [n, width] tensor of any dtype by an int32 list;
    indices are clamped into [0, n)."""
    _index_list(idx, "gather_rows")
    rb, lds = _row_bytes(src, "gather_rows src")
    out = torch.empty((idx.shape[0], src.shape[1]), dtype=src.dtype, device=src.device) if out is None else out
    rbo, ldo = _row_bytes(out, "gather_rows out")
    if rbo != rb or out.dtype != src.dtype or out.shape[0] != idx.shape[0] or out.device != src.device or idx.device != src.device:
        raise ValueError(f"gather_rows: src {tuple(src.shape)} {src.dtype}, {idx.shape[0]} indices, out {tuple(out.shape)} {out.dtype}")
    _lib.check(_lib.lib().fino_gather_rows(_p(src), lds, src.shape[0], _p(idx), idx.shape[0], rb, _p(out), ldo, _stream()),
               "fino_gather_rows")
    return out


def scatter_rows(src, idx, out):
    """out[idx[r]] = src[r] (fino_scatter_rows): the inverse of `gather_rows`; indices are clamped into [0, rows of out)."""
    _index_list(idx, "scatter_rows")
    rb, lds = _row_bytes(src, "scatter_rows src")
    rbo, ldo = _row_bytes(out, "scatter_rows out")
    if rbo != rb or out.dtype != src.dtype or src.shape[0] != idx.shape[0] or out.device != src.device or idx.device != src.device:
        raise ValueError(f"scatter_rows: src {tuple(src.shape)} {src.dtype}, {idx.shape[0]} indices, out {tuple(out.shape)} {out.dtype}")
    _lib.check(_lib.lib().fino_scatter_rows(_p(src), lds, _p(idx), idx.shape[0], rb, _p(out), ldo, out.shape[0], _stream()),
               "fino_scatter_rows")
    return out


def qkv_rmsnorm_rope_rows_(qkv, dim, q_weight, q_eps, k_weight, k_eps, cos, sin, head_dim, idx, kcache, vcache, q_out_scale=1.0):
    """`qkv_rmsnorm_rope_` (in place, bit for bit) on a compact projection qkv [rows, 3 dim] whose row r is token idx[r] (int32
    [rows]; None: token r) and whose cos / sin rows are the compact rows' own; the same launch writes row r's k (as just normed
    and rotated) to kcache[idx[r]] and its v to vcache[idx[r]] -- row-strided [n, dim] planes with one row stride
    (fino_qkv_rmsnorm_rope_rows).  Indices are clamped into [0, n)."""
    x2, rows, width, ldx = _rows2d(qkv)
    assert width == 3 * dim
    assert cos.dtype == torch.float32 and cos.is_contiguous() and cos.shape == (rows, head_dim // 2) and sin.shape == cos.shape
    assert sin.dtype == torch.float32 and sin.is_contiguous()
    _rows_of(kcache, qkv.dtype, "qkv_rmsnorm_rope_rows_ kcache")
    _rows_of(vcache, qkv.dtype, "qkv_rmsnorm_rope_rows_ vcache")
    if kcache.shape != vcache.shape or kcache.shape[1] != dim or kcache.stride(0) != vcache.stride(0):
        raise ValueError(f"qkv_rmsnorm_rope_rows_: planes {tuple(kcache.shape)} / {tuple(vcache.shape)} strides "
                         f"{kcache.stride()} / {vcache.stride()}: need two [n, {dim}] planes with one row stride")
    if idx is not None and _index_list(idx, "qkv_rmsnorm_rope_rows_").shape[0] != rows:
        raise ValueError(f"qkv_rmsnorm_rope_rows_: {idx.shape[0]} indices for {rows} rows")
    if idx is None and rows > kcache.shape[0]:
        raise ValueError(f"qkv_rmsnorm_rope_rows_: {rows} rows for planes of {kcache.shape[0]}")
    _lib.check(_lib.lib().fino_qkv_rmsnorm_rope_rows(_p(x2), rows, dim, ldx, _p(q_weight), q_eps, _p(k_weight), k_eps, _p(cos),
                                                     _p(sin), head_dim, float(q_out_scale), _p(idx), kcache.shape[0], _p(kcache),
                                                     _p(vcache), kcache.stride(0), _dt(qkv), _stream()),
               "fino_qkv_rmsnorm_rope_rows")
    return qkv
