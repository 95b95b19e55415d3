"""Float64 reference, derived per-element bound, loop predictor and edge-geometry table of the implicit-GEMM convolution
(fino_conv3d / fino_conv3d_split, frameino_amd/csrc/fino_gemm.hip).  CPU, torch only: shared by tests/test_conv_ref_cpu.py
(which shows that the bound rejects subtly wrong gathers) and tests/test_conv3d_edges_gpu.py (which holds the kernels to it).

THE BOUND.  With operands already rounded to the storage type, the kernel computes acc = sum of K exact products in the
MFMA's fp32 accumulator, adds the bias in fp32 and rounds ONCE to T:
    |got - ref| <= roundings * u_T * |ref|  +  2 * K * 2^-24 * S,        S = conv(|x|, |w|) + |b|
  * 2 * K * 2^-24 * S: recursive fp32 summation of K terms has the classical bound (K - 1) * u * sum|terms| with u = 2^-24
    for round-to-nearest; the factor 2 allows for the MFMA's internal accumulate not being round-to-nearest (u = 2^-23 if it
    truncates).  K = kt * kh * kw * c_in_pad (times the number of products for the split conv); the fp32 bias add is one
    more rounding of a value <= S and is inside the slack between K - 1 and 2 K.
  * roundings * u_T * |ref|: u_T = 2^-8 (bf16, 8 significant bits) or 2^-11 (fp16, 11) per rounding.  That is one whole
    ulp at the top of a binade and half an ulp at its bottom, where round-to-nearest-even attains it: the honest reference
    rounded once reaches 0.99 of the bound on a K = 64 row (tests/test_conv_ref_cpu.py prints it).  The rounding acts on the
    computed value v = ref + e, not on ref: |T(v) - ref| <= |e| (1 + u_T) + u_T |ref|, and the factor (1 + u_T) on the
    accumulation error e is inside the factor 2 above.
    roundings = 1, counted in gemm_epilogue_t (frameino_amd/csrc/fino_gemm_common.h): the only conversion of the
    accumulator is T::from_f32(acc + bias) in the loop that writes the tile to LDS ("y = T(acc + bias)"); FINO_EPI_NONE then
    copies those bits to global memory.  FINO_EPI_RESIDUAL unpacks that T value again, adds r in fp32 and packs once more
    (pack8<T>(rv + y)): a second rounding, but of a value that the plain run has already fixed, so the residual run is checked
    bit for bit -- torch.equal(y_res, (y.float() + r.float()).to(T)) -- and never needs roundings = 2.
  * split conv (fp32 in, fp32 out, ops.SPLIT_PRODUCTS[planes]): no rounding to T; the first term becomes drop * S, the weight
    of the products the truncated expansion leaves out.  split3 (fino_vae.hip) writes x = hi + mid + lo + rest with every
    plane rounded to nearest: |mid| <= 2^-8 |x|, |lo| <= 2^-16 |x|, |rest| <= 2^-24 |x|, |hi| <= (1 + 2^-8) |x|.
      2 planes (x = xh + xl + xr, |xl| <= 2^-8 |x|, |xr| <= 2^-16 |x|; products hh, hl, lh kept):
          x w - kept = xl wl + xl wr + xr w + xh wr
                    <= (2^-16 + 2^-24 + 2^-16 + (1 + 2^-8) 2^-16) |x||w|            ~ 3 * 2^-16 = 1.5 * 2^-15
      3 planes (products hh, hm, hl, mh, mm, lh kept):
          x w - kept = xm wl + xl wm + xl wl + xr w + (x - xr) wr
                    <= (2^-24 + 2^-24 + 2^-32 + 2^-24 + (1 + 2^-24) 2^-24) |x||w|    ~ 4 * 2^-24 = 2^-22
    and the accumulate term keeps its form with K = taps * c_in_pad * products (the products are exact in fp32: 16
    significant bits).  The fp32 store is the accumulator itself.
"""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

BM, BN, BK = 256, 256, 64
U_T = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
SPLIT_DROP = {2: 2.0 ** -16 + 2.0 ** -24 + 2.0 ** -16 + (1 + 2.0 ** -8) * 2.0 ** -16,
              3: 2.0 ** -24 + 2.0 ** -24 + 2.0 ** -32 + 2.0 ** -24 + (1 + 2.0 ** -24) * 2.0 ** -24}
SPLIT_NPROD = {0: 1, 2: 3, 3: 6}

Geom = namedtuple("Geom", "id kernel stride pad up thw cin_pad cout_pad out_thw loop")

# The smallest shapes that reach each edge (tile arithmetic: M = To*Ho*Wo rows in 256-row tiles, N = cout_pad in 256-column
# tiles, K-tiles of 64 = one 64-channel chunk of one tap).  `loop` is what conv3d_impl picks with no tune key.  No shape had
# to be adjusted: expected_loop and the tile arithmetic below agree with every edge named.
GEOMS = [
    # M = 693 = 256 + 256 + 181 (ragged last tile); hw = 99: tile 1 starts at m = 256 -> t_first = 2, base max(0, 2 - 2) = 0;
    # tile 2 at m = 512 -> t_first = 5, base 3 > 0; both start mid-frame; cin_chunks = 1 (offsets recomputed every K-tile)
    Geom("causal-3tiles", (3, 3, 3), (1, 1, 1), (2, 1, 1), False, (7, 9, 11), 64, 64, None, "pingpong"),
    # hw = 323 > 256: tile 1 (m = 256) starts in row 13, column 9 of frame 0 with base max(0, -2) = 0 (NEGATIVE before the
    # clamp), tile 2 straddles frames 1 | 2; M = 969 = 3 * 256 + 201 (four tiles, the last ragged); N = 320: N tile 1 has 64 columns -> w_pieces = 2, gemm_load_bias fast on N tile 0 only
    Geom("causal-midrow", (3, 3, 3), (1, 1, 1), (2, 1, 1), False, (3, 17, 19), 128, 320, None, "pingpong"),
    # hw = 4: tile 0 spans 64 frames (t_span = 65 of the 8-bit frame field), M = 280: tile 1 has 24 rows, t_first = 64
    Geom("many-frames", (3, 3, 3), (1, 1, 1), (2, 1, 1), False, (70, 2, 2), 64, 64, None, "pingpong"),
    # hw = 1: t_span = 256 does not fit the 8-bit field -> one-barrier loop by itself; M = 300
    Geom("one-pixel", (3, 3, 3), (1, 1, 1), (2, 1, 1), False, (300, 1, 1), 64, 64, None, "one_barrier"),
    # To = 20, M = 400; tile 1: t_first = 12, t_in_first = 24
    Geom("time-down", (3, 1, 1), (2, 1, 1), (0, 0, 0), False, (41, 4, 5), 64, 128, None, "pingpong"),
    # out (3, 10, 11): one implicit zero row and column at the far edge; M = 330
    Geom("space-down", (1, 3, 3), (1, 2, 2), (0, 0, 0), False, (3, 20, 22), 64, 64, (3, 10, 11), "pingpong"),
    # out (3, 14, 18), M = 756 = 2 * 256 + 244; hi >> 1, wi >> 1 on odd H, W; N = 256: one full tile (bias fast branch)
    Geom("up2x", (1, 3, 3), (1, 1, 1), (0, 1, 1), True, (3, 7, 9), 128, 256, None, "pingpong"),
    # nk = 1: the `if (nk > 1)` prologue is skipped; N = 512: two full N tiles
    Geom("1x1-nk1", (1, 1, 1), (1, 1, 1), (0, 0, 0), False, (3, 10, 11), 64, 512, None, "pingpong"),
    # nk = 3 (odd), cin_chunks = 3
    Geom("1x1-nk3", (1, 1, 1), (1, 1, 1), (0, 0, 0), False, (3, 10, 11), 192, 64, None, "pingpong"),
    # cin_chunks = 5, nk = 15; N = 96 -> w_pieces = 3; M = 378, hw = 63: tile 1 t_first = 4, base 2
    Geom("time-conv-wideK", (3, 1, 1), (1, 1, 1), (2, 0, 0), False, (6, 7, 9), 320, 96, None, "pingpong"),
    # c_out_pad = 72 is no multiple of 32 -> one-barrier loop by itself (and the split conv refuses); M = 312
    Geom("narrow-N", (1, 3, 3), (1, 1, 1), (0, 1, 1), False, (2, 12, 13), 64, 72, None, "one_barrier"),
]
GEOM_BY_ID = {g.id: g for g in GEOMS}
SPLIT_ROWS = ("causal-3tiles", "causal-midrow", "many-frames", "time-down", "space-down", "up2x", "1x1-nk1")


def out_thw(g):
    """the output extent of ops.conv3d_cl: given, or from the front time pad and the symmetric spatial pads"""
    if g.out_thw is not None:
        return g.out_thw
    up = 2 if g.up else 1
    t, h, w = g.thw
    return ((t + g.pad[0] - g.kernel[0]) // g.stride[0] + 1, (h * up + 2 * g.pad[1] - g.kernel[1]) // g.stride[1] + 1,
            (w * up + 2 * g.pad[2] - g.kernel[2]) // g.stride[2] + 1)


def taps(g):
    return g.kernel[0] * g.kernel[1] * g.kernel[2]


def _padded(x5, kernel, stride, pad, up, out):
    """[1, C, T, H, W] -> upsampled, zero-padded so that a VALID convolution yields at least `out` positions"""
    if up:
        x5 = x5.repeat_interleave(2, dim=3).repeat_interleave(2, dim=4)      # nearest-exact x2: source index = i >> 1
    far = [max(0, (out[d] - 1) * stride[d] + kernel[d] - x5.shape[2 + d] - pad[d]) for d in range(3)]
    return F.pad(x5, (pad[2], far[2], pad[1], far[1], pad[0], far[0]))


def conv_ref64(x, w, b, kernel, stride, pad, up, out_thw):
    """What ops.conv3d_cl documents, in float64, on operands ALREADY rounded to the storage type:
      x [T, H, W, Cin_pad] channels-last, w [Cout_pad, kt*kh*kw*Cin_pad] tap-major / channel-minor, b [Cout_pad] or None;
      nearest-exact 2x spatial upsample first (if `up`), front-only time pad pad[0], symmetric pad[1], pad[2], and implicit
      zero rows / columns at the far edge where out_thw asks for more than that gives (the `down conv2d s2` convention).
    Returns (ref, S) as float64 [To, Ho, Wo, Cout_pad], S = conv(|x|, |w|) + |b| (the scale of the accumulation error)."""
    kt, kh, kw = kernel
    cin = x.shape[3]
    cout = w.shape[0]
    assert w.shape[1] == kt * kh * kw * cin
    x5 = x.double().permute(3, 0, 1, 2)[None]
    w5 = w.double().reshape(cout, kt, kh, kw, cin).permute(0, 4, 1, 2, 3).contiguous()
    b1 = torch.zeros(cout, dtype=torch.float64) if b is None else b.double()
    xp = _padded(x5, kernel, stride, pad, up, out_thw)
    to, ho, wo = out_thw
    ref = F.conv3d(xp, w5, b1, stride=stride)[0, :, :to, :ho, :wo].permute(1, 2, 3, 0).contiguous()
    s = F.conv3d(xp.abs(), w5.abs(), b1.abs(), stride=stride)[0, :, :to, :ho, :wo].permute(1, 2, 3, 0).contiguous()
    assert tuple(ref.shape) == (to, ho, wo, cout), (ref.shape, out_thw)
    return ref, s


def bound(ref, S, K, dtype, roundings=1, planes=0):
    """per-element |got - ref| allowed (module docstring): dtype bf16 / fp16 with `roundings` roundings to T, or the fp32
    split conv of `planes` planes (K then counts the products too)"""
    acc = 2.0 * K * 2.0 ** -24 * S
    if planes:
        assert dtype == torch.float32
        return SPLIT_DROP[planes] * S + acc
    return roundings * U_T[dtype] * ref.abs() + acc


def expected_loop(g, planes=0, tune=0, pingpong_env=True):
    """the `pp` condition of conv3d_impl (fino_gemm.hip) restated: "pingpong" or "one_barrier" """
    to, ho, wo = out_thw(g)
    t_in, h_in, w_in = g.thw
    kt, st = g.kernel[0], g.stride[0]
    products = SPLIT_NPROD[planes]
    a_width = (planes if planes else 1) * g.cin_pad
    k = taps(g) * g.cin_pad * products
    hw_out = ho * wo
    t_span = (BM - 1 + hw_out - 1) // hw_out + 1                 # output frames a 256-row tile can straddle
    in_span_bytes = (t_span * st + kt) * h_in * w_in * a_width * 2
    w_bytes = ((g.cout_pad - 1) * k + k) * 2
    pp = (pingpong_env and tune != 1 and in_span_bytes < (1 << 31) and ho < 4096 and wo < 4096 and t_span < 256 and
          g.cout_pad % 32 == 0 and w_bytes < (1 << 31))
    return "pingpong" if pp else "one_barrier"


def common_grid(v):
    """round fp32 values so that bf16 AND fp16 hold them exactly (bf16's 8 bits, fp16's range): one reference serves both"""
    v = v.bfloat16().float().half().float()
    assert torch.equal(v.bfloat16().float(), v) and torch.equal(v.half().float(), v)
    return v


def make_operands(g, seed=0, exact16=True):
    """seeded randn operands of geometry g on the CPU in fp32: x [T, H, W, cin_pad], w [cout_pad, taps * cin_pad] scaled
    by 1 / sqrt(c_in * taps), b [cout_pad]; the pad channels (the last 3 inputs, the last 5 outputs) are zero.  exact16:
    values on the grid that bf16 and fp16 share (common_grid); otherwise plain fp32 (the split conv's inputs)."""
    gen = torch.Generator().manual_seed(seed)
    t, h, w_ = g.thw
    cin, cout = g.cin_pad - 3, g.cout_pad - 5
    x = torch.zeros(t, h, w_, g.cin_pad)
    x[..., :cin] = torch.randn(t, h, w_, cin, generator=gen)
    w = torch.zeros(g.cout_pad, taps(g), g.cin_pad)
    w[:cout, :, :cin] = torch.randn(cout, taps(g), cin, generator=gen) / math.sqrt(cin * taps(g))
    w = w.reshape(g.cout_pad, -1)
    b = torch.zeros(g.cout_pad)
    b[:cout] = torch.randn(cout, generator=gen) * 0.1
    if exact16:
        x, w, b = common_grid(x), common_grid(w), common_grid(b)
    return x, w, b, cout
