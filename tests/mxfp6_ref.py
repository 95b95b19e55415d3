"""Plain-torch restatement of the MXFP6 (e2m3) rule and of the layout `fino_quantize_mxfp6` writes (include/frameino_hip.h).
No library call: the tests compare the kernels against this file.

Element: 6 bits = sign (bit 5), exponent (bits 4:3, bias 1), mantissa (bits 2:0); exponent 0 is subnormal (m / 8), otherwise
(1 + m / 8) * 2^(exponent - 1); largest magnitude 7.5.  Block = 32 consecutive K-elements with scale 2^e, e the smallest
integer with amax <= 7.5 * 2^e, clamped to [-127, 127], -127 for an all-zero block; element = RNE(v / 2^e) onto the grid."""
import torch

# the 32 non-negative e2m3 values, indexed by the 5 low code bits
GRID = torch.tensor([m / 8 for m in range(8)] + [(1 + m / 8) * 2.0 ** (ex - 1) for ex in (1, 2, 3) for m in range(8)],
                    dtype=torch.float64)


def block_exponent(amax):
    """smallest integer e with amax <= 7.5 * 2^e (amax > 0; float64 tensor), computed from frexp: no division"""
    m, x = torch.frexp(amax)                       # amax = m * 2^x, m in [0.5, 1)
    return x - torch.where(m <= 0.9375, 3, 2)


def quantize_ref(x):
    """x [rows, cols] (cols % 32 == 0) -> (codes uint8 [rows, cols] in 0..63, e int32 [rows, cols / 32])"""
    rows, cols = x.shape
    xf = x.detach().cpu().double()
    blk = xf.view(rows, cols // 32, 32)
    amax = blk.abs().amax(-1)
    e = block_exponent(torch.where(amax > 0, amax, torch.ones_like(amax))).to(torch.int32)
    e = torch.where(amax > 0, e, torch.full_like(e, -127)).clamp(-127, 127)
    y = (blk * torch.exp2(-e.double()).unsqueeze(-1)).abs()          # exact: powers of two
    # round to nearest, ties to the even code: the grid is uniform inside a binade and consecutive codes alternate parity
    hi = torch.searchsorted(GRID, y.contiguous(), right=False).clamp(max=31)      # first grid value >= y
    lo = (hi - 1).clamp(min=0)
    dlo, dhi = y - GRID[lo], GRID[hi] - y
    pick_hi = (dhi < dlo) | ((dhi == dlo) & (hi % 2 == 0))
    mag = torch.where(pick_hi, hi, lo)
    sign = torch.signbit(blk).to(torch.int64) * 32
    return (mag + sign).to(torch.uint8).view(rows, cols), e


def decode(codes, e):
    """-> fp32 [rows, cols]"""
    c = codes.long()
    val = GRID[c & 31] * torch.where((c & 32) != 0, -1.0, 1.0)
    return (val * torch.exp2(e.double()).repeat_interleave(32, dim=1)).float()


def unpack(q, scales, rows, cols):
    """the library's two buffers -> (codes [rows, cols] uint8, e [rows, cols / 32] int32).
    q: [cols/128][rows_pad/16] fragments of 1536 B; lane l = 16 g + r owns bytes [16 l, +16) and [1024 + 8 l, +8) = the
    192-bit little-endian string of block g of row r, element j in bits [6j, 6j + 6).  scales: the MXFP8 layout."""
    rp = (rows + 255) // 256 * 256
    kt = cols // 128
    f = q.detach().cpu().view(kt, rp // 16, 1536)
    lane = torch.cat([f[..., :1024].reshape(kt, rp // 16, 64, 16), f[..., 1024:].reshape(kt, rp // 16, 64, 8)], dim=-1)
    b = lane.reshape(kt, rp // 16, 64, 8, 3).long()                          # 3 bytes = 4 codes
    v = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
    c = torch.stack([(v >> (6 * i)) & 63 for i in range(4)], dim=-1).reshape(kt, rp // 16, 4, 16, 32)   # [kt][rg][g][r][j]
    codes = c.permute(1, 3, 0, 2, 4).reshape(rp, cols)[:rows].to(torch.uint8)
    s = scales.detach().cpu().view(kt, rp // 256, 4, 16, 16)                 # [kt][rt][g][row & 15][row >> 4]
    e = s.permute(1, 4, 3, 0, 2).reshape(rp, cols // 32)[:rows].to(torch.int32) - 127
    return codes, e


def quantize_e4m3_ref(x):
    """MXFP8 by this repository's rule (amax scaled into (224, 448], RNE) -> dequantised fp32 [rows, cols]"""
    rows, cols = x.shape
    blk = x.detach().cpu().float().view(rows, cols // 32, 32)
    amax = blk.abs().amax(-1, keepdim=True)
    _, ex = torch.frexp(torch.where(amax > 0, amax, torch.ones_like(amax)) / 448.0)
    scale = torch.exp2(ex.float())
    return ((blk / scale).to(torch.float8_e4m3fn).float() * scale).view(rows, cols)
