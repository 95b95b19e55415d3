"""MXFP6 (e2m3) linears, the part that needs no GPU: the four entry points exist in header, ctypes table and library and
validate their arguments, and the torch restatement of the rule (tests/mxfp6_ref.py) has the properties the GPU tests
and the format's case rest on."""
import os

import pytest
import torch

from frameino_amd import _lib
from tests import mxfp6_ref as R

SYMBOLS = ["fino_mxfp6_bytes", "fino_mxfp6_scale_bytes", "fino_quantize_mxfp6", "fino_gemm_mxfp6"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_symbols_in_header_table_and_library(lib):
    declared = _lib.declared_symbols()
    for name in SYMBOLS:
        assert name in declared, f"{name} not declared in include/frameino_hip.h"
        assert name in _lib.SIGNATURES, f"{name} not in the ctypes table"
        assert hasattr(lib, name), f"{name} not exported"
    assert lib.fino_version() == 103


def test_sizes_and_argument_validation(lib):
    # the header's layout: [cols/128][rows_pad/16] fragments of 1536 bytes, rows_pad = rows rounded up to 256
    assert lib.fino_mxfp6_bytes(300, 256) == 2 * (512 // 16) * 1536 >= 300 * 256 * 3 // 4
    assert lib.fino_mxfp6_bytes(256, 128) == 256 * 128 * 3 // 4
    assert lib.fino_mxfp6_bytes(300, 100) == 0 and lib.fino_mxfp6_bytes(0, 128) == 0
    assert lib.fino_mxfp6_scale_bytes(256, 100) == 0 and lib.fino_mxfp6_scale_bytes(300, 256) == 2 * 2 * 1024
    rc = lib.fino_quantize_mxfp6(16, 16, 16, 4, 100, 104, 0, 0)
    assert rc == -1 and b"multiple of 128" in lib.fino_last_error()
    rc = lib.fino_quantize_mxfp6(16, 16, 16, 4, 128, 128, 7, 0)
    assert rc == -1 and b"dtype" in lib.fino_last_error()
    rc = lib.fino_quantize_mxfp6(16, 0, 16, 4, 128, 128, 0, 0)
    assert rc == -1 and b"null" in lib.fino_last_error()
    rc = lib.fino_gemm_mxfp6(16, 16, 16, 16, 0, 16, 8, 8, 64, 8, 0, 0, 0, 0, 0, 0, 0, 0)
    assert rc == -1 and b"multiple of 128" in lib.fino_last_error()
    rc = lib.fino_gemm_mxfp6(16, 16, 16, 16, 0, 16, 8, 8, 128, 8, 9, 0, 0, 0, 0, 0, 0, 0)
    assert rc == -1 and b"epilogue" in lib.fino_last_error()
    rc = lib.fino_gemm_mxfp6(16, 16, 16, 16, 0, 16, 8, 8, 128, 8, 2, 0, 0, 0, 0, 0, 0, 0)
    assert rc == -1 and b"residual" in lib.fino_last_error()
    rc = lib.fino_gemm_mxfp6(16, 16, 16, 16, 0, 16, 1 << 20, 8, 1 << 12, 8, 0, 0, 0, 0, 0, 0, 0, 0)
    assert rc == -3 and b"2 GiB" in lib.fino_last_error()
    assert lib.fino_gemm_mxfp6(16, 16, 16, 16, 0, 16, 0, 8, 128, 8, 0, 0, 0, 0, 0, 0, 0, 0) == 0      # M = 0: nothing to do


def _x(rows, cols, seed, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, cols, generator=g) * torch.exp2(torch.randint(-6, 6, (rows, 1), generator=g).float())).to(dtype)
    x[0, :32] = 0
    return x


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_reference_quantiser_error_bound_zero_blocks_and_fixed_point(dtype):
    x = _x(77, 1024, 1, dtype)
    codes, e = R.quantize_ref(x)
    assert codes.dtype == torch.uint8 and int(codes.max()) < 64 and e.shape == (77, 32)
    y = R.decode(codes, e)
    blk = x.float().view(77, 32, 32)
    amax = blk.abs().amax(-1, keepdim=True)
    # the scaled amax is above 3.75 and half an e2m3 step in the top binade is 0.25: |error| <= amax * 0.25 / 3.75
    assert ((y.view(77, 32, 32) - blk).abs() <= amax / 15).all()
    assert (y[0, :32] == 0).all() and int(e[0, 0]) == -127
    # the scaled amax lies in (3.75, 7.5]: nothing saturates, no scale is a binade too large
    scaled = amax.squeeze(-1)[amax.squeeze(-1) > 0] / torch.exp2(e.float()[amax.squeeze(-1) > 0])
    assert (scaled > 3.75).all() and (scaled <= 7.5).all()
    codes2, e2 = R.quantize_ref(y)
    assert torch.equal(R.decode(codes2, e2), y)                       # decoding is a fixed point (codes may differ)


def test_block_with_amax_exactly_at_the_top_keeps_it():
    for k in (-20, -3, 0, 5, 40):
        x = torch.zeros(1, 32)
        x[0, 3] = -7.5 * 2.0 ** k                                     # exactly the largest e2m3 magnitude times 2^k
        x[0, 4] = 3.0 * 2.0 ** k
        codes, e = R.quantize_ref(x.bfloat16())
        assert int(e[0, 0]) == k and int(codes[0, 3]) == 63
        assert torch.equal(R.decode(codes, e), x)
        x[0, 3] = 7.75 * 2.0 ** k                                     # the next bf16-representable step up moves the scale
        codes, e = R.quantize_ref(x.bfloat16())
        assert int(e[0, 0]) == k + 1


def test_ties_round_to_even_and_every_code_decodes():
    codes = torch.arange(64, dtype=torch.uint8).view(2, 32)
    e = torch.zeros(2, 1, dtype=torch.int32)
    vals = R.decode(codes, e)
    assert vals[0].tolist() == R.GRID.float().tolist() and torch.equal(vals[1], -vals[0])
    x = torch.zeros(1, 32)
    x[0, 0] = 7.5                                                     # pins e = 0
    x[0, 1:7] = torch.tensor([0.0625, 0.1875, 1.9375, 2.125, 2.375, 4.25])        # ties between neighbours
    got = R.decode(*R.quantize_ref(x))[0, 1:7].tolist()
    assert got == [0.0, 0.25, 2.0, 2.0, 2.5, 4.0]


def test_gemm_error_of_e2m3_is_that_of_e4m3():
    """the claim the format rests on: with the block scale supplying the range, e2m3's three mantissa bits give the MXFP8
    GEMM error on Gaussian operands (ratio 1.06 measured)"""
    g = torch.Generator().manual_seed(11)
    a = torch.randn(128, 3072, generator=g).bfloat16()
    w = torch.randn(128, 3072, generator=g).bfloat16()
    ref = a.double() @ w.double().T

    def err(ad, wd):
        return float(((ad.double() @ wd.double().T - ref).pow(2).mean() / ref.pow(2).mean()).sqrt())

    r6 = err(R.decode(*R.quantize_ref(a)), R.decode(*R.quantize_ref(w)))
    r8 = err(R.quantize_e4m3_ref(a), R.quantize_e4m3_ref(w))
    print(f"GEMM rel-RMS K=3072: e2m3 {r6:.4f}  e4m3 {r8:.4f}  ratio {r6 / r8:.3f}")
    assert 0.95 <= r6 / r8 <= 1.2


def test_unpack_inverts_the_documented_layout():
    """pack a known code matrix by the header's words, in plain python, and read it back with unpack()"""
    rows, cols = 20, 256
    g = torch.Generator().manual_seed(5)
    codes = torch.randint(0, 64, (rows, cols), generator=g).to(torch.uint8)
    e = torch.randint(-10, 10, (rows, cols // 32), generator=g).to(torch.int32)
    rp = 256
    q = torch.zeros(cols // 128 * rp // 16 * 1536, dtype=torch.uint8)
    s = torch.zeros(cols // 128 * rp * 4, dtype=torch.uint8)
    for row in range(rows):
        for b in range(cols // 32):
            kt, gk = b // 4, b % 4
            bits = 0
            for j in range(32):
                bits |= int(codes[row, b * 32 + j]) << (6 * j)
            raw = bits.to_bytes(24, "little")
            lane = 16 * gk + (row & 15)
            base = (kt * (rp // 16) + row // 16) * 1536
            q[base + 16 * lane: base + 16 * lane + 16] = torch.tensor(list(raw[:16]), dtype=torch.uint8)
            q[base + 1024 + 8 * lane: base + 1024 + 8 * lane + 8] = torch.tensor(list(raw[16:]), dtype=torch.uint8)
            s[(kt * (rp // 256) + row // 256) * 1024 + gk * 256 + (row & 15) * 16 + ((row & 255) >> 4)] = int(e[row, b]) + 127
    c2, e2 = R.unpack(q, s, rows, cols)
    assert torch.equal(c2, codes) and torch.equal(e2, e)
