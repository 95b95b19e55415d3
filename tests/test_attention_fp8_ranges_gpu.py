"""fino_attn_fwd_fp8_ranges (csrc/fino_attention_fp8.hip, attn_fp8_fr_kernel<T, PX, true>): the head_dim-64 fp8 attention in which
every 256 query rows walk up to three ranges of 64-key tiles taken from a device table (two 128-row workgroups share a table row).

The expected result is EXACT.  The free-running kernel runs whole 128-row blocks (no tail split), the pre-pass quantises K per key
and V per 32 keys inside a 64-key tile, so K / V gathered from whole tiles carry the same bytes and scales in the same tile
positions, and a q-block that walks the tiles T does the arithmetic of `ops.attention_fp8` over that gather in the same order.
The table set is the one of tests/test_attention_ranges_gpu.py.  Smooth K over a per-block table has no exact twin (the mean over
all keys is not the mean over the gathered keys): that case is held to the bounds tests/test_attention_fp8_gpu.py holds the dense
kernel to, against fp32 SDPA under the expanded block mask."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests.attn_fp8_ref import LOG2E, mxq
from tests.parity import record, rel_rms

pytestmark = pytest.mark.gpu

DEV = "cuda"
DH = 64
FINO_TUNE_ATTN_FP8_KERNEL = 5               # include/frameino_hip.h
B, HEADS, LQ, LK = 2, 3, 600, 1100          # 3 table rows, 5 workgroups of 128 rows (the last: 88 rows); 18 key tiles, 12 keys in
NQB, NT = 3, 18                             # the last; 6 head-batches: not a multiple of 8, the virtual-head block mapping


def _table(*blocks):
    """q-block rows of up to three (begin, end) pairs -> [nqb, 3, 2] int32, unused entries (0, 0)"""
    t = torch.zeros(len(blocks), 3, 2, dtype=torch.int32)
    for i, blk in enumerate(blocks):
        for j, (s, e) in enumerate(blk):
            t[i, j, 0], t[i, j, 1] = s, e
    return t


def _same(blk):
    return _table(blk, blk, blk)


# name -> table.  nt = tiles walked per q-block: 1, 2, 3, 4, 5 and 9 cover the four-slot rings and the 3-tile look-ahead
TABLES = {
    "nt1": _same([(5, 6)]),
    "nt2": _same([(3, 5)]),
    "nt3_three_single_tiles": _same([(1, 2), (7, 8), (16, 17)]),
    "nt4": _same([(2, 4), (9, 11)]),
    "nt5_first_not_at_0_last_ragged": _same([(4, 6), (10, 11), (16, 18)]),          # ends at tile 18: the 12-key tile
    "nt9": _same([(0, 3), (6, 10), (12, 14)]),
    "last_ends_at_17": _same([(0, 2), (15, 17)]),            # the last tile WALKED is full: a local-index ragged mask is wrong
    "ragged_only": _same([(17, 18)]),
    "per_block": _table([(0, 2), (17, 18)], [(3, 4), (6, 9), (11, 17)], [(1, 18)]),
    "full": _same([(0, 18)]),
}


@pytest.fixture(params=["exp2", "ramp"])
def p_mode(request):
    return request.param


def _inputs(dtype):
    d = HEADS * DH
    g = torch.Generator(device=DEV).manual_seed(1234 + DH)
    qkv = torch.randn(B, max(LQ, LK), 3 * d + 64, device=DEV, generator=g).to(dtype)      # a fused buffer: row-strided views
    return qkv[:, :LQ, :d], qkv[:, :LK, d:2 * d], qkv[:, :LK, 2 * d:3 * d]


def _clip(blk):
    out = []
    for s, e in blk:
        s = min(max(int(s), 0), NT)
        e = min(max(int(e), s), NT)
        if e > s:
            out.append((s, e))
    return out


def _gather(x, tiles):
    return torch.cat([x[:, 64 * s:min(64 * e, LK)] for s, e in tiles], dim=1)


def _expect(ops, q, k, v, table, p_mode):
    """per q-block: the dense fp8 call (default kernel) of that block's rows over the gathered K / V; zeros without tiles"""
    want = torch.empty(B, LQ, q.shape[2], dtype=q.dtype, device=DEV)
    for i in range(NQB):
        r0, r1 = 256 * i, min(256 * i + 256, LQ)
        tiles = _clip(table[i].tolist())
        if not tiles:
            want[:, r0:r1] = 0
            continue
        want[:, r0:r1] = ops.attention_fp8(q[:, r0:r1], _gather(k, tiles), _gather(v, tiles), HEADS, p_mode=p_mode)
    return want


def _run(ops, q, k, v, table, p_mode, **kw):
    out = torch.zeros(B, LQ + 5, q.shape[2], dtype=q.dtype, device=DEV)          # a view of a larger zeroed buffer
    got = ops.attention_fp8_ranges(q, k, v, HEADS, table.to(DEV), out=out[:, :LQ], p_mode=p_mode, **kw)
    assert not out[:, LQ:].any(), "rows past Lq were written"
    assert torch.isfinite(got.float()).all()
    return got


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name", sorted(TABLES))
def test_ranges_equal_the_dense_fp8_kernel_over_the_gathered_tiles(name, dtype, p_mode):
    from frameino_amd import ops
    q, k, v = _inputs(dtype)
    table = TABLES[name]
    want = _expect(ops, q, k, v, table, p_mode)
    got = _run(ops, q, k, v, table, p_mode)
    assert torch.equal(got, want), (name, (got.float() - want.float()).abs().max().item())
    if name == "full":                      # the whole K / V in one range: the dense call as it stands, with and without smooth K
        assert torch.equal(got, ops.attention_fp8(q, k, v, HEADS, p_mode=p_mode))
        assert torch.equal(_run(ops, q, k, v, table, p_mode, smooth_k=True),
                           ops.attention_fp8(q, k, v, HEADS, p_mode=p_mode, smooth_k=True))


def test_the_ranges_entry_ignores_the_fp8_kernel_knob(p_mode):
    """FINO_TUNE_ATTN_FP8_KERNEL = 1 selects the ping-pong kernel for the dense call only: the ranges launch is unchanged"""
    from frameino_amd import _lib, ops
    q, k, v = _inputs(torch.bfloat16)
    want = _run(ops, q, k, v, TABLES["per_block"], p_mode)
    before = _lib.lib().fino_tune_get(FINO_TUNE_ATTN_FP8_KERNEL)
    _lib.lib().fino_tune_set(FINO_TUNE_ATTN_FP8_KERNEL, 1)
    try:
        got = _run(ops, q, k, v, TABLES["per_block"], p_mode)
    finally:
        _lib.lib().fino_tune_set(FINO_TUNE_ATTN_FP8_KERNEL, before)
    assert torch.equal(got, want)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_a_q_block_without_tiles_stores_finite_zeros(dtype, p_mode):
    from frameino_amd import ops
    q, k, v = _inputs(dtype)
    table = _table([(2, 5)], [], [(0, 1), (17, 18)])
    got = _run(ops, q, k, v, table, p_mode)
    assert not got[:, 256:512].any()
    assert torch.equal(got, _expect(ops, q, k, v, table, p_mode))


def test_a_range_beyond_the_last_tile_is_clipped(p_mode):
    """`end` beyond ceil(lk / 64), a `begin` beyond it, a negative begin: the clipped table's result"""
    from frameino_amd import ops
    q, k, v = _inputs(torch.bfloat16)
    bad = _table([(1, 3), (15, 40)], [(-4, 2), (16, 1000)], [(3, 4), (19, 25)])
    clipped = _table([(1, 3), (15, 18)], [(0, 2), (16, 18)], [(3, 4)])
    got = _run(ops, q, k, v, bad, p_mode)
    assert torch.equal(got, _run(ops, q, k, v, clipped, p_mode))
    assert torch.equal(got, _expect(ops, q, k, v, clipped, p_mode))


def _mask(table):
    mask = torch.zeros(LQ, LK, dtype=torch.bool, device=DEV)
    for i in range(NQB):
        for s, e in _clip(table[i].tolist()):
            mask[256 * i:256 * i + 256, 64 * s:min(64 * e, LK)] = True
    return mask


def _emulated_masked_smooth(q, k, v, mask, p_mode):
    """tests/attn_fp8_ref.py::emulated with smooth_k (the mean over ALL keys) and the softmax restricted to `mask`"""
    qh, kh, vh = (t.float().view(B, -1, HEADS, DH).transpose(1, 2) for t in (q, k, v))
    kh = kh - kh.mean(2, keepdim=True)
    q8 = mxq(qh * (DH ** -0.5 * LOG2E))
    k8 = mxq(kh)
    v8 = mxq(F.pad(vh, (0, 0, 0, (-LK) % 32)), dim=2)[:, :, :LK]
    s = (q8 @ k8.transpose(2, 3)).masked_fill(~mask, float("-inf"))
    if p_mode == "ramp":
        m = torch.round(s.amax(-1, keepdim=True) - 6)
        p8 = torch.round(8 * (s - m) + 55.5).clamp(0, 126).to(torch.uint8).view(torch.float8_e4m3fn).float()
    else:
        p8 = (torch.exp2(s - s.amax(-1, keepdim=True)) * 64).to(torch.float8_e4m3fn).float() / 64
    return ((p8 @ v8) / p8.sum(-1, keepdim=True)).transpose(1, 2).reshape(B, LQ, HEADS * DH)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_smooth_k_over_a_per_block_table_against_fp32_sdpa_under_the_block_mask(dtype, p_mode):
    """the dense kernel's bounds (tests/test_attention_fp8_gpu.py): rel-RMS < 8e-2 and < 1.2 x the torch emulation of the same
    quantisation under the same mask + 2e-3; V = 1 gives 1 within 4e-3"""
    from frameino_amd import ops
    q, k, v = _inputs(dtype)
    table = TABLES["per_block"]
    mask = _mask(table)
    sp = lambda x: x.float().reshape(B, -1, HEADS, DH).transpose(1, 2)      # noqa: E731
    ref = F.scaled_dot_product_attention(sp(q), sp(k), sp(v), attn_mask=mask).transpose(1, 2).reshape(B, LQ, HEADS * DH)
    emu = _emulated_masked_smooth(q, k, v, mask, p_mode)
    got = _run(ops, q, k, v, table, p_mode, smooth_k=True)
    r, re = rel_rms(got, ref), rel_rms(emu, ref)
    print(f"smooth K, per-block table, {p_mode}, {dtype}: rel-RMS vs fp32 SDPA {r:.4e}, emulation {re:.4e}")
    record(f"attention_fp8_ranges[smooth-{p_mode}-per_block-{str(dtype)[6:]}]",
           f"rel_rms vs fp32 SDPA under the block mask (torch emulation of the quantisation: {re:.4f})", r, 8e-2)
    assert r < 8e-2 and r < 1.2 * re + 2e-3, (r, re)
    o1 = _run(ops, q, k, torch.ones_like(v), table, p_mode, smooth_k=True)       # every block of this table has tiles
    d1 = (o1.float() - 1).abs().max().item()
    print(f"V = 1: max |o - 1| = {d1:.3e}")
    record(f"attention_fp8_ranges[smooth-{p_mode}-per_block-{str(dtype)[6:]}, V = 1]", "max |o - 1|", d1, 4e-3)
    assert d1 < 4e-3


def test_folded_scale_is_as_close_to_the_plain_scale_as_the_dense_kernel_s_two_forms(p_mode):
    """scale = SCALE_FOLDED with q pre-scaled (one more rounding of q) against the plain-scale call: the distance the dense fp8
    kernel's two forms have on the same inputs, measured here, is the bound"""
    from frameino_amd import ops
    q, k, v = _inputs(torch.bfloat16)
    qs = (q.float() * (DH ** -0.5 * LOG2E)).to(q.dtype)
    dense = rel_rms(ops.attention_fp8(qs, k, v, HEADS, scale=ops.SCALE_FOLDED, p_mode=p_mode),
                    ops.attention_fp8(q, k, v, HEADS, p_mode=p_mode))
    table = TABLES["full"]
    full = rel_rms(_run(ops, qs, k, v, table, p_mode, scale=ops.SCALE_FOLDED), _run(ops, q, k, v, table, p_mode))
    print(f"folded vs plain scale, {p_mode}: dense {dense:.4e}, ranges over the full table {full:.4e}")
    # (the full-table launch is bit-equal to the dense call, so this holds with equality: it pins that the folded scale takes the
    # same route through the ranges entry.  What bounds the SPARSE case is the exact twin below.)
    assert full <= dense
    # a sparse table: the same rounding of q over fewer keys -- every q-block torch.equal to the dense folded-scale call over its
    # gathered tiles, whose distance to the plain-scale form is the one measured above
    table = TABLES["per_block"]
    got = _run(ops, qs, k, v, table, p_mode, scale=ops.SCALE_FOLDED)
    want = torch.empty_like(got)
    for i in range(NQB):
        r0, r1 = 256 * i, min(256 * i + 256, LQ)
        tiles = _clip(table[i].tolist())
        want[:, r0:r1] = ops.attention_fp8(qs[:, r0:r1], _gather(k, tiles), _gather(v, tiles), HEADS, scale=ops.SCALE_FOLDED,
                                           p_mode=p_mode)
    assert torch.equal(got, want)


def test_argument_checks():
    from frameino_amd import _lib, ops
    q, k, v = _inputs(torch.bfloat16)
    assert ops.attention_fp8_ranges_supported(B, HEADS, LQ, LK, 64)
    assert not ops.attention_fp8_ranges_supported(B, HEADS, LQ, LK, 128)
    assert not ops.attention_fp8_ranges_supported(B, HEADS, LQ, LK, 96)
    with pytest.raises(AssertionError, match="ranges"):
        ops.attention_fp8_ranges(q, k, v, HEADS, TABLES["full"][:2].to(DEV))        # two q-blocks' rows for three q-blocks
    with pytest.raises(AssertionError, match="ranges"):
        ops.attention_fp8_ranges(q, k, v, HEADS, TABLES["full"].to(DEV).long())
    with pytest.raises(AssertionError, match="ranges"):
        ops.attention_fp8_ranges(q, k, v, HEADS, TABLES["full"])                     # a host table
    lib = _lib.lib()
    args = (16, 16, 16, 16, 1, 1, 8, 8)
    tail = (*([8] * 8), ctypes.c_float(1.0), 0, 0, 16, 1 << 20, 0)
    rc = lib.fino_attn_fwd_fp8_ranges(*args, 64, *tail, 0, 0)
    assert rc == -1 and b"ranges" in lib.fino_last_error()
    rc = lib.fino_attn_fwd_fp8_ranges(*args, 128, *tail, 16, 0)
    assert rc == -3 and b"head_dim" in lib.fino_last_error()
