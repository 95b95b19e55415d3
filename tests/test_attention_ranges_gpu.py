"""fino_attn_fwd_ranges (csrc/fino_attention.hip, attn_ppd_kernel<T, D, 2>): attention in which every 256-row q-block walks up
to three ranges of 64-key tiles taken from a device table.

The expected result is EXACT.  A q-block that walks the tiles T does the same arithmetic, in the same order, as the dense
attn_ppd_kernel over K / V gathered from T (torch.cat of the tile-aligned slices): local tile t of the walk holds the keys of
gathered tile t, the ring slots and the softmax order go by t, and the ragged last tile is masked at the same keys.  So the
rows of every q-block must be torch.equal to that dense call's (forced onto attn_ppd_kernel, whole blocks: FINO_TUNE_ATTN_KERNEL
= 4, no tail split).  One case is also held against fp32 SDPA under the expanded boolean block mask: the semantics, by a route
that shares nothing with the kernel."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, HEADS, LQ, LK = 2, 3, 600, 1100          # 3 q-blocks (the last: 88 rows); 18 key tiles, 12 keys in the last; 6 head-batches:
NQB, NT = 3, 18                             # not a multiple of 8, the virtual-head block mapping


def _table(*blocks):
    """q-block rows of up to three (begin, end) pairs -> [nqb, 3, 2] int32, unused entries (0, 0)"""
    t = torch.zeros(len(blocks), 3, 2, dtype=torch.int32)
    for i, blk in enumerate(blocks):
        for j, (s, e) in enumerate(blk):
            t[i, j, 0], t[i, j, 1] = s, e
    return t


def _same(blk):
    return _table(blk, blk, blk)


# name -> table.  nt = tiles walked per q-block: 1, 2, 3, 4, 5 and 9 cover the four-slot rings and the 3 - 4-tile look-ahead
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


def _inputs(dtype, dh):
    d = HEADS * dh
    g = torch.Generator(device=DEV).manual_seed(1234 + dh)
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


class _ForcedDense:
    """the dense call on attn_ppd_kernel, whole blocks (tests/test_kernels_gpu.py does the same)"""

    def __enter__(self):
        from frameino_amd import _lib, ops
        self.lib, self.ops, self.split = _lib.lib(), ops, ops.SPLIT_ATTENTION_TAIL
        self.lib.fino_tune_set(4, 4)
        ops.SPLIT_ATTENTION_TAIL = False
        return ops

    def __exit__(self, *exc):
        self.lib.fino_tune_set(4, 0)
        self.ops.SPLIT_ATTENTION_TAIL = self.split


def _expect(ops, q, k, v, table):
    """per q-block: the forced-dense call of that block's rows over the gathered K / V (zeros for a block without tiles)"""
    want = torch.empty(B, LQ, q.shape[2], dtype=q.dtype, device=DEV)
    for i in range(NQB):
        r0, r1 = 256 * i, min(256 * i + 256, LQ)
        tiles = _clip(table[i].tolist())
        if not tiles:
            want[:, r0:r1] = 0
            continue
        want[:, r0:r1] = ops.attention(q[:, r0:r1], _gather(k, tiles), _gather(v, tiles), HEADS)
    return want


def _run(ops, q, k, v, table):
    out = torch.zeros(B, LQ + 5, q.shape[2], dtype=q.dtype, device=DEV)          # a view of a larger zeroed buffer
    got = ops.attention_ranges(q, k, v, HEADS, table.to(DEV), out=out[:, :LQ])
    assert not out[:, LQ:].any(), "rows past Lq were written"
    assert torch.isfinite(got.float()).all()
    return got


@pytest.mark.parametrize("dh", [128, 64])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name", sorted(TABLES))
def test_ranges_equal_the_dense_kernel_over_the_gathered_tiles(name, dtype, dh):
    q, k, v = _inputs(dtype, dh)
    table = TABLES[name]
    with _ForcedDense() as ops:
        want = _expect(ops, q, k, v, table)
        if name == "full":                  # the whole K / V in one range: the dense call as it stands, no gather
            assert torch.equal(want, ops.attention(q, k, v, HEADS))
    from frameino_amd import ops
    got = _run(ops, q, k, v, table)
    assert torch.equal(got, want), (name, (got.float() - want.float()).abs().max().item())


@pytest.mark.parametrize("dh", [128, 64])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_a_q_block_without_tiles_stores_finite_zeros(dtype, dh):
    q, k, v = _inputs(dtype, dh)
    table = _table([(2, 5)], [], [(0, 1), (17, 18)])
    with _ForcedDense() as ops:
        want = _expect(ops, q, k, v, table)
    from frameino_amd import ops
    got = _run(ops, q, k, v, table)
    assert not got[:, 256:512].any()
    assert torch.equal(got, want)


@pytest.mark.parametrize("dh", [128, 64])
def test_a_range_beyond_the_last_tile_is_clipped(dh):
    """`end` beyond ceil(lk / 64), a `begin` beyond it, a negative begin: the clipped table's result, nothing read past K / V"""
    q, k, v = _inputs(torch.bfloat16, dh)
    from frameino_amd import ops
    bad = _table([(1, 3), (15, 40)], [(-4, 2), (16, 1000)], [(3, 4), (19, 25)])
    clipped = _table([(1, 3), (15, 18)], [(0, 2), (16, 18)], [(3, 4)])
    assert torch.equal(_run(ops, q, k, v, bad), _run(ops, q, k, v, clipped))
    with _ForcedDense() as fops:
        want = _expect(fops, q, k, v, clipped)
    assert torch.equal(_run(ops, q, k, v, bad), want)


@pytest.mark.parametrize("dh,dtype", [(128, torch.bfloat16), (64, torch.float16)])
def test_ranges_against_fp32_sdpa_with_the_expanded_block_mask(dh, dtype):
    """the bound of tests/test_kernels_gpu.py::test_attention_vs_fp32_sdpa: P is rounded to the operand type before P.V, 4 ulp
    rel-RMS"""
    from frameino_amd import ops
    q, k, v = _inputs(dtype, dh)
    table = TABLES["per_block"]
    mask = torch.zeros(LQ, LK, dtype=torch.bool, device=DEV)
    for i in range(NQB):
        for s, e in _clip(table[i].tolist()):
            mask[256 * i:256 * i + 256, 64 * s:min(64 * e, LK)] = True
    sp = lambda x: x.float().reshape(B, -1, HEADS, dh).transpose(1, 2)      # noqa: E731
    ref = F.scaled_dot_product_attention(sp(q), sp(k), sp(v), attn_mask=mask).transpose(1, 2).reshape(B, LQ, HEADS * dh)
    got = _run(ops, q, k, v, table).float()
    eps = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    rel = ((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()
    print(f"rel-RMS vs fp32 SDPA (head_dim {dh}, {dtype}): {rel:.3e} (bound {4 * eps:.3e})")
    assert rel < 4 * eps, rel


def test_argument_checks():
    from frameino_amd import _lib, ops
    q, k, v = _inputs(torch.bfloat16, 128)
    assert ops.attention_ranges_supported(B, HEADS, LQ, LK, 128) and ops.attention_ranges_supported(B, HEADS, LQ, LK, 64)
    assert not ops.attention_ranges_supported(B, HEADS, LQ, LK, 96)
    with pytest.raises(AssertionError, match="ranges"):
        ops.attention_ranges(q, k, v, HEADS, TABLES["full"][:2].to(DEV))            # two q-blocks' rows for three q-blocks
    with pytest.raises(AssertionError, match="ranges"):
        ops.attention_ranges(q, k, v, HEADS, TABLES["full"].to(DEV).long())
    import ctypes
    rc = _lib.lib().fino_attn_fwd_ranges(16, 16, 16, 16, 1, 1, 8, 8, 128, *([8] * 12), ctypes.c_float(1.0), 0, 0, 0)
    assert rc == -1 and b"ranges" in _lib.lib().fino_last_error()
    rc = _lib.lib().fino_attn_fwd_ranges(16, 16, 16, 16, 1, 1, 8, 8, 96, *([8] * 12), ctypes.c_float(1.0), 0, 16, 0)
    assert rc == -3 and b"head_dim" in _lib.lib().fino_last_error()
