"""fino_attn_fwd_tiles (csrc/fino_attention.hip, attn_ppd_kernel<T, D, 3>): attention in which every (batch element, head,
256-row q-block) walks the 64-key tiles named by a bitmask.

The expected result is EXACT, as in tests/test_attention_ranges_gpu.py: a q-block that walks the tiles T does the arithmetic of
the dense attn_ppd_kernel over K / V gathered from T, in the same order -- here per head and batch element, so the expectation
is that head's column slice run with heads = 1 (forced onto attn_ppd_kernel, whole blocks: FINO_TUNE_ATTN_KERNEL = 4, no tail
split).  Shape, generator and the forcing are that file's."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests.sparse_attn_ref import expand_mask, pack_mask, unpack_mask
from tests.test_attention_ranges_gpu import B, HEADS, LK, LQ, NQB, NT, TABLES, _ForcedDense, _inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"

# one tile set per (batch element, head, q-block), all different: popcounts 1, 2, 3, 4, 5 and 9 (the four-slot rings and the
# 3 - 4-tile look-ahead), scattered single tiles, a set whose last walked tile is the ragged tile 17, one whose last walked tile
# is full while tile 17 is not set, only the ragged tile, all tiles
SETS = [
    [5], [3, 11], [1, 7, 16],                                    # b 0, h 0
    [2, 6, 9, 13], [4, 5, 10, 16, 17], [0, 1, 2, 6, 8, 9, 12, 13, 15],      # b 0, h 1
    [0, 1, 15, 16], [17], list(range(18)),                       # b 0, h 2
    [0, 17], [1, 2, 3, 4, 5, 6, 7, 8, 17], [16],                 # b 1, h 0
    list(range(0, 18, 2)), [3, 4], [15, 16, 17],                 # b 1, h 1
    [8], [2, 9, 10, 11, 12], [0, 5, 9, 14],                      # b 1, h 2
]


def _keep(sets=SETS):
    keep = torch.zeros(B, HEADS, NQB, NT, dtype=torch.bool)
    for j, s in enumerate(sets):
        keep.view(-1, NT)[j, s] = True
    return keep


def _gather(x, tiles):
    return torch.cat([x[:, 64 * t:min(64 * t + 64, LK)] for t in tiles], dim=1)


def _expect(ops, q, k, v, keep, dh):
    """per (b, h, q-block): the forced-dense call, heads = 1, of that head's columns over the gathered K / V (zeros: no tiles)"""
    want = torch.empty(B, LQ, q.shape[2], dtype=q.dtype, device=DEV)
    for b in range(B):
        for h in range(HEADS):
            c = slice(h * dh, (h + 1) * dh)
            for i in range(NQB):
                r0, r1 = 256 * i, min(256 * i + 256, LQ)
                tiles = keep[b, h, i].nonzero().flatten().tolist()
                if not tiles:
                    want[b, r0:r1, c] = 0
                    continue
                want[b:b + 1, r0:r1, c] = ops.attention(q[b:b + 1, r0:r1, c], _gather(k[b:b + 1, :, c], tiles),
                                                        _gather(v[b:b + 1, :, c], tiles), 1)
    return want


def _run(ops, q, k, v, mask):
    out = torch.zeros(B, LQ + 5, q.shape[2], dtype=q.dtype, device=DEV)          # a view of a larger zeroed buffer
    got = ops.attention_tiles(q, k, v, HEADS, mask.to(DEV), out=out[:, :LQ])
    assert not out[:, LQ:].any(), "rows past Lq were written"
    assert torch.isfinite(got.float()).all()
    return got


def test_the_masks_are_the_ones_the_issue_asks_for():
    keep = _keep()
    assert sorted({len(s) for s in SETS}) == [1, 2, 3, 4, 5, 9, 18] and len({tuple(s) for s in SETS}) == B * HEADS * NQB
    assert [17] in SETS and any(s[-1] == 17 and len(s) > 1 for s in SETS) and any(s[-1] == 16 for s in SETS)
    assert torch.equal(unpack_mask(pack_mask(keep), NT), keep) and LK - 64 * (NT - 1) == 12


@pytest.mark.parametrize("dh", [128, 64])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_tiles_equal_the_dense_kernel_over_the_gathered_tiles(dtype, dh):
    q, k, v = _inputs(dtype, dh)
    keep = _keep()
    with _ForcedDense() as ops:
        want = _expect(ops, q, k, v, keep, dh)
    from frameino_amd import ops
    got = _run(ops, q, k, v, pack_mask(keep))
    assert torch.equal(got, want), (got.float() - want.float()).abs().max().item()
    # bits at or beyond tile 18 are ignored (and a second word is allowed)
    junk = pack_mask(torch.cat([keep, torch.ones(B, HEADS, NQB, 64 - NT, dtype=torch.bool)], dim=-1))
    assert junk.shape[-1] == 2 and torch.equal(_run(ops, q, k, v, junk), want)
    # an empty row gives finite zeros, the other rows what they gave
    holed = keep.clone()
    holed[1, 2, 1] = False
    got = _run(ops, q, k, v, pack_mask(holed))
    assert not got[1, 256:512, 2 * dh:].any()
    got[1, 256:512, 2 * dh:] = want[1, 256:512, 2 * dh:]
    assert torch.equal(got, want)


@pytest.mark.parametrize("dh", [128, 64])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_a_full_mask_is_the_dense_attention_and_a_shared_mask_the_range_walk(dtype, dh):
    from frameino_amd import ops
    q, k, v = _inputs(dtype, dh)
    with _ForcedDense() as fops:
        dense = fops.attention(q, k, v, HEADS)
    full = pack_mask(torch.ones(B, HEADS, NQB, NT, dtype=torch.bool))
    assert torch.equal(_run(ops, q, k, v, full), dense)
    for name, table in sorted(TABLES.items()):                  # one mask row per q-block, strides 0 over heads and batch
        keep = torch.zeros(1, 1, NQB, NT, dtype=torch.bool)
        for i, blk in enumerate(table.tolist()):
            for a, b in blk:
                keep[0, 0, i, max(a, 0):max(b, 0)] = True
        want = ops.attention_ranges(q, k, v, HEADS, table.to(DEV))
        assert torch.equal(_run(ops, q, k, v, pack_mask(keep)), want), name
        per_head = pack_mask(keep.expand(1, HEADS, NQB, NT))    # ... and [1, heads]: shared over the batch only
        assert torch.equal(_run(ops, q, k, v, per_head), want), name


def test_tiles_against_fp32_sdpa_with_the_expanded_mask():
    """the bound of tests/test_attention_ranges_gpu.py: P is rounded to the operand type before P.V, 4 ulp rel-RMS"""
    from frameino_amd import ops
    dh, dtype = 128, torch.bfloat16
    q, k, v = _inputs(dtype, dh)
    keep = _keep()
    mask = expand_mask(keep, LQ, LK).to(DEV)
    sp = lambda x: x.float().reshape(B, -1, HEADS, dh).transpose(1, 2)      # noqa: E731
    ref = F.scaled_dot_product_attention(sp(q), sp(k), sp(v), attn_mask=mask).transpose(1, 2).reshape(B, LQ, HEADS * dh)
    got = _run(ops, q, k, v, pack_mask(keep)).float()
    eps = 2.0 ** -8
    rel = ((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()
    print(f"rel-RMS vs fp32 SDPA (head_dim {dh}, {dtype}): {rel:.3e} (bound {4 * eps:.3e})")
    assert rel < 4 * eps, rel


def test_argument_checks():
    from frameino_amd import _lib, ops
    q, k, v = _inputs(torch.bfloat16, 128)
    assert ops.attention_tiles_supported(B, HEADS, LQ, LK, 128) and ops.attention_tiles_supported(B, HEADS, LQ, LK, 64)
    assert not ops.attention_tiles_supported(B, HEADS, LQ, LK, 96)
    assert ops.attention_tiles_supported(1, 1, 256, 65536, 128) and not ops.attention_tiles_supported(1, 1, 256, 65537, 128)
    good = pack_mask(_keep())
    with pytest.raises(ValueError, match="mask"):
        ops.attention_tiles(q, k, v, HEADS, good[:, :, :2].contiguous().to(DEV))         # two q-blocks' rows for three
    with pytest.raises(ValueError, match="mask"):
        ops.attention_tiles(q, k, v, HEADS, good.to(DEV).long())
    with pytest.raises(ValueError, match="mask"):
        ops.attention_tiles(q, k, v, HEADS, good)                                        # a host tensor
    with pytest.raises(ValueError, match="mask"):
        ops.attention_tiles(q, k, v, HEADS, good[:, :, :, :0].contiguous().to(DEV))       # no words at all
    lib = _lib.lib()
    f1 = ctypes.c_float(1.0)
    rc = lib.fino_attn_fwd_tiles(16, 16, 16, 16, 1, 1, 8, 8, 128, *([8] * 12), f1, 0, 0, 0, 0, 1, 0)
    assert rc == -1 and b"mask" in lib.fino_last_error()
    rc = lib.fino_attn_fwd_tiles(16, 16, 16, 16, 1, 1, 8, 64 * 33, 128, *([8] * 12), f1, 0, 16, 0, 0, 1, 0)
    assert rc == -1 and b"mask words" in lib.fino_last_error()                           # 33 tiles need two words
    rc = lib.fino_attn_fwd_tiles(16, 16, 16, 16, 1, 1, 8, 8, 96, *([8] * 12), f1, 0, 16, 0, 0, 1, 0)
    assert rc == -3 and b"head_dim" in lib.fino_last_error()
    rc = lib.fino_attn_fwd_tiles(16, 16, 16, 16, 1, 1, 8, 65537, 128, *([8] * 12), f1, 0, 16, 0, 0, 4096, 0)
    assert rc == -3 and b"key tiles" in lib.fino_last_error()
