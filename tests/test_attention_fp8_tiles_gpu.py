"""fino_attn_fwd_fp8_tiles (csrc/fino_attention_fp8.hip: attn_fp8_d128_kernel<T, PX, true>): the fp8
attention of head_dim 128 over the key tiles a bitmask names per (batch element, head, 256-row q-block).

B = 2, heads = 3, LQ = 600, LK = 1100: three q-blocks (the last with 88 rows), 18 key tiles, 12 keys in the last.  One tile set per
(batch element, head, q-block), all different, of 1, 2, 3, 4, 5, 8, 9 and 15 tiles: the eight-slot ring wraps, the four-tile
look-ahead runs past the list, the ragged tile 17 is walked last, is left out, and is walked alone.

  * exact: a q-block that walks T is torch.equal to ops.attention_fp8 of its rows with heads = 1 on that head's columns over K / V
    gathered from the whole tiles of T (K is quantised per key, V per 32 keys inside a tile: whole gathered tiles carry the same
    bytes and scales in the same order).  Only while that reference call is not tail-split: a one-block call stays whole below 16
    key tiles, which is why no set exceeds 15 and why fino_attn_workspace_bytes(1, 1, 256, gathered keys, 128) == 0 is asserted;
  * stride-0 masks (rows shared over heads, over batch elements) equal the expanded mask's result;
  * what has no exact twin -- the full mask (the dense call is tail-split there) and smooth K / smooth V on partial masks -- is
    held against fp32 SDPA under the expanded block mask to the bounds tests/test_attention_fp8_gpu.py holds the dense kernel to
    (rel-RMS < 8e-2 and < 1.2 x the torch emulation of the quantisation + 2e-3; that file states them as literals);
  * smooth V: values with an 8 sigma offset per channel stay within 1.2 x the smoothed emulation, the recipe and the check of
    tests/test_attention_fp8_smooth_v_gpu.py;
  * empty rows store finite zeros (not the value mean), bits at or beyond tile 18 are ignored, rows past LQ of a larger output stay
    untouched, two launches give the same bits, argument errors raise from ops."""
import functools

import pytest
import torch

from frameino_amd.window_attention import pack_tile_mask
from tests.attn_fp8_smooth_v_ref import emulated, offset_v_inputs, sdpa_masked
from tests.parity import record, rel_rms
from tests.sparse_attn_ref import expand_mask
from tests.test_attention_fp8_smooth_v_gpu import _offset_check

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, HEADS, LQ, LK, DH = 2, 3, 600, 1100, 128
NQB, NT = 3, 18
D = HEADS * DH
POPCOUNTS = (1, 2, 3, 4, 5, 8, 9, 15)
# the bounds of tests/test_attention_fp8_gpu.py::test_fp8_attention_vs_fp32_and_vs_the_emulated_quantisation
FP32_BOUND, EMU_FACTOR, EMU_TERM = 8e-2, 1.2, 2e-3
dtypes = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
p_modes = pytest.mark.parametrize("p_mode", ["exp2", "ramp"])


@functools.lru_cache(None)
def tile_sets():
    """bool [B, HEADS, NQB, NT]: row i = (b, h, qb) flattened walks POPCOUNTS[i % 8] tiles.  Row 0 walks tile 17 alone, rows 8 and
    16 one scattered tile each; of the others the odd rows end on the ragged tile 17 and the even rows leave it out."""
    g = torch.Generator().manual_seed(18)
    keep = torch.zeros(B * HEADS * NQB, NT, dtype=torch.bool)
    for i in range(keep.shape[0]):
        n = POPCOUNTS[i % 8]
        if n == 1:
            keep[i, {0: NT - 1, 8: 5, 16: 11}[i]] = True
        elif i % 2:
            keep[i, torch.randperm(NT - 1, generator=g)[:n - 1]] = True
            keep[i, NT - 1] = True
        else:
            keep[i, torch.randperm(NT - 1, generator=g)[:n]] = True
        assert int(keep[i].sum()) == n
    assert len({tuple(r) for r in keep.tolist()}) == keep.shape[0]                                   # all different
    assert sorted(set(keep.sum(1).tolist())) == list(POPCOUNTS)
    last = [max(t for t in range(NT) if r[t]) for r in keep.tolist()]
    assert any(x == NT - 1 and n > 1 for x, n in zip(last, keep.sum(1).tolist()))                   # ... ends on the ragged tile
    assert any(x < NT - 1 and n > 1 for x, n in zip(last, keep.sum(1).tolist()))                    # ... ends on a full tile
    assert keep[0].tolist() == [False] * (NT - 1) + [True]                                           # ... tile 17 alone
    assert int(keep[8].sum()) == 1 and int(keep[16].sum()) == 1 and not keep[8, NT - 1]              # ... scattered single tiles
    return keep.view(B, HEADS, NQB, NT)


def _mask(keep):
    return pack_tile_mask(keep).to(DEV)


@functools.lru_cache(None)
def inputs(dtype):
    """q and row-strided k | v views of one buffer, N(0, 1), seeded on the CPU"""
    g = torch.Generator().manual_seed(1100)
    q = torch.randn(B, LQ, D, generator=g).to(dtype).to(DEV)
    kv = torch.randn(B, LK, 2 * D + 64, generator=g).to(dtype).to(DEV)
    return q, kv[:, :, :D], kv[:, :, D:2 * D]


@functools.lru_cache(None)
def masked_refs(dtype, p_mode, smooth_k, smooth_v, full):
    """(fp32 SDPA, the emulation of the quantisation) under the expanded block mask of tile_sets() -- or of the full mask"""
    q, k, v = inputs(dtype)
    keep = torch.ones(B, HEADS, NQB, NT, dtype=torch.bool) if full else tile_sets()
    big = expand_mask(keep, LQ, LK).to(DEV)
    return sdpa_masked(q, k, v, HEADS, big), emulated(q, k, v, HEADS, p_mode, smooth_k=smooth_k, smooth_v=smooth_v, mask=big)


def _gathered(t, bi, h, tiles):
    return torch.cat([t[bi:bi + 1, 64 * j:min(64 * j + 64, LK), DH * h:DH * (h + 1)] for j in tiles], 1).contiguous()


@dtypes
@p_modes
def test_a_q_block_equals_the_dense_call_over_its_gathered_tiles(dtype, p_mode):
    from frameino_amd import _lib, ops
    assert ops.attention_fp8_tiles_supported(B, HEADS, LQ, LK, DH) and not ops.attention_fp8_tiles_supported(B, HEADS, LQ, LK, 64)
    q, k, v = inputs(dtype)
    keep = tile_sets()
    out = torch.full((B, LQ + 5, D), 3.0, device=DEV, dtype=dtype)
    got = ops.attention_fp8_tiles(q, k, v, HEADS, _mask(keep), out=out[:, :LQ], p_mode=p_mode)
    assert got.data_ptr() == out.data_ptr() and (out[:, LQ:] == 3.0).all() and torch.isfinite(got.float()).all()
    bad = []
    for bi in range(B):
        for h in range(HEADS):
            for qb in range(NQB):
                tiles = [t for t in range(NT) if keep[bi, h, qb, t]]
                kg, vg = _gathered(k, bi, h, tiles), _gathered(v, bi, h, tiles)
                # the twin is exact only while the reference call is not tail-split
                assert _lib.lib().fino_attn_workspace_bytes(1, 1, 256, kg.shape[1], DH) == 0, tiles
                rows = slice(256 * qb, min(256 * qb + 256, LQ))
                want = ops.attention_fp8(q[bi:bi + 1, rows, DH * h:DH * (h + 1)], kg, vg, 1, p_mode=p_mode)
                if not torch.equal(got[bi:bi + 1, rows, DH * h:DH * (h + 1)], want):
                    bad.append((bi, h, qb, tiles, rel_rms(got[bi:bi + 1, rows, DH * h:DH * (h + 1)], want)))
    assert not bad, bad
    assert torch.equal(ops.attention_fp8_tiles(q, k, v, HEADS, _mask(keep), p_mode=p_mode), got)    # launched twice: the same bits


@dtypes
def test_stride_0_masks_share_their_rows(dtype):
    from frameino_amd import ops
    q, k, v = inputs(dtype)
    keep = tile_sets()
    for shared in (keep[:, :1], keep[:1], keep[:1, :1]):                 # over heads, over batch elements, over both
        want = ops.attention_fp8_tiles(q, k, v, HEADS, _mask(shared.expand(B, HEADS, NQB, NT).contiguous()))
        assert torch.equal(ops.attention_fp8_tiles(q, k, v, HEADS, _mask(shared.contiguous())), want), tuple(shared.shape)


@dtypes
@p_modes
@pytest.mark.parametrize("case", ["full", "smooth_k", "smooth_v", "smooth_k_v"])
def test_the_full_mask_and_the_smooth_flags_vs_fp32_under_the_block_mask(dtype, p_mode, case):
    from frameino_amd import ops
    q, k, v = inputs(dtype)
    full = case == "full"
    smooth_k, smooth_v = "k" in case.split("_")[1:], "v" in case.split("_")[1:]
    keep = torch.ones(B, HEADS, NQB, NT, dtype=torch.bool) if full else tile_sets()
    got = ops.attention_fp8_tiles(q, k, v, HEADS, _mask(keep), p_mode=p_mode, smooth_k=smooth_k, smooth_v=smooth_v)
    ref, emu = masked_refs(dtype, p_mode, smooth_k, smooth_v, full)
    r, re = rel_rms(got, ref), rel_rms(emu, ref)
    print(f"fp8 tiles [{case}, {p_mode}, {dtype}]: rel-RMS {r:.4f} against fp32 SDPA under the block mask, emulation {re:.4f}")
    record(f"attention_fp8_tiles[{case}-{p_mode}-{str(dtype)[6:]}]", f"rel_rms vs masked fp32 SDPA (torch emulation: {re:.4f})", r,
           FP32_BOUND)
    assert torch.isfinite(got.float()).all() and r < FP32_BOUND and r < EMU_FACTOR * re + EMU_TERM, (r, re)
    if not full:
        plain = ops.attention_fp8_tiles(q, k, v, HEADS, _mask(keep), p_mode=p_mode)
        assert not torch.equal(got, plain)                               # the flags reach the kernel's pre-pass


@dtypes
@p_modes
def test_smooth_v_keeps_an_8_sigma_value_offset_out_of_the_error(dtype, p_mode):
    from frameino_amd import ops
    q, k, v = offset_v_inputs(B, HEADS, LQ, LK, DH, dtype, DEV)
    keep = tile_sets()
    big, mask = expand_mask(keep, LQ, LK).to(DEV), _mask(keep)
    _offset_check(f"attention_fp8_tiles_smooth_v_offset_values[{p_mode}-{str(dtype)[6:]}]", dtype,
                  sdpa_masked(q, k, v, HEADS, big), emulated(q, k, v, HEADS, p_mode, smooth_v=True, mask=big),
                  emulated(q, k, v, HEADS, p_mode, mask=big),
                  ops.attention_fp8_tiles(q, k, v, HEADS, mask, p_mode=p_mode, smooth_v=True),
                  ops.attention_fp8_tiles(q, k, v, HEADS, mask, p_mode=p_mode))


@dtypes
@pytest.mark.parametrize("smooth_v", [False, True], ids=["plain", "smooth-v"])
def test_empty_rows_store_zeros_and_bits_past_the_last_tile_are_ignored(dtype, smooth_v):
    from frameino_amd import ops
    q, k, v = inputs(dtype)
    keep = tile_sets().clone()
    keep[0, 1, 1] = False                                                # one empty row in the middle, one at the ragged q-block
    keep[1, 2, 2] = False
    words = pack_tile_mask(keep)
    out = torch.full((B, LQ + 5, D), float("nan"), device=DEV, dtype=dtype)
    got = ops.attention_fp8_tiles(q, k, v, HEADS, words.to(DEV), out=out[:, :LQ], smooth_v=smooth_v)
    assert torch.isfinite(got.float()).all() and torch.isnan(out[:, LQ:].float()).all()
    assert not got[0, 256:512, DH:2 * DH].any() and not got[1, 512:, 2 * DH:].any()                  # zeros, not the value mean
    assert got[0, :256, DH:2 * DH].any() and got[1, 512:, :2 * DH].any() and got[0, 256:512, :DH].any()
    # bits 18 .. 31 set in every row (the empty ones included), and a second word of ones: the same bits out
    junk = torch.stack([words[..., 0] | (-1 << NT), torch.full_like(words[..., 0], -1)], -1).contiguous()
    assert torch.equal(ops.attention_fp8_tiles(q, k, v, HEADS, junk.to(DEV), smooth_v=smooth_v), got)


def test_argument_errors_raise_from_ops():
    from frameino_amd import ops
    q, k, v = inputs(torch.bfloat16)
    mask = _mask(tile_sets())
    with pytest.raises(ValueError, match="mask"):
        ops.attention_fp8_tiles(q, k, v, HEADS, mask.float())
    with pytest.raises(ValueError, match="mask"):
        ops.attention_fp8_tiles(q, k, v, HEADS, mask[:, :, :2].contiguous())
    with pytest.raises(ValueError, match="mask"):
        ops.attention_fp8_tiles(q, k, v, HEADS, mask.cpu())
    with pytest.raises(ValueError, match="mask"):
        ops.attention_fp8_tiles(q, k, v, HEADS, mask[..., :0].contiguous())
    with pytest.raises(RuntimeError, match="head_dim 64"):
        ops.attention_fp8_tiles(q, k, v, 2 * HEADS, mask.repeat(1, 2, 1, 1).contiguous())
