"""fino_attn_tile_plan (csrc/fino_attention_plan.hip, `ops.attention_tile_plan`): the device-side predictor of the dynamic
block-sparse self-attention, against the float64 restatement in tests/sparse_attn_ref.py.

The GPU sums in fp32, the reference in float64, so a tile whose mass sits within rounding of the threshold may fall either way:
the assertions are the five properties below with the margin delta = eps = 1e-3 -- derived, not measured: an fp32 sum of <= 1024
terms is off by <= 1024 x 2^-24 = 6.1e-5 relative, the margin leaves a factor of 16 over that.

Inputs: the generator of tests/test_attention_ranges_gpu.py (seed 1234 + dh) with structure added, so that the pooled softmax is
neither uniform nor one-hot: a unit direction u per (b, h) scaled to norm sqrt(dh); K tile t gets + 0.5 c[b, t, h] u, c ~ N(0, 1);
every q row gets + 0.5 u.  Forced tiles of q-block i: {0} and [4 i, 4 i + 4).  test_the_inputs_are_not_vacuous (CPU only) holds
the inputs to what makes the properties bite."""
import pytest
import torch

from tests import sparse_attn_ref as R

B, HEADS, LQ, LK = 2, 3, 600, 1100
NQB, NT = 3, 18
DELTA = EPS = 1e-3
CDFS = (0.5, 0.9)
KEEP = torch.tensor([[[0, 1], [4 * i, 4 * i + 4], [0, 0]] if i else [[0, 4], [0, 0], [0, 0]] for i in range(NQB)], dtype=torch.int32)


def _inputs(dtype, dh, device="cpu"):
    """(q, k) on the CPU in `dtype`: row-strided views of a fused buffer, as the model's are"""
    d = HEADS * dh
    g = torch.Generator().manual_seed(1234 + dh)
    qkv = torch.randn(B, max(LQ, LK), 3 * d + 64, generator=g)
    u = torch.randn(B, HEADS, dh, generator=g)
    u = u / u.norm(dim=-1, keepdim=True) * dh ** 0.5
    c = torch.randn(B, NT, HEADS, generator=g)
    kadd = (0.5 * c[..., None] * u[:, None]).repeat_interleave(64, dim=1)[:, :LK].reshape(B, LK, d)
    qkv[:, :LK, d:2 * d] += kadd
    qkv[:, :LQ, :d] += (0.5 * u).reshape(B, 1, d)
    # 64 further rows behind the last key, far from zero: a pool that read the ragged tile's 64 rows would pick them up
    qkv = torch.cat([qkv, torch.full((B, 64, qkv.shape[2]), 3.0)], dim=1).to(dtype).to(device)
    return qkv[:, :LQ, :d], qkv[:, :LK, d:2 * d]


def _properties(keep, p, forced, cdf, what):
    """the five properties of a kept set `keep` [B, H, nqb, nt] against the float64 p; -> how many rows each one bit on"""
    bit = {"mass": 0, "order": 0, "minimal": 0, "forced_only": 0}
    for b in range(p.shape[0]):
        for h in range(p.shape[1]):
            for i in range(p.shape[2]):
                kp, pr, f = keep[b, h, i], p[b, h, i], forced[i]
                tag = (what, b, h, i, kp.nonzero().flatten().tolist())
                assert bool(kp[f].all()), ("a forced tile was dropped",) + tag                                    # 1
                mass, m_f = float(pr[kp].sum()), float(pr[f].sum())
                assert mass >= cdf - DELTA, ("kept mass", mass) + tag                                             # 2
                bit["mass"] += 1
                extra, dropped = kp & ~f, ~kp
                if extra.any() and dropped.any():                                                                 # 3
                    assert float(pr[extra].min()) >= (1 - EPS) * float(pr[dropped].max()), ("order",) + tag
                    bit["order"] += 1
                if m_f < cdf - DELTA and extra.any():                                                             # 4
                    assert mass - float(pr[extra].min()) < cdf + DELTA, ("not minimal", mass) + tag
                    bit["minimal"] += 1
                if m_f >= cdf + DELTA:                                                                            # 5
                    assert not extra.any(), ("more than the forced tiles",) + tag
                    bit["forced_only"] += 1
    return bit


def test_the_inputs_are_not_vacuous():
    """a condition on the INPUTS (CPU, float64 reference alone): no row keeps everything or only its forced tiles everywhere,
    the kept sets at cdf +- 1e-3 differ in under 1 % of the entries, and the reference itself has the five properties"""
    for dh in (128, 64):
        q, k = _inputs(torch.bfloat16, dh)
        forced = R.forced_tiles(KEEP, NQB, NT)
        for cdf in CDFS:
            keep, p = R.plan(q, k, HEADS, cdf, KEEP)
            n = keep.sum(-1)
            print(f"dh {dh} cdf {cdf}: kept tiles per row {int(n.min())} .. {int(n.max())} of {NT}; forced {forced.sum(-1).tolist()}")
            assert int(n.max()) < NT and bool((n > forced.sum(-1)).any())
            lo, hi = R.plan(q, k, HEADS, cdf - DELTA, KEEP)[0], R.plan(q, k, HEADS, cdf + DELTA, KEEP)[0]
            assert float((lo != hi).float().mean()) < 0.01
            bit = _properties(keep, p, forced, cdf, "reference")
            assert bit["order"] > 0 and bit["minimal"] > 0
        if dh == 128:
            n5, n9 = R.plan(q, k, HEADS, 0.5, KEEP)[0].sum(-1), R.plan(q, k, HEADS, 0.9, KEEP)[0].sum(-1)
            assert 4 <= int(n5.min()) and int(n5.max()) <= 7 and 6 <= int(n9.min()) and int(n9.max()) <= 11, (n5, n9)


def test_reference_ties_and_packing():
    p = torch.tensor([0.3, 0.2, 0.2, 0.2, 0.1], dtype=torch.float64)
    none = torch.zeros(5, dtype=torch.bool)
    assert R.select_row(p, none, 0.4).tolist() == [True, True, True, True, False]        # ties at theta are all kept
    assert R.select_row(p, none, 0.3).tolist() == [True, False, False, False, False]
    assert R.select_row(p, none, 1.5).all()                                               # nothing qualifies: everything
    f = torch.tensor([False, False, False, False, True])
    assert R.select_row(p, f, 0.1).tolist() == f.tolist() and R.select_row(p, f, 0.35).tolist() == [True, False, False, False, True]
    keep = torch.rand(2, 3, 70, generator=torch.Generator().manual_seed(0)) < 0.5
    assert torch.equal(R.unpack_mask(R.pack_mask(keep), 70), keep) and R.pack_mask(keep).shape[-1] == 3
    from frameino_amd.window_attention import pack_tile_mask, unpack_tile_mask
    assert torch.equal(pack_tile_mask(keep), R.pack_mask(keep)) and torch.equal(unpack_tile_mask(R.pack_mask(keep), 70 * 64), keep)


@pytest.mark.gpu
@pytest.mark.parametrize("dh", [128, 64])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_the_plan_has_the_properties_of_the_definition(dtype, dh):
    from frameino_amd import ops
    q, k = _inputs(dtype, dh, "cuda")
    forced = R.forced_tiles(KEEP, NQB, NT)
    p = R.tile_probs(q, k, HEADS)
    for cdf in CDFS:
        mask = ops.attention_tile_plan(q, k, HEADS, cdf, keep_ranges=KEEP.cuda())
        assert mask.dtype == torch.int32 and tuple(mask.shape) == (B, HEADS, NQB, 1)
        assert torch.equal(mask, ops.attention_tile_plan(q, k, HEADS, cdf, keep_ranges=KEEP.cuda()))              # 6
        keep = R.unpack_mask(mask, NT)
        assert not (mask.cpu().to(torch.int64) & 0xffffffff >> NT << NT).any()        # no bit at or beyond tile 18
        bit = _properties(keep, p, forced, cdf, (str(dtype), dh, cdf))
        want = R.select(p, forced, cdf)
        print(f"{dtype} dh {dh} cdf {cdf}: {int((keep != want).sum())} of {keep.numel()} entries differ from the float64 "
              f"selection; density {ops.tile_mask_density(mask, LK):.3f}; properties bit on {bit}")
        assert abs(ops.tile_mask_density(mask, LK) - float(keep.float().mean())) < 1e-6
        # the folded scale: q pre-multiplied by scale * log2(e), logits taken as log2 units -- the same five properties, against
        # the float64 p of the pre-scaled q.  The pre-scaled q is rounded to the storage type once more (2^-9 of every logit in
        # bf16), so a tile at the threshold may fall the other way: the mask need not be the plain-scale mask bit for bit, and
        # how many entries differ is printed, not asserted (no bound for it follows from the formats).
        qf = (q.float() * (dh ** -0.5 * ops.LOG2E)).to(dtype)
        keep_f = R.unpack_mask(ops.attention_tile_plan(qf, k, HEADS, cdf, keep_ranges=KEEP.cuda(), scale=ops.SCALE_FOLDED), NT)
        _properties(keep_f, R.tile_probs(qf, k, HEADS, folded=True), forced, cdf, "folded")
        print(f"folded scale: {int((keep_f != keep).sum())} of {keep.numel()} entries differ from the plain-scale mask")
        # without forced tiles
        keep_n = R.unpack_mask(ops.attention_tile_plan(q, k, HEADS, cdf), NT)
        bit = _properties(keep_n, p, torch.zeros_like(forced), cdf, "keep_ranges=None")
        assert bit["order"] > 0 and bit["minimal"] == B * HEADS * NQB


@pytest.mark.gpu
def test_the_ragged_tile_counts_its_real_keys():
    """tile 17 holds 12 keys: its mean is over those 12 and its weight n = 12.  The buffer k is a view of holds 64 more rows
    behind the last key, all 3.0 (`_inputs`): a mean over the tile's 64 rows, or a weight of 64, moves p[17] far past the margin."""
    from frameino_amd import ops
    q, k = _inputs(torch.bfloat16, 128, "cuda")
    behind = k.as_strided((B, LK + 64, k.shape[2]), k.stride(), k.storage_offset())[:, LK:]
    assert k.stride(0) == (LK + 64) * k.stride(1) and bool((behind == 3.0).all())
    p = R.tile_probs(q, k, HEADS)
    for cdf in (0.3, 0.6):
        keep = R.unpack_mask(ops.attention_tile_plan(q, k, HEADS, cdf), NT)
        _properties(keep, p, torch.zeros(NQB, NT, dtype=torch.bool), cdf, "ragged")
    # all the mass on the ragged tile: it alone is kept, for any cdf < 1
    k2 = k.clone()
    k2[:, 64 * 17:] = 0
    k2[:, 64 * 17:, :] += q[:, :1].float().mean(1, keepdim=True).to(k2.dtype) * 4
    p2 = R.tile_probs(q, k2, HEADS)
    keep = R.unpack_mask(ops.attention_tile_plan(q, k2, HEADS, 0.9), NT)
    _properties(keep, p2, torch.zeros(NQB, NT, dtype=torch.bool), 0.9, "ragged heavy")
    assert bool(keep[..., 17].all())


@pytest.mark.gpu
def test_plan_argument_checks():
    from frameino_amd import ops
    q, k = _inputs(torch.bfloat16, 128, "cuda")
    with pytest.raises(AssertionError, match="ranges"):
        ops.attention_tile_plan(q, k, HEADS, 0.5, keep_ranges=KEEP[:2].cuda())
    with pytest.raises(AssertionError, match="out"):
        ops.attention_tile_plan(q, k, HEADS, 0.5, out=torch.zeros(B, HEADS, NQB, 1, dtype=torch.int64, device="cuda"))
    with pytest.raises(RuntimeError, match="cdf"):
        ops.attention_tile_plan(q, k, HEADS, 0.0)
    assert ops.attention_tile_plan_bytes(B, HEADS, LQ, LK, 128) == B * HEADS * (NQB + NT) * 128 * 4
    assert ops.attention_tile_plan_bytes(B, HEADS, LQ, LK, 96) == 0
    out = torch.full((B, HEADS, NQB, 3), -1, dtype=torch.int32, device="cuda")           # wider rows: every word is written
    ops.attention_tile_plan(q, k, HEADS, 0.5, out=out)
    assert not out[..., 1:].any() and torch.equal(out[..., :1], ops.attention_tile_plan(q, k, HEADS, 0.5))
