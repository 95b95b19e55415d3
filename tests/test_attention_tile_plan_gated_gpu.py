"""fino_attn_tile_plan_gated (csrc/fino_attention_plan.hip, `ops.attention_tile_plan(cdf_heads=, similarity_threshold=)`): the
similarity gate and the per-head thresholds of the dynamic block-sparse self-attention, against the
float64 restatement in tests/sparse_gate_ref.py.

Shape, forced tiles, the five properties and their derived margin 1e-3 are those of tests/test_attention_tile_plan_gpu.py: B = 2,
H = 3, Lq = 600 (a ragged 88-row q-block), Lk = 1100 (a ragged 12-key tile), head_dim 64 and 128, bf16 and fp16.

Inputs (`_inputs`, seed 4321 + dh): N(0, 1) rows plus a unit direction u per (b, h) scaled to norm sqrt(dh).  Key tile t gets
+ c u, |c| drawn from {0.15, 1, 1.5, 2} with a random sign; q-block i gets + a_i u, a = (1, 0.1, 1); theta = 0.25.  A row z + c u
has |x|^2 ~ dh (1 + c^2), so a block's similarity is ~ c^2 / (1 + c^2) + 1 / n: >= 0.49 for |c| >= 1, ~ 0.01 .. 0.11 for the
incoherent blocks.  On the float64 reference (tests/test_sparse_gate_cpu.py asserts it): no similarity within 0.13 of theta, 3 .. 7
of the 18 key tiles unpredictable per (b, h), exactly the middle q-block dense.  The fp32 similarity is orders of magnitude closer
than that gap: an fp32 sum of at most 256 unit-norm terms is off by at most 256 x 2^-24 relative, the assertion allows 1e-4."""
import pytest
import torch

from tests import sparse_attn_ref as R
from tests import sparse_gate_ref as G
from tests.test_attention_tile_plan_gpu import B, HEADS, KEEP, LK, LQ, NQB, NT, _properties

THETA = 0.25
CDFS = (0.5, 0.9)
SIM_TOL = 1e-4
MAGNITUDES = (0.15, 1.0, 1.5, 2.0)
Q_STRENGTH = (1.0, 0.1, 1.0)


def _inputs(dtype, dh, device="cpu", strength=(1.0, 1.0, 1.0), seed=4321):
    """(q, k, v) on `device` in `dtype`: row-strided views of a fused buffer, as the model's are.  `strength`: a factor per head
    on the structure added to q and k (tests/test_sparse_calibration_gpu.py makes the heads differ with it)."""
    d = HEADS * dh
    g = torch.Generator().manual_seed(seed + dh)
    qkv = torch.randn(B, max(LQ, LK), 3 * d + 64, generator=g)
    u = torch.randn(B, HEADS, dh, generator=g)
    u = u / u.norm(dim=-1, keepdim=True) * dh ** 0.5
    mag = torch.tensor(MAGNITUDES)[torch.randint(0, len(MAGNITUDES), (B, NT, HEADS), generator=g)]
    sign = torch.randint(0, 2, (B, NT, HEADS), generator=g).float() * 2 - 1
    st = torch.tensor(strength, dtype=torch.float32)
    c = mag * sign * st
    qkv[:, :LK, d:2 * d] += (c[..., None] * u[:, None]).repeat_interleave(64, dim=1)[:, :LK].reshape(B, LK, d)
    a = torch.tensor(Q_STRENGTH).repeat_interleave(256)[:LQ]
    qkv[:, :LQ, :d] += (a[None, :, None, None] * st[None, None, :, None] * u[:, None]).reshape(B, LQ, d)
    # 64 further rows behind the last key, far from zero: a pass that read the ragged tile's 64 rows would pick them up
    qkv = torch.cat([qkv, torch.full((B, 64, qkv.shape[2]), 3.0)], dim=1).to(dtype).to(device)
    return qkv[:, :LQ, :d], qkv[:, :LK, d:2 * d], qkv[:, :LK, 2 * d:3 * d]


def _gated_properties(keep, p, dense, unpred, forced, cdf, what):
    """dense rows are full, every unpredictable tile is kept in every row, and the other rows have the five properties against
    the gated p with the forced set F + U (`forced`: F, bool [nqb, nt])"""
    bit = {"mass": 0, "order": 0, "minimal": 0, "forced_only": 0}
    for b in range(B):
        for h in range(HEADS):
            assert bool(keep[b, h][:, unpred[b, h]].all()), ("an unpredictable tile was dropped", what, b, h)
            for i in range(NQB):
                if bool(dense[b, h, i]):
                    assert bool(keep[b, h, i].all()), ("a dense row is not full", what, b, h, i)
            rows = [i for i in range(NQB) if not bool(dense[b, h, i])]
            got = _properties(keep[b:b + 1, h:h + 1][:, :, rows], p[b:b + 1, h:h + 1][:, :, rows], (forced | unpred[b, h])[rows],
                              cdf, (what, b, h, rows))
            bit = {n: bit[n] + got[n] for n in bit}
    return bit


@pytest.mark.gpu
@pytest.mark.parametrize("dh", [128, 64])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_the_gated_plan_has_the_properties_of_the_definition(dtype, dh):
    from frameino_amd import ops
    q, k, _ = _inputs(dtype, dh, "cuda")
    sq, sk = G.similarity(q, k, HEADS)
    p, dense, unpred = G.gated_probs(q, k, HEADS, THETA)
    forced, none = R.forced_tiles(KEEP, NQB, NT), torch.zeros(NQB, NT, dtype=torch.bool)
    for cdf in CDFS:
        mask, (gq, gk) = ops.attention_tile_plan(q, k, HEADS, cdf, keep_ranges=KEEP.cuda(), similarity_threshold=THETA,
                                                 return_similarity=True)
        assert mask.dtype == torch.int32 and tuple(mask.shape) == (B, HEADS, NQB, 1)
        assert tuple(gq.shape) == (B, HEADS, NQB) and tuple(gk.shape) == (B, HEADS, NT) and gq.dtype == torch.float32
        eq, ek = float((gq.cpu().double() - sq).abs().max()), float((gk.cpu().double() - sk).abs().max())
        print(f"{dtype} dh {dh} cdf {cdf}: similarity off by {eq:.2e} (q-blocks), {ek:.2e} (key tiles)")
        assert eq <= SIM_TOL and ek <= SIM_TOL
        again = ops.attention_tile_plan(q, k, HEADS, cdf, keep_ranges=KEEP.cuda(), similarity_threshold=THETA)
        assert torch.equal(mask, again)                                                    # two runs are bit-equal
        assert not (mask.cpu().to(torch.int64) & 0xffffffff >> NT << NT).any()             # no bit at or beyond tile 18
        keep = R.unpack_mask(mask, NT)
        bit = _gated_properties(keep, p, dense, unpred, forced, cdf, (str(dtype), dh, cdf))
        want = G.plan_gated(q, k, HEADS, cdf, KEEP, THETA)[0]
        print(f"   {int((keep != want).sum())} of {keep.numel()} entries differ from the float64 selection; density "
              f"{float(keep.float().mean()):.3f}; properties bit on {bit}")
        assert bit["mass"] == B * HEADS * 2 and bit["order"] > 0
        # the gate changes the mask: the ungated plan drops unpredictable tiles and thins the dense rows
        plain = R.unpack_mask(ops.attention_tile_plan(q, k, HEADS, cdf, keep_ranges=KEEP.cuda()), NT)
        assert not torch.equal(plain, keep)
        # without forced tiles
        keep_n = R.unpack_mask(ops.attention_tile_plan(q, k, HEADS, cdf, similarity_threshold=THETA), NT)
        _gated_properties(keep_n, p, dense, unpred, none, cdf, "keep_ranges=None")
    # the folded scale: the same properties against the float64 p of the pre-scaled q
    qf = (q.float() * (dh ** -0.5 * ops.LOG2E)).to(dtype)
    pf, densef, unpredf = G.gated_probs(qf, k, HEADS, THETA, folded=True)
    assert torch.equal(densef, dense) and torch.equal(unpredf, unpred)
    keep_f = R.unpack_mask(ops.attention_tile_plan(qf, k, HEADS, 0.9, keep_ranges=KEEP.cuda(), scale=ops.SCALE_FOLDED,
                                                   similarity_threshold=THETA), NT)
    _gated_properties(keep_f, pf, dense, unpred, forced, 0.9, "folded")


@pytest.mark.gpu
@pytest.mark.parametrize("dh", [128, 64])
def test_gate_off_and_a_uniform_table_are_the_old_entry_bit_for_bit(dh):
    from frameino_amd import ops
    q, k, _ = _inputs(torch.bfloat16, dh, "cuda")
    for cdf in CDFS + (1.0, 1.5):
        old = ops.attention_tile_plan(q, k, HEADS, cdf, keep_ranges=KEEP.cuda())
        table = torch.full((HEADS,), cdf, dtype=torch.float32, device="cuda")
        if cdf < 1:
            assert torch.equal(ops.attention_tile_plan(q, k, HEADS, cdf, keep_ranges=KEEP.cuda(), cdf_heads=table), old), cdf
            assert torch.equal(ops.attention_tile_plan(q, k, HEADS, 0.123, keep_ranges=KEEP.cuda(), cdf_heads=table), old)  # the table wins
        else:                             # a table value >= 1 keeps every tile, explicitly
            full = R.unpack_mask(ops.attention_tile_plan(q, k, HEADS, cdf, keep_ranges=KEEP.cuda(), cdf_heads=table), NT)
            assert bool(full.all())
    # the C entry itself with neither: what the old entry gives
    from frameino_amd import _lib
    old = ops.attention_tile_plan(q, k, HEADS, 0.5, keep_ranges=KEEP.cuda())
    out = torch.full_like(old, -1)
    ws = torch.empty(ops.attention_tile_plan_bytes(B, HEADS, LQ, LK, dh) // 4, dtype=torch.float32, device="cuda")
    rc = _lib.lib().fino_attn_tile_plan_gated(q.data_ptr(), k.data_ptr(), B, HEADS, LQ, LK, dh, q.stride(0), q.stride(1), dh,
                                              k.stride(0), k.stride(1), dh, dh ** -0.5, ops._dt(q), 0.5, 0, 0.0, KEEP.cuda().data_ptr(),
                                              out.data_ptr(), 1, ws.data_ptr(), ws.numel() * 4,
                                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(out, old)


@pytest.mark.gpu
@pytest.mark.parametrize("dh", [128, 64])
def test_a_per_head_table_gives_each_head_its_scalar_mask(dh):
    from frameino_amd import ops
    q, k, _ = _inputs(torch.bfloat16, dh, "cuda")
    table = torch.tensor([0.5, 0.9, 1.0], dtype=torch.float32, device="cuda")
    for gate in ({}, {"similarity_threshold": THETA}):
        got = ops.attention_tile_plan(q, k, HEADS, 0.7, keep_ranges=KEEP.cuda(), cdf_heads=table, **gate)
        m5 = ops.attention_tile_plan(q, k, HEADS, 0.5, keep_ranges=KEEP.cuda(), **gate)
        m9 = ops.attention_tile_plan(q, k, HEADS, 0.9, keep_ranges=KEEP.cuda(), **gate)
        assert torch.equal(got[:, 0], m5[:, 0]) and torch.equal(got[:, 1], m9[:, 1])
        assert not torch.equal(m5[:, 0], m9[:, 0])
        assert bool(R.unpack_mask(got[:, 2:], NT).all()) and int(got[0, 2, 0, 0]) == (1 << NT) - 1


@pytest.mark.gpu
def test_more_than_256_tiles_a_thread_owns_several():
    """B = H = 1, Lq = 256, Lk = 16455: 258 key tiles, threads 0 and 1 of the select kernel own two, the last tile holds 7 keys"""
    from frameino_amd import ops
    dh, lq, lk = 64, 256, 16455
    nt = R.ntiles(lk)
    g = torch.Generator().manual_seed(99)
    u = torch.randn(dh, generator=g)
    u = u / u.norm() * dh ** 0.5
    c = torch.tensor(MAGNITUDES)[torch.randint(0, 4, (nt,), generator=g)] * (torch.randint(0, 2, (nt,), generator=g).float() * 2 - 1)
    c[256], c[257] = 0.15, 2.0                      # the two tiles of the second round: one unpredictable, one not
    k = (torch.randn(1, lk, dh, generator=g) + (c[:, None] * u).repeat_interleave(64, dim=0)[:lk]).bfloat16().cuda()
    # q: coherent along a second direction w the keys do not carry, and only 0.05 u, so that the logits stay moderate (+- 0.8)
    # and the pooled softmax over 258 tiles is neither uniform nor one-hot
    w = torch.randn(dh, generator=g)
    w = w / w.norm() * dh ** 0.5
    q = (torch.randn(1, lq, dh, generator=g) + w + 0.05 * u).bfloat16().cuda()
    theta = THETA
    sq, sk = G.similarity(q, k, 1)
    gap = float((torch.cat([sq.flatten(), sk.flatten()]) - theta).abs().min())
    p, dense, unpred = G.gated_probs(q, k, 1, theta)
    print(f"258 tiles: {int(unpred.sum())} unpredictable, smallest distance to theta {gap:.3e}")
    assert gap > 0.05 and 0 < int(unpred.sum()) < nt and not bool(dense.any())
    assert bool(unpred[0, 0, 256]) and not bool(unpred[0, 0, 257])
    mask, (gq, gk) = ops.attention_tile_plan(q, k, 1, 0.5, similarity_threshold=theta, return_similarity=True)
    assert tuple(mask.shape) == (1, 1, 1, 9) and tuple(gk.shape) == (1, 1, nt)
    assert float((gk.cpu().double() - sk).abs().max()) <= SIM_TOL and float((gq.cpu().double() - sq).abs().max()) <= SIM_TOL
    keep = R.unpack_mask(mask, nt)
    assert bool(keep[0, 0, 0][unpred[0, 0]].all())
    none = torch.zeros(1, nt, dtype=torch.bool)
    bit = _properties(keep, p, none | unpred[0, 0], 0.5, "258 tiles")
    assert bit["order"] == 1 and bit["minimal"] == 1
    assert not (mask.cpu().to(torch.int64)[..., 8] & 0xffffffff >> 2 << 2).any()          # no bit at or beyond tile 258
    assert torch.equal(mask, ops.attention_tile_plan(q, k, 1, 0.5, similarity_threshold=theta))


@pytest.mark.gpu
def test_gated_plan_argument_checks():
    from frameino_amd import ops
    q, k, _ = _inputs(torch.bfloat16, 128, "cuda")
    ok = torch.full((HEADS,), 0.5, dtype=torch.float32, device="cuda")
    for bad in (ok.cpu(), ok.double(), torch.full((HEADS + 1,), 0.5, device="cuda"), ok.repeat(2)[::2], [0.5] * HEADS):
        with pytest.raises(AssertionError, match="cdf_heads"):
            ops.attention_tile_plan(q, k, HEADS, 0.5, cdf_heads=bad)
    for bad in (0.0, -0.1, 1.5):
        with pytest.raises(AssertionError, match="similarity_threshold"):
            ops.attention_tile_plan(q, k, HEADS, 0.5, similarity_threshold=bad)
    with pytest.raises(AssertionError, match="return_similarity"):
        ops.attention_tile_plan(q, k, HEADS, 0.5, return_similarity=True)
    plain = ops.attention_tile_plan_bytes(B, HEADS, LQ, LK, 128)
    assert ops.attention_tile_plan_gated_bytes(B, HEADS, LQ, LK, 128) == plain + B * HEADS * (NQB + NT) * 4
    assert ops.attention_tile_plan_gated_bytes(B, HEADS, LQ, LK, 96) == 0
    small = torch.empty(plain // 4, dtype=torch.float32, device="cuda")                   # the ungated size: too small under the gate
    with pytest.raises(AssertionError):
        ops.attention_tile_plan(q, k, HEADS, 0.5, similarity_threshold=THETA, workspace=small)
    ops.attention_tile_plan(q, k, HEADS, 0.5, cdf_heads=ok, workspace=small)              # ... enough for a table alone
    with pytest.raises(RuntimeError, match="cdf"):
        ops.attention_tile_plan(q, k, HEADS, 0.0, cdf_heads=ok)
    out = torch.full((B, HEADS, NQB, 3), -1, dtype=torch.int32, device="cuda")            # wider rows: every word is written
    ops.attention_tile_plan(q, k, HEADS, 0.5, similarity_threshold=THETA, out=out)
    assert not out[..., 1:].any()
    assert torch.equal(out[..., :1], ops.attention_tile_plan(q, k, HEADS, 0.5, similarity_threshold=THETA))
    # a caller-owned workspace of the gated size: the similarities are read from ITS tail
    ws = torch.zeros(ops.attention_tile_plan_gated_bytes(B, HEADS, LQ, LK, 128) // 4, dtype=torch.float32, device="cuda")
    _, (gq, gk) = ops.attention_tile_plan(q, k, HEADS, 0.5, similarity_threshold=THETA, workspace=ws, return_similarity=True)
    assert torch.equal(ws[plain // 4:plain // 4 + B * HEADS * NQB].view(B, HEADS, NQB), gq) and float(gk.min()) > 0
