"""Smooth V of the fp8 attention (fino_attn_fwd_fp8_smoothed, csrc/fino_attention_fp8.hip): the mean of V over the keys, per (batch
element, head, channel), is subtracted before V becomes e4m3 and added back, in fp32, to the normalised output before its one
rounding to bf16 / fp16.  O = P (V - mu) / l + mu is exact because l sums the same rounded P bytes: the weights sum to 1.  What is
stated and checked, at head_dim 64 (free-running and ping-pong kernel) and 128, bf16 and fp16, both p_modes:

  * exact properties on integer values: a value mean of zero gives the plain call's bits; a constant V comes back exactly (and does
    NOT without smoothing), per batch element, channel and sub-head, through the dense kernels, the range walk and the head_dim 128
    tail split + combine; V + c gives (V's result) + c to one ulp of the storage dtype;
  * against fp32 SDPA on values with a per-(batch element, channel) offset 8 x N(0, 1): within 1.2 x the torch emulation of the
    same quantisation rounded to the storage dtype (tests/attn_fp8_smooth_v_ref.py), no additive term, on inputs where the plain
    emulation is at least 3 x (fp16) / 1.45 x (bf16) worse;
  * N(0, 1) inputs keep the bounds of tests/test_attention_fp8_gpu.py, V = 1 gives 1, rows past lq stay untouched, two calls give
    the same bits;
  * `enable_fp8_attention(smooth_v=True)` on the tiny Wan and CogVideoX models (the default staying the plain path bit for bit),
    the CogVideoX windowed forward, and the Wan hipGraph loop replaying the eager loop's bits with both switches on."""
import pytest
import torch

from tests.attn_fp8_smooth_v_ref import (CONDITION, OFFSET_SHAPES, constant_c, emulated, offset_v_inputs, plan_split, sdpa,
                                         sdpa_masked, table_mask, ulp)
from tests.parity import record, rel_rms
from tests.test_attention_fp8_ranges_gpu import TABLES, _table
from tests.test_attention_fp8_ranges_gpu import B as RB, HEADS as RH, LK as RLK, LQ as RLQ
from tests.test_attention_fp8_smooth_gpu import COG_FP8_BOUND, WAN_FP8_BOUND
from tests.test_window_attention_cog_gpu import setup  # noqa: F401  (the fixture: weights that separate a window from none)

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
dtypes = pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
p_modes = pytest.mark.parametrize("p_mode", ["exp2", "ramp"])


@pytest.fixture(params=[(64, 0), (64, 1), (128, 0)], ids=["d64-free-running", "d64-ping-pong", "d128"])
def variant(request):
    """head_dim and main kernel, as tests/test_attention_fp8_smooth_gpu.py: at head_dim 64 the default (4 waves) and
    FINO_TUNE_ATTN_FP8_KERNEL = 1 (tune knob 5); head_dim 128 has one"""
    from frameino_amd import _lib
    dh, knob = request.param
    _lib.lib().fino_tune_set(5, knob)
    yield dh
    _lib.lib().fino_tune_set(5, 0)


def _heads(heads, dh):
    return heads if dh == 64 else max(1, heads // 2)


def _qk(b, lq, lk, d, dtype, seed):
    """q = N(0, 1) / 8 and a k | v buffer (row-strided views) whose k part is N(0, 1)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    q = (torch.randn(b, lq, d, device=DEV, generator=g) / 8).to(dtype)
    kv = torch.randn(b, lk, 2 * d + 64, device=DEV, generator=g)
    return q, kv, g


# ------------------------------------------------------------------ 1. a value mean of exactly zero: the plain call's bits
@pytest.mark.parametrize("lk", [128, 640])
@dtypes
@p_modes
def test_zero_value_mean_gives_the_bits_of_the_plain_call(variant, p_mode, dtype, lk):
    """V = [X ; -X] over the keys with integer X in [-4, 4]: every partial sum is an fp32 integer in any order, the mean is exactly
    0, V - 0 = V and x + 0 = x.  K is built the same way, so both switches together must give the plain bits as well."""
    from frameino_amd import ops
    dh, heads = variant, _heads(4, variant)
    d = heads * dh
    q, kv, g = _qk(2, 100, lk, d, dtype, 41 + lk)
    x = torch.randint(-4, 5, (2, lk // 2, 2 * d), device=DEV, generator=g).float()
    kv[:, :, :2 * d] = torch.cat([x, -x], 1)
    kv = kv.to(dtype)
    k, v = kv[:, :, :d], kv[:, :, d:2 * d]
    assert not v.float().sum(1).any() and not k.float().sum(1).any()
    plain = ops.attention_fp8(q, k, v, heads, p_mode=p_mode)
    assert torch.isfinite(plain.float()).all() and plain.float().abs().max() > 0
    assert torch.equal(ops.attention_fp8(q, k, v, heads, p_mode=p_mode, smooth_v=True), plain)
    assert torch.equal(ops.attention_fp8(q, k, v, heads, p_mode=p_mode, smooth_k=True, smooth_v=True), plain)


# ------------------------------------------------------------------ 2. a constant V comes back exactly
def _constant_case(b, heads, dh, lq, lk, dtype, seed):
    d = heads * dh
    q, kv, _ = _qk(b, lq, lk, d, dtype, seed)
    c = constant_c(b, d).to(DEV)
    kv[:, :, d:2 * d] = c[:, None]
    kv = kv.to(dtype)
    assert torch.equal(kv[:, :, d:2 * d].float(), c[:, None].expand(b, lk, d))          # (exact in the storage type)
    return q, kv[:, :, :d], kv[:, :, d:2 * d], c


def _check_constant(ops, q, k, v, c, heads, p_mode, **kw):
    lq = q.shape[1]
    want = c[:, None].expand(-1, lq, -1)
    for smooth_k in (False, True):
        got = ops.attention_fp8(q, k, v, heads, p_mode=p_mode, smooth_k=smooth_k, smooth_v=True, **kw).float()
        bad = (got != want).nonzero()
        assert not len(bad), (smooth_k, bad[:4].tolist(), got[tuple(bad[0])].item(), want[tuple(bad[0])].item())
    plain = ops.attention_fp8(q, k, v, heads, p_mode=p_mode, **kw).float()
    assert not torch.equal(plain, want)                   # e4m3 has no odd integer above 16: the plain path cannot return c


@pytest.mark.parametrize("lk", [65, 256, 1024])
@dtypes
@p_modes
def test_a_constant_value_comes_back_exactly(variant, p_mode, dtype, lk):
    """every key's V = c[batch element, channel], odd integers in [33, 63] that differ per batch element, channel and sub-head
    (a mean over the wrong axis, the other sub-head's means or a batch stride error all show).  lk x c is exact in fp32 (65 x 63
    included, a ragged tile and a ragged 256-key chunk), the division is exact, V - mu = 0 and 0 + mu = c.  At head_dim 128,
    lk = 1024 is cut by the tail split (16 key tiles of the one q-block over 2 workgroups): the combine adds mu."""
    from frameino_amd import ops
    dh, heads = variant, _heads(4, variant)
    q, k, v, c = _constant_case(2, heads, dh, 300, lk, dtype, 53 + lk)
    _check_constant(ops, q, k, v, c, heads, p_mode)


# ------------------------------------------------------------------ 3. V + c: the result + c, to one ulp
@pytest.mark.parametrize("lk", [256, 1024])
@dtypes
@p_modes
def test_an_integer_offset_per_channel_moves_the_result_by_the_offset(variant, p_mode, dtype, lk):
    """V integer in [-8, 8], c integer in [-64, 64] per (batch element, channel), lk a power of two: V + c is exact in bf16 / fp16,
    the sums and the division by lk are exact in fp32, (V + c) - (mu + c) = V - mu exactly, so the quantiser and the matrix pipe
    see the same numbers and x = P (V - mu) / l has the same bits.  The outputs are T(x + mu + c) and T(x + mu): each is within
    half an ulp (of its own magnitude) of its fp32 sum, so T(x + mu + c) - (T(x + mu) + c), evaluated in fp32, is at most one ulp
    of the larger of the two outputs' magnitudes.  Without smoothing the offset reaches e4m3 and this fails somewhere."""
    from frameino_amd import ops
    dh, heads = variant, _heads(4, variant)
    d = heads * dh
    q, kv, g = _qk(2, 100, lk, d, dtype, 67 + lk)
    kv[:, :, d:2 * d] = torch.randint(-8, 9, (2, lk, d), device=DEV, generator=g).float()
    c = torch.randint(-64, 65, (2, 1, d), device=DEV, generator=g).float()
    kv = kv.to(dtype)
    kvc = kv.clone()
    kvc[:, :, d:2 * d] = (kv[:, :, d:2 * d].float() + c).to(dtype)
    assert torch.equal(kvc[:, :, d:2 * d].float(), kv[:, :, d:2 * d].float() + c)
    k, v, vc = kv[:, :, :d], kv[:, :, d:2 * d], kvc[:, :, d:2 * d]

    def excess(**kw):
        base = ops.attention_fp8(q, k, v, heads, p_mode=p_mode, **kw).float()
        shifted = ops.attention_fp8(q, k, vc, heads, p_mode=p_mode, **kw).float()
        assert torch.isfinite(shifted).all()
        # (the larger of the two OUTPUTS: base + c is not an output, and where c cancels base it is far smaller than either rounding)
        return ((shifted - (base + c)).abs() / ulp(torch.maximum(shifted.abs(), base.abs()), dtype)).max().item()
    e = excess(smooth_v=True)
    eb = excess(smooth_k=True, smooth_v=True)
    ep = excess()
    print(f"V + c vs (V) + c in ulps of the larger: smooth V {e}, both {eb}, plain {ep}")
    assert e <= 1.0 and eb <= 1.0, (e, eb)
    assert ep > 1.0, ep


# ------------------------------------------------------------------ 4. values with a channel offset, against fp32 SDPA
def _offset_check(name, dtype, ref, emu_smooth, emu_plain, kernel_smooth, kernel_plain):
    re, rpe = rel_rms(emu_smooth, ref), rel_rms(emu_plain, ref)
    assert rpe >= CONDITION[dtype] * re, (rpe, re)        # the condition on the inputs: the offset does cost the plain quantiser
    r, rp = rel_rms(kernel_smooth, ref), rel_rms(kernel_plain, ref)
    print(f"{name}: smoothed kernel {r:.5f}  smoothed emulation {re:.5f}  plain kernel {rp:.5f}  plain emulation {rpe:.5f}")
    record(name, f"rel_rms vs fp32 SDPA (smoothed emulation {re:.5f}; plain kernel {rp:.5f}, plain emulation {rpe:.5f})", r, 1.2 * re)
    assert torch.isfinite(kernel_smooth.float()).all() and r < 1.2 * re, (r, re, rp, rpe)


@pytest.mark.parametrize("b,heads,lq,lk", OFFSET_SHAPES)
@dtypes
@p_modes
def test_offset_values_vs_fp32_and_vs_the_smoothed_emulation(variant, p_mode, dtype, b, heads, lq, lk):
    """V = N(0, 1) + 8 N(0, 1) per (batch element, channel).  Bound: 1.2 x the smoothed emulation (rounded to the storage dtype like
    the kernel's output), the margin the other fp8 tests grant the kernel over its emulation; no additive term -- the errors here
    are 5e-4 .. 5e-3 and the 2e-3 of those tests would swallow the effect."""
    from frameino_amd import ops
    dh, heads = variant, _heads(heads, variant)
    q, k, v = offset_v_inputs(b, heads, lq, lk, dh, dtype, DEV)
    _offset_check(f"attention_fp8_smooth_v_offset_values[{p_mode}-b{b}-h{heads}x{dh}-lq{lq}-lk{lk}-{str(dtype)[6:]}]", dtype,
                  sdpa(q, k, v, heads), emulated(q, k, v, heads, p_mode, smooth_v=True), emulated(q, k, v, heads, p_mode),
                  ops.attention_fp8(q, k, v, heads, p_mode=p_mode, smooth_v=True), ops.attention_fp8(q, k, v, heads, p_mode=p_mode))


# ------------------------------------------------------------------ 5 / 6 / 8. N(0, 1) inputs, V = 1, guard rows
@pytest.mark.parametrize("b,heads,lq,lk", [(1, 2, 256, 256), (2, 3, 300, 1000), (1, 8, 1000, 777)])
@dtypes
@p_modes
def test_standard_normal_inputs_keep_the_bounds_of_the_plain_path(variant, p_mode, dtype, b, heads, lq, lk):
    """tests/test_attention_fp8_gpu.py's bounds (rel-RMS < 8e-2 and < 1.2 x the emulation + 2e-3) with smooth_v and with both
    switches; V = 1 gives 1 within 4e-3; rows past lq of a larger `out` stay untouched"""
    from frameino_amd import ops
    dh, heads = variant, _heads(heads, variant)
    d = heads * dh
    g = torch.Generator(device=DEV).manual_seed(lq + lk + heads + 3)
    q = torch.randn(b, lq, d, device=DEV, generator=g).to(dtype)
    kv = torch.randn(b, lk, 2 * d + 64, device=DEV, generator=g).to(dtype)
    k, v = kv[:, :, :d], kv[:, :, d:2 * d]
    ref = sdpa(q, k, v, heads)
    for smooth_k in (False, True):
        out = torch.full((b, lq + 7, d), 3.0, device=DEV, dtype=dtype)
        o = ops.attention_fp8(q, k, v, heads, out=out[:, :lq], p_mode=p_mode, smooth_k=smooth_k, smooth_v=True)
        assert torch.isfinite(o.float()).all() and (out[:, lq:] == 3.0).all()
        r, re = rel_rms(o, ref), rel_rms(emulated(q, k, v, heads, p_mode, smooth_k=smooth_k, smooth_v=True), ref)
        record(f"attention_fp8_smooth_v[{p_mode}-k{int(smooth_k)}-b{b}-h{heads}x{dh}-lq{lq}-lk{lk}-{str(dtype)[6:]}]",
               f"rel_rms vs fp32 SDPA (smoothed emulation: {re:.4f})", r, 8e-2)
        assert r < 8e-2 and r < 1.2 * re + 2e-3, (smooth_k, r, re)
        o1 = ops.attention_fp8(q, k, torch.ones_like(v), heads, p_mode=p_mode, smooth_k=smooth_k, smooth_v=True)
        assert (o1.float() - 1).abs().max().item() < 4e-3


# ------------------------------------------------------------------ 7. the same inputs, the same bits
@dtypes
def test_two_calls_give_the_same_bits(variant, dtype):
    from frameino_amd import ops
    dh, heads = variant, _heads(3, variant)
    q, k, v = offset_v_inputs(2, heads, 300, 1000, dh, dtype, DEV)
    for smooth_k in (False, True):
        first = ops.attention_fp8(q, k, v, heads, smooth_k=smooth_k, smooth_v=True).clone()
        assert torch.equal(ops.attention_fp8(q, k, v, heads, smooth_k=smooth_k, smooth_v=True), first)


# ------------------------------------------------------------------ 9. the range walk (head_dim 64)
def _ranges(ops, q, k, v, table, p_mode, **kw):
    lq = q.shape[1]
    out = torch.full((q.shape[0], lq + 5, q.shape[2]), 3.0, dtype=q.dtype, device=DEV)
    got = ops.attention_fp8_ranges(q, k, v, RH, table.to(DEV), out=out[:, :lq], p_mode=p_mode, **kw)
    assert (out[:, lq:] == 3.0).all() and torch.isfinite(got.float()).all()
    return got


EMPTY_BLOCK = _table([(2, 5)], [], [(0, 1), (17, 18)])          # q-block 1 walks no tile


@pytest.mark.parametrize("name", ["per_block", "nt5_first_not_at_0_last_ragged", "ragged_only", "empty_block"])
@dtypes
@p_modes
def test_range_walk_a_constant_value_comes_back_exactly_and_an_empty_block_gets_zeros(name, dtype, p_mode):
    """the mean is the mean over ALL keys, whatever subset a q-block walks: c exactly on every row that walks a tile, zeros -- not
    the mean -- on the rows of a q-block without tiles"""
    from frameino_amd import ops
    table = EMPTY_BLOCK if name == "empty_block" else TABLES[name]
    q, k, v, c = _constant_case(RB, RH, 64, RLQ, RLK, dtype, 71)
    want = c[:, None].expand(-1, RLQ, -1).clone()
    walked = table_mask(table, RLQ, RLK, DEV).any(1)
    want[:, ~walked] = 0
    assert name != "empty_block" or (~walked).sum().item() == 256
    for smooth_k in (False, True):
        got = _ranges(ops, q, k, v, table, p_mode, smooth_k=smooth_k, smooth_v=True).float()
        assert torch.equal(got, want), (smooth_k, (got != want).nonzero()[:4].tolist())
    assert not torch.equal(_ranges(ops, q, k, v, table, p_mode).float(), want)


@pytest.mark.parametrize("name", ["per_block", "empty_block"])
@dtypes
@p_modes
def test_range_walk_offset_values_vs_fp32_under_the_block_mask(name, dtype, p_mode):
    """test 4 through the range walk: fp32 SDPA and the emulation masked from the same table (a q-block without tiles: zeros in all
    of them)"""
    from frameino_amd import ops
    table = EMPTY_BLOCK if name == "empty_block" else TABLES[name]
    q, k, v = offset_v_inputs(RB, RH, RLQ, RLK, 64, dtype, DEV)
    mask = table_mask(table, RLQ, RLK, DEV)
    got = _ranges(ops, q, k, v, table, p_mode, smooth_v=True)
    if name == "empty_block":
        assert not got[:, 256:512].any()
    _offset_check(f"attention_fp8_ranges_smooth_v_offset_values[{p_mode}-{name}-{str(dtype)[6:]}]", dtype,
                  sdpa_masked(q, k, v, RH, mask), emulated(q, k, v, RH, p_mode, smooth_v=True, mask=mask),
                  emulated(q, k, v, RH, p_mode, mask=mask), got, _ranges(ops, q, k, v, table, p_mode))


@dtypes
@p_modes
def test_range_walk_over_an_all_covering_table_gives_the_dense_call_s_bits(dtype, p_mode):
    from frameino_amd import ops
    q, k, v = offset_v_inputs(RB, RH, RLQ, RLK, 64, dtype, DEV)
    for smooth_k in (False, True):
        assert torch.equal(_ranges(ops, q, k, v, TABLES["full"], p_mode, smooth_k=smooth_k, smooth_v=True),
                           ops.attention_fp8(q, k, v, RH, p_mode=p_mode, smooth_k=smooth_k, smooth_v=True))


# ------------------------------------------------------------------ 10. head_dim 128: the tail split and its combine
@pytest.mark.parametrize("lk", [1024, 1000, 256])
@dtypes
@p_modes
def test_d128_tail_split_and_whole_blocks_return_a_constant_value_exactly(p_mode, dtype, lk):
    """batch 2 x 4 heads x one q-block (lq = 200) = 8 blocks, one per XCD: a last round of rem_x = 1 block per XCD.  With lk = 1024
    or 1000 (16 key tiles, the last ragged at 1000) csrc/fino_attention.hip::plan_split cuts them over nwg = 2 workgroups of
    per = 8 tiles -- partials without mu, attn_combine_kernel adds it; with lk = 256 (4 tiles: fewer than the 8 a range needs)
    rem_x = 0 and the main kernel's epilogue adds it.  Both derived from the plan restated in tests/attn_fp8_smooth_v_ref.py on
    this device's CU count."""
    from frameino_amd import ops
    b, heads, lq = 2, 4, 200
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    full_x, rem_x, nwg, per = plan_split(b, heads, -(-lq // 256), -(-lk // 64), cus)
    if lk == 256:
        assert rem_x == 0, (cus, full_x, rem_x, nwg, per)
    else:
        assert rem_x > 0 and 1 < nwg <= 32 and per < -(-lk // 64), (cus, full_x, rem_x, nwg, per)
    q, k, v, c = _constant_case(b, heads, 128, lq, lk, dtype, 83 + lk)
    _check_constant(ops, q, k, v, c, heads, p_mode)
    # ... and on offset values the split shape keeps test 4's bound
    q, k, v = offset_v_inputs(b, heads, lq, lk, 128, dtype, DEV)
    _offset_check(f"attention_fp8_smooth_v_offset_values[{p_mode}-b{b}-h{heads}x128-lq{lq}-lk{lk}-{str(dtype)[6:]}]", dtype,
                  sdpa(q, k, v, heads), emulated(q, k, v, heads, p_mode, smooth_v=True), emulated(q, k, v, heads, p_mode),
                  ops.attention_fp8(q, k, v, heads, p_mode=p_mode, smooth_v=True), ops.attention_fp8(q, k, v, heads, p_mode=p_mode))


# ------------------------------------------------------------------ 11. models and the denoise loop
def _check_switch(name, m, run, bound):
    ref = run()
    m.enable_fp8_attention()
    assert m.fp8_attention and m.fp8_smooth_v is False and m.fp8_smooth_k is False
    default = run()
    m.enable_fp8_attention(smooth_v=False)
    assert torch.equal(run(), default)                                # without the argument: the plain path, bit for bit
    m.enable_fp8_attention(smooth_v=True)
    assert m.fp8_smooth_v is True and m.fp8_smooth_k is False
    smooth = run()
    assert torch.equal(run(), smooth) and not torch.equal(smooth, default)            # deterministic, and the switch reaches the kernel
    r, rp = rel_rms(smooth, ref.float()), rel_rms(default, ref.float())
    print(f"{name}: fp8 attention vs own bf16 forward rel-RMS: smooth V {r:.4e}  plain {rp:.4e}")
    record(f"{name}[fp8-attention-smooth-v-vs-own-bf16]", f"rel_rms (plain fp8 attention: {rp:.4e})", r, bound)
    assert torch.isfinite(smooth.float()).all() and r < bound, (r, rp)
    m.enable_fp8_attention(False)
    assert torch.equal(run(), ref)


def _bias_plus_4(name, m, run, biases):
    """a large constant on to_v's bias reaches the quantiser unchanged (no norm, no RoPE), but how much of the model's output error
    it makes on a tiny grid is not known: both errors recorded, no order asserted"""
    with torch.no_grad():
        for bias in biases:
            bias.data += 4.0
    if hasattr(m, "reset_caches"):
        m.reset_caches()
    m.enable_fp8_attention(False)
    ref = run()
    errs = {}
    for smooth_v in (False, True):
        m.enable_fp8_attention(smooth_v=smooth_v)
        out = run()
        assert torch.isfinite(out.float()).all()
        errs[smooth_v] = rel_rms(out, ref.float())
    print(f"{name}, to_v.bias + 4: fp8 attention vs own bf16 rel-RMS: plain {errs[False]:.4e}  smooth V {errs[True]:.4e}")
    record(f"{name}[to_v.bias+4, fp8-attention-smooth-v-vs-own-bf16]", f"rel_rms (plain: {errs[False]:.4e}); recorded only", errs[True], 1.0)


def test_wan_model_with_smooth_v_vs_own_bf16_and_the_default_stays_plain():
    from tests.test_mxfp6_gpu import _wan_tiny
    m, _, _, run = _wan_tiny()
    _check_switch("wan_tiny", m, run, WAN_FP8_BOUND)
    _bias_plus_4("wan_tiny", m, run, [blk.attn1.to_v.bias for blk in m.blocks])


def test_cog_model_with_smooth_v_vs_own_bf16_and_the_default_stays_plain(golden):
    from frameino_amd.cogvideox_transformer_3d import CogVideoXTransformer3DModel
    from tests.test_oracle_golden import _cog_cfg
    cfg, sd, a = golden("cog_dit_tiny")
    cfg = _cog_cfg(cfg)
    assert cfg["attention_head_dim"] == 64                            # (any other head_dim stays on the bf16 kernel)
    m = CogVideoXTransformer3DModel(**cfg).to(DEV)
    m.load_reference_state_dict(sd, dtype=torch.bfloat16)
    m = m.eval()
    run = lambda: m(hidden_states=a["x_def"].to(DEV).bfloat16(), encoder_hidden_states=a["txt_def"].to(DEV).bfloat16(),   # noqa: E731
                    timestep=a["ts_def"].to(DEV), image_rotary_emb=(a["cos_def"].to(DEV), a["sin_def"].to(DEV)),
                    return_dict=False)[0]
    _check_switch("cog_dit_tiny", m, run, COG_FP8_BOUND)
    biases = [blk.attn1.to_v.bias for blk in m.transformer_blocks if getattr(blk.attn1.to_v, "bias", None) is not None]
    if biases:
        _bias_plus_4("cog_dit_tiny", m, run, biases)


@pytest.mark.parametrize("fp8", [dict(smooth_v=True), dict(smooth_k=True, smooth_v=True)], ids=["smooth-v", "smooth-k-v"])
def test_cog_windowed_forward_with_smooth_v_matches_the_restatement(setup, fp8):  # noqa: F811
    """tests/test_window_attention_cog_gpu.py::test_fp8_attention_with_a_window_matches_the_restatement with smooth_v: the windowed
    path passes the switch to ops.attention_fp8_ranges"""
    from tests import test_window_attention_cog_gpu as W
    sd, sdb, inp, dense, _, _ = setup
    windowed = W._ref(sdb, inp[0][:1], inp[1][:1], inp[2][:1], inp[3], W.R.layer_masks(2, W.FRAMES, W.TPF, W.TEXT, 1, W.SINKS))
    m = W._model(sd, fp8=fp8, window_frames=1)
    assert m.fp8_attention and m.fp8_smooth_v is True
    out = W._fwd(m, inp, id_frames=1)
    err, far = rel_rms(out, windowed), rel_rms(out, dense)
    print(f"fp8 attention {fp8} + window: rel-RMS {err:.3e} against the restatement, {far:.3e} against the dense restatement")
    record(f"cog_window_attention[tiny, fp8 attention {fp8}]", f"rel_rms vs the masked restatement (vs the dense one: {far:.3e})",
           err, W.FP8_BOUND)
    assert torch.isfinite(out.float()).all() and err < W.FP8_BOUND
    # the switch reaches the range walk: not the windowed forward without it, and not the dense forward with it
    without = {k: v for k, v in fp8.items() if k != "smooth_v"}
    assert not torch.equal(out, W._fwd(W._model(sd, fp8=without, window_frames=1), inp, id_frames=1))
    assert not torch.equal(out, W._fwd(W._model(sd, fp8=fp8), inp))


def test_wan_denoise_with_both_switches_hip_graph_replay_equals_eager(golden):
    from tests.test_wan_pipeline_gpu import _pipe, _run
    pipe, a = _pipe(golden)
    pipe.transformer.enable_fp8_attention(smooth_k=True, smooth_v=True)
    pipe.use_hip_graph = False
    eager = _run(pipe, a)
    pipe.use_hip_graph = True                  # (True makes a failed capture an error)
    graphed = _run(pipe, a)
    assert torch.isfinite(eager.float()).all() and torch.equal(eager, graphed)
