"""Smooth Q of the fp8 attention (fino_attn_fwd_fp8_smooth_q, csrc/fino_attention_fp8.hip): the mean of q over each block of 256
consecutive query rows, per (batch element, head, channel), leaves q before it becomes e4m3, and qbar . k_key -- fp32, from the
unquantised keys, one number per (q-block, key) -- joins the logits again on the matrix pipe.  s_ij = (q_i - qbar) . k_j + qbar . k_j
is exact.  What is stated and checked, at head_dim 64 (always the free-running kernel, whatever the tuning knob says) and 128,
bf16 and fp16, both p_modes:

  * exact properties on integer queries: block means of zero give the bits of the call without smooth Q; an integer offset of
    +-2^15 per (block, head, channel) on channels where K - mu is exactly 0 changes no bit with smooth Q (and does without): a mean over the
    wrong rows or axis, a ragged block divided by 256, a sub-head reading the other half's means, padded rows taking -qbar all show;
  * the bias alone: all rows of a block equal, so every logit comes from the table -- within 1.2 x the smoothed emulation against
    fp32 SDPA; a table indexed by the wrong key, block, head or batch element misses that by an order of magnitude;
  * offset queries (q + 8 N(0, 1) per (256-row block, head, channel)) on the three shapes of tests/attn_fp8_smooth_q_ref.py:
    within 1.2 x the smoothed emulation (the factor the smooth-K tests use), on inputs where the plain emulation is >= 2 x worse
    (tests/test_attention_fp8_smooth_q_cpu.py asserts that condition);
  * N(0, 1) operands keep the plain path's bounds; two calls give the same bits; every combination with smooth_k / smooth_v is
    close to the emulation with the same flags;
  * `enable_fp8_attention(smooth_q=True)` on the tiny Wan and CogVideoX models within the smooth-K / smooth-V model bounds, the
    default staying the plain path bit for bit, and the Wan hipGraph loop replaying the eager loop's bits."""
import pytest
import torch

from tests.attn_fp8_smooth_q_ref import (CONDITION, CONDITION_SHAPES, Q_BLOCK, SHAPES, block_constant_inputs, emulated, heads_at,
                                         offset_q_inputs, sdpa)
from tests.parity import record, rel_rms
from tests.test_attention_fp8_smooth_gpu import COG_FP8_BOUND, WAN_FP8_BOUND

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
dtypes = pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
p_modes = pytest.mark.parametrize("p_mode", ["exp2", "ramp"])
head_dims = pytest.mark.parametrize("dh", [64, 128], ids=["d64", "d128"])
FLAGS = [dict(), dict(smooth_k=True), dict(smooth_v=True), dict(smooth_k=True, smooth_v=True)]


def _name(tag, p_mode, b, heads, dh, lq, lk, dtype):
    return f"attention_fp8_smooth_q_{tag}[{p_mode}-b{b}-h{heads}x{dh}-lq{lq}-lk{lk}-{str(dtype)[6:]}]"


# ------------------------------------------------------------------ 1 / 2. exact properties on integer queries
def _integer_case(b, heads, dh, lq, lk, dtype, seed, const_channels=None):
    """integer queries in [-4, 4] whose column sums over every 256-row block are exactly zero (+- pairs of rows, a zero row where the
    block's row count is odd), integer keys in [-4, 4], v = N(0, 1).  const_channels: those channels of K are one integer per channel
    over all keys, so with smooth_k K - mu is exactly 0 there."""
    d = heads * dh
    g = torch.Generator().manual_seed(seed)
    q = torch.zeros(b, lq, d)
    for r0 in range(0, lq, Q_BLOCK):
        n = min(Q_BLOCK, lq - r0)
        x = torch.randint(-4, 5, (b, n // 2, d), generator=g).float()
        q[:, r0:r0 + n // 2] = x
        q[:, r0 + n // 2:r0 + 2 * (n // 2)] = -x                      # (an odd block keeps its last row zero)
    kv = torch.randn(b, lk, 2 * d + 64, generator=g)
    kv[:, :, :d] = torch.randint(-4, 5, (b, lk, d), generator=g).float()
    if const_channels is not None:
        kv[:, :, :d][:, :, const_channels] = torch.randint(1, 4, (int(const_channels.sum()),), generator=g).float()
    for r0 in range(0, lq, Q_BLOCK):
        assert not q[:, r0:r0 + Q_BLOCK].sum(1).any()
    kv = kv.to(dtype).to(DEV)
    return q.to(dtype).to(DEV), kv[:, :, :d], kv[:, :, d:2 * d]


@pytest.mark.parametrize("b,heads,lq,lk", SHAPES)
@head_dims
@dtypes
@p_modes
def test_zero_block_means_give_the_bits_of_the_call_without_smooth_q(p_mode, dtype, dh, b, heads, lq, lk):
    """qbar = 0 exactly (integer sums are exact in any order), so q - qbar = q, every table entry is a zero pair and the fold adds
    0.0 to the logits: the same bits as the call without smooth Q, under every combination of the other two switches"""
    from frameino_amd import ops
    heads = heads_at(heads, dh)
    q, k, v = _integer_case(b, heads, dh, lq, lk, dtype, 11 + lq + lk + dh)
    for kw in FLAGS:
        plain = ops.attention_fp8(q, k, v, heads, p_mode=p_mode, **kw)
        assert torch.isfinite(plain.float()).all() and plain.float().abs().max() > 0
        got = ops.attention_fp8(q, k, v, heads, p_mode=p_mode, smooth_q=True, **kw)
        assert torch.equal(got, plain), (kw, (got != plain).nonzero()[:4].tolist())


@pytest.mark.parametrize("b,heads,lq,lk", SHAPES)
@head_dims
@dtypes
@p_modes
def test_an_offset_that_q_alone_carries_changes_no_bit(p_mode, dtype, dh, b, heads, lq, lk):
    """On a third of the channels (some in every 32-channel block of every sub-head) K is one integer per channel over all keys, so
    with smooth_k K - mu is exactly 0 there; the base q is 0 on them and integers / 16 elsewhere (a power-of-two unit: sums stay
    exact).  q gets an offset of +-2^15 per (block, head, channel) on those channels.  With smooth_q the block mean IS the offset
    (sums of up to 256 x 2^15 and their division by the block's real row count are exact in fp32), q - qbar is the base q, and the
    offset's logits are offset x 0: the base call's bits.
    Why 2^15 against |q| <= 1/4 and not a few times |q|: the e8m0 scale is a power of two, so an offset that only moves the scale
    rounds the other channels of its block to the same e4m3 numbers -- until they leave e4m3's normal range.  With the block's amax
    at 2^15 the scaled amax lies in (224, 448], so base values of 1/16 .. 1/4 land in (2^-11.2, 2^-8.2): in e4m3's subnormal range
    (fixed step 2^-9), where they keep one bit or none.  So without smooth_q the base channels are rounded away and the output
    moves (the torch emulation: > 95 % of the output elements); 2^15 is exact in bf16 and in fp16."""
    from frameino_amd import ops
    heads = heads_at(heads, dh)
    d = heads * dh
    const = (torch.arange(d) % 3) == 1
    q, k, v = _integer_case(b, heads, dh, lq, lk, dtype, 23 + lq + lk + dh, const_channels=const)
    q = q.float() / 16
    q[:, :, const.to(DEV)] = 0                                          # (column sums stay zero)
    q = q.to(dtype)
    g = torch.Generator().manual_seed(5 + lq + dh)
    nqb = -(-lq // Q_BLOCK)
    off = (32768.0 * (2 * torch.randint(0, 2, (nqb, d), generator=g) - 1)) * const             # differs per block, head, channel
    qo = (q.float().cpu() + off.repeat_interleave(Q_BLOCK, 0)[:lq]).to(dtype).to(DEV)
    assert torch.equal(qo.float().cpu(), q.float().cpu() + off.repeat_interleave(Q_BLOCK, 0)[:lq])       # exact in the storage type
    for kw in (dict(smooth_k=True), dict(smooth_k=True, smooth_v=True)):
        base = ops.attention_fp8(q, k, v, heads, p_mode=p_mode, **kw)
        assert torch.isfinite(base.float()).all() and base.float().abs().max() > 0
        got = ops.attention_fp8(qo, k, v, heads, p_mode=p_mode, smooth_q=True, **kw)
        assert torch.equal(got, base), (kw, (got != base).nonzero()[:4].tolist())
        assert not torch.equal(ops.attention_fp8(qo, k, v, heads, p_mode=p_mode, **kw), base)


# ------------------------------------------------------------------ 3. the bias alone
@pytest.mark.parametrize("b,heads,lq,lk", [(2, 3, 600, 1000), (2, 2, 300, 320)])
@head_dims
@dtypes
@p_modes
def test_the_bias_table_alone_carries_the_logits(p_mode, dtype, dh, b, heads, lq, lk):
    """all rows of a 256-row block equal (another N(0, 1) row per batch element, block, head): q - qbar = 0 and every logit is a
    table entry.  Three blocks (the last ragged), two batch elements, several heads, a ragged last key tile."""
    from frameino_amd import ops
    heads = heads_at(heads, dh)
    q, k, v = block_constant_inputs(b, heads, lq, lk, dh, dtype, DEV)
    ref = sdpa(q, k, v, heads)
    got = ops.attention_fp8(q, k, v, heads, p_mode=p_mode, smooth_q=True)
    r, re = rel_rms(got, ref), rel_rms(emulated(q, k, v, heads, p_mode, smooth_q=True), ref)
    print(f"bias alone {(b, heads, dh, lq, lk)} {dtype} {p_mode}: kernel {r:.5f} emulation {re:.5f}")
    record(_name("bias_alone", p_mode, b, heads, dh, lq, lk, dtype), f"rel_rms vs fp32 SDPA (smoothed emulation {re:.5f})", r, 1.2 * re)
    assert torch.isfinite(got.float()).all() and r <= 1.2 * re, (r, re)


# ------------------------------------------------------------------ 4. offset queries, N(0, 1) operands
@pytest.mark.parametrize("b,heads,lq,lk", SHAPES)
@head_dims
@dtypes
@p_modes
def test_offset_queries_vs_fp32_and_vs_the_smoothed_emulation(p_mode, dtype, dh, b, heads, lq, lk):
    """q = N(0, 1) + 8 N(0, 1) per (256-row block, head, channel).  Bound: 1.2 x the smoothed emulation, no additive term.  On the
    first two shapes the plain emulation is >= 2 x worse (asserted here as well); (33, 65) is nearly one-hot: closeness only."""
    from frameino_amd import ops
    condition = (b, heads, lq, lk) in CONDITION_SHAPES
    heads = heads_at(heads, dh)
    q, k, v = offset_q_inputs(b, heads, lq, lk, dh, dtype, DEV)
    ref = sdpa(q, k, v, heads)
    re, rpe = rel_rms(emulated(q, k, v, heads, p_mode, smooth_q=True), ref), rel_rms(emulated(q, k, v, heads, p_mode), ref)
    got = ops.attention_fp8(q, k, v, heads, p_mode=p_mode, smooth_q=True)
    r, rp = rel_rms(got, ref), rel_rms(ops.attention_fp8(q, k, v, heads, p_mode=p_mode), ref)
    print(f"offset q {(b, heads, dh, lq, lk)} {dtype} {p_mode}: smoothed kernel {r:.5f} emulation {re:.5f}  plain kernel {rp:.5f} "
          f"emulation {rpe:.5f}")
    record(_name("offset_queries", p_mode, b, heads, dh, lq, lk, dtype),
           f"rel_rms vs fp32 SDPA (smoothed emulation {re:.5f}; plain kernel {rp:.5f}, plain emulation {rpe:.5f})", r, 1.2 * re)
    if condition:
        assert rpe >= CONDITION * re, (rpe, re)
    assert torch.isfinite(got.float()).all() and r <= 1.2 * re, (r, re, rp, rpe)


@pytest.mark.parametrize("b,heads,lq,lk", [(1, 2, 256, 256), (2, 3, 300, 1000), (1, 8, 1000, 777)])
@head_dims
@dtypes
@p_modes
def test_standard_normal_operands_keep_the_bounds_of_the_plain_path(p_mode, dtype, dh, b, heads, lq, lk):
    """tests/test_attention_fp8_gpu.py's bounds (rel-RMS < 8e-2 and < 1.2 x the emulation + 2e-3); rows past lq of a larger `out`
    stay untouched"""
    from frameino_amd import ops
    heads = heads_at(heads, dh)
    d = heads * dh
    g = torch.Generator(device=DEV).manual_seed(lq + lk + heads + 5)
    q = torch.randn(b, lq, d, device=DEV, generator=g).to(dtype)
    kv = torch.randn(b, lk, 2 * d + 64, device=DEV, generator=g).to(dtype)
    k, v = kv[:, :, :d], kv[:, :, d:2 * d]
    ref = sdpa(q, k, v, heads)
    out = torch.full((b, lq + 7, d), 3.0, device=DEV, dtype=dtype)
    o = ops.attention_fp8(q, k, v, heads, out=out[:, :lq], p_mode=p_mode, smooth_q=True)
    assert torch.isfinite(o.float()).all() and (out[:, lq:] == 3.0).all()
    r, re = rel_rms(o, ref), rel_rms(emulated(q, k, v, heads, p_mode, smooth_q=True), ref)
    record(_name("normal", p_mode, b, heads, dh, lq, lk, dtype), f"rel_rms vs fp32 SDPA (smoothed emulation: {re:.4f})", r, 8e-2)
    assert r < 8e-2 and r < 1.2 * re + 2e-3, (r, re)


# ------------------------------------------------------------------ 5 / 6. determinism, flag combinations, the tuning knob
@head_dims
@dtypes
def test_two_calls_give_the_same_bits(dtype, dh):
    from frameino_amd import ops
    heads = heads_at(3, dh)
    q, k, v = offset_q_inputs(2, heads, 300, 1000, dh, dtype, DEV)
    for kw in (dict(), dict(smooth_k=True, smooth_v=True)):
        first = ops.attention_fp8(q, k, v, heads, smooth_q=True, **kw).clone()
        assert torch.equal(ops.attention_fp8(q, k, v, heads, smooth_q=True, **kw), first)


@pytest.mark.parametrize("kw", FLAGS[1:], ids=["k", "v", "k-v"])
@head_dims
@dtypes
@p_modes
def test_flag_combinations_are_close_to_the_emulation_with_the_same_flags(p_mode, dtype, dh, kw):
    from frameino_amd import ops
    b, heads, lq, lk = SHAPES[1]
    heads = heads_at(heads, dh)
    q, k, v = offset_q_inputs(b, heads, lq, lk, dh, dtype, DEV)
    ref = sdpa(q, k, v, heads)
    got = ops.attention_fp8(q, k, v, heads, p_mode=p_mode, smooth_q=True, **kw)
    r, re = rel_rms(got, ref), rel_rms(emulated(q, k, v, heads, p_mode, smooth_q=True, **kw), ref)
    print(f"flags {kw} dh {dh} {dtype} {p_mode}: kernel {r:.5f} emulation {re:.5f}")
    assert torch.isfinite(got.float()).all() and r <= 1.2 * re, (kw, r, re)


@dtypes
def test_head_dim_64_takes_the_free_running_kernel_whatever_the_tuning_knob_says(dtype):
    from frameino_amd import _lib, ops
    q, k, v = offset_q_inputs(2, 3, 300, 1000, 64, dtype, DEV)
    want = ops.attention_fp8(q, k, v, 3, smooth_q=True).clone()
    _lib.lib().fino_tune_set(5, 1)
    try:
        assert torch.equal(ops.attention_fp8(q, k, v, 3, smooth_q=True), want)
    finally:
        _lib.lib().fino_tune_set(5, 0)


# ------------------------------------------------------------------ 7. models and the denoise loop
def _check_switch(name, m, run, bound):
    ref = run()
    m.enable_fp8_attention()
    assert m.fp8_attention and m.fp8_smooth_q is False
    default = run()
    m.enable_fp8_attention(smooth_q=False)
    assert torch.equal(run(), default)                                # without the switch: the plain path, bit for bit
    m.enable_fp8_attention(smooth_q=True)
    assert m.fp8_smooth_q is True and m.fp8_smooth_k is False and m.fp8_smooth_v is False
    smooth = run()
    assert torch.equal(run(), smooth) and not torch.equal(smooth, default)            # deterministic, and the switch reaches the kernel
    r, rp = rel_rms(smooth, ref.float()), rel_rms(default, ref.float())
    print(f"{name}: fp8 attention vs own bf16 forward rel-RMS: smooth Q {r:.4e}  plain {rp:.4e}")
    record(f"{name}[fp8-attention-smooth-q-vs-own-bf16]", f"rel_rms (plain fp8 attention: {rp:.4e})", r, bound)
    assert torch.isfinite(smooth.float()).all() and r < bound, (r, rp)
    m.enable_fp8_attention(smooth_k=True, smooth_v=True, smooth_q=True)
    r3 = rel_rms(run(), ref.float())
    print(f"{name}: all three switches {r3:.4e}")
    assert r3 < bound, r3
    m.enable_fp8_attention(False)
    assert torch.equal(run(), ref)


def test_wan_model_with_smooth_q_vs_own_bf16_and_the_default_stays_plain():
    from tests.test_mxfp6_gpu import _wan_tiny
    m, _, _, run = _wan_tiny()
    _check_switch("wan_tiny", m, run, WAN_FP8_BOUND)


def test_cog_model_with_smooth_q_vs_own_bf16_and_the_default_stays_plain(golden):
    from frameino_amd.cogvideox_transformer_3d import CogVideoXTransformer3DModel
    from tests.test_oracle_golden import _cog_cfg
    cfg, sd, a = golden("cog_dit_tiny")
    cfg = _cog_cfg(cfg)
    assert cfg["attention_head_dim"] == 64
    m = CogVideoXTransformer3DModel(**cfg).to(DEV)
    m.load_reference_state_dict(sd, dtype=torch.bfloat16)
    m = m.eval()
    run = lambda: m(hidden_states=a["x_def"].to(DEV).bfloat16(), encoder_hidden_states=a["txt_def"].to(DEV).bfloat16(),   # noqa: E731
                    timestep=a["ts_def"].to(DEV), image_rotary_emb=(a["cos_def"].to(DEV), a["sin_def"].to(DEV)),
                    return_dict=False)[0]
    _check_switch("cog_dit_tiny", m, run, COG_FP8_BOUND)


def test_wan_denoise_with_smooth_q_hip_graph_replay_equals_eager(golden):
    from tests.test_wan_pipeline_gpu import _pipe, _run
    pipe, a = _pipe(golden)
    pipe.transformer.enable_fp8_attention(smooth_k=True, smooth_v=True, smooth_q=True)
    pipe.use_hip_graph = False
    eager = _run(pipe, a)
    pipe.use_hip_graph = True                  # (True makes a failed capture an error)
    graphed = _run(pipe, a)
    assert torch.isfinite(eager.float()).all() and torch.equal(eager, graphed)
