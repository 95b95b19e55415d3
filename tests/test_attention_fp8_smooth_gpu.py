"""Smooth K of the fp8 attention (fino_attn_fwd_fp8_smooth, csrc/fino_attention_fp8.hip): the mean of K over the keys, per (batch
element, head, channel), is subtracted before K becomes e4m3.  q.(k_j - mu) = q.k_j - q.mu and q.mu is one constant per query
row, which the softmax drops, so nothing else changes.  What is stated and checked:

  * exact properties, on integer-valued keys whose sums and means fp32 holds exactly: a key mean of zero gives the bits of the
    plain call; adding an integer to every key of a channel gives the same bits (and does NOT without smoothing);
  * against fp32 SDPA on keys with a per-channel offset 8 x N(0, 1): within 1.2 x the torch emulation of the same quantisation
    (tests/attn_fp8_ref.py), on inputs where the plain emulation is at least 2 x worse;
  * N(0, 1) keys: the bounds of tests/test_attention_fp8_gpu.py hold with smoothing on;
  * two calls give the same bits (fixed partition, fixed order, no atomics);
  * `enable_fp8_attention(smooth_k=True)` on the tiny Wan and CogVideoX models, the default staying the plain path bit for bit, and
    the hipGraph loop replaying the eager loop's bits."""
import pytest
import torch

from tests.attn_fp8_ref import OFFSET_SHAPES, emulated, offset_inputs, sdpa
from tests.parity import record, rel_rms

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]


@pytest.fixture(params=[(64, 0), (64, 1), (128, 0)], ids=["d64-free-running", "d64-ping-pong", "d128"])
def variant(request):
    """head_dim and main kernel: at head_dim 64 the default (4 waves) and FINO_TUNE_ATTN_FP8_KERNEL = 1; head_dim 128 has one"""
    from frameino_amd import _lib
    dh, knob = request.param
    _lib.lib().fino_tune_set(5, knob)
    yield dh
    _lib.lib().fino_tune_set(5, 0)


def _heads(heads, dh):
    return heads if dh == 64 else max(1, heads // 2)


def _int_inputs(b, heads, dh, lq, lk, dtype, kmax, seed, antisymmetric=False):
    """q = N(0, 1) / 8, v = N(0, 1), K integer-valued in [-kmax, kmax] ([X ; -X] over the keys if antisymmetric), k | v row-strided"""
    d = heads * dh
    g = torch.Generator(device=DEV).manual_seed(seed)
    q = (torch.randn(b, lq, d, device=DEV, generator=g) / 8).to(dtype)
    kv = torch.randn(b, lk, 2 * d + 64, device=DEV, generator=g)
    n = lk // 2 if antisymmetric else lk
    x = torch.randint(-kmax, kmax + 1, (b, n, d), device=DEV, generator=g).float()
    kv[:, :, :d] = torch.cat([x, -x], 1) if antisymmetric else x
    kv = kv.to(dtype)
    return q, kv, d


# ------------------------------------------------------------------ 1. a key mean of exactly zero: the plain call's bits
@pytest.mark.parametrize("lk", [128, 640])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("p_mode", ["exp2", "ramp"])
def test_zero_key_mean_gives_the_bits_of_the_plain_call(variant, p_mode, dtype, lk):
    """K = [X ; -X] with integer X in [-4, 4]: every partial sum is an fp32 integer in any order, so the mean is exactly 0"""
    from frameino_amd import ops
    dh, heads = variant, _heads(4, variant)
    q, kv, d = _int_inputs(2, heads, dh, 100, lk, dtype, 4, 17 + lk, antisymmetric=True)
    k, v = kv[:, :, :d], kv[:, :, d:2 * d]
    assert not k.float().sum(1).any()
    plain = ops.attention_fp8(q, k, v, heads, p_mode=p_mode, smooth_k=False)
    smooth = ops.attention_fp8(q, k, v, heads, p_mode=p_mode, smooth_k=True)
    assert torch.isfinite(plain.float()).all() and torch.equal(smooth, plain)


# ------------------------------------------------------------------ 2. K + c and K: the same bits
@pytest.mark.parametrize("lk", [256, 1024])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("p_mode", ["exp2", "ramp"])
def test_an_integer_offset_per_channel_changes_no_bit(variant, p_mode, dtype, lk):
    """K integer in [-8, 8], c integer in [-64, 64] per (batch element, channel), lk a power of two: K + c is exact in bf16 / fp16
    (|.| <= 72), the sums are exact in fp32 (<= 1024 x 72), the division by lk is exact, and (K + c) - (mean + c) = K - mean needs
    8 + 10 bits: the quantiser sees the same numbers.  Without smoothing the offset reaches e4m3 and the bits change."""
    from frameino_amd import ops
    dh, heads = variant, _heads(4, variant)
    q, kv, d = _int_inputs(2, heads, dh, 100, lk, dtype, 8, 29 + lk)
    g = torch.Generator(device=DEV).manual_seed(31)
    c = torch.randint(-64, 65, (2, 1, d), device=DEV, generator=g).float()
    kvc = kv.clone()
    kvc[:, :, :d] = (kv[:, :, :d].float() + c).to(dtype)
    assert torch.equal(kvc[:, :, :d].float(), kv[:, :, :d].float() + c)              # (exact in the storage type)
    k, kc, v = kv[:, :, :d], kvc[:, :, :d], kv[:, :, d:2 * d]
    base = ops.attention_fp8(q, k, v, heads, p_mode=p_mode, smooth_k=True)
    shifted = ops.attention_fp8(q, kc, v, heads, p_mode=p_mode, smooth_k=True)
    assert torch.isfinite(base.float()).all() and torch.equal(shifted, base)
    assert not torch.equal(ops.attention_fp8(q, kc, v, heads, p_mode=p_mode, smooth_k=False),
                           ops.attention_fp8(q, k, v, heads, p_mode=p_mode, smooth_k=False))


# ------------------------------------------------------------------ 3. keys with a channel offset, against fp32 SDPA
@pytest.mark.parametrize("b,heads,lq,lk", OFFSET_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("p_mode", ["exp2", "ramp"])
def test_offset_keys_vs_fp32_and_vs_the_smoothed_emulation(variant, p_mode, dtype, b, heads, lq, lk):
    from frameino_amd import ops
    dh, heads = variant, _heads(heads, variant)
    q, k, v = offset_inputs(b, heads, lq, lk, dh, dtype, DEV)
    ref = sdpa(q, k, v, heads)
    re, rpe = rel_rms(emulated(q, k, v, heads, p_mode, smooth_k=True), ref), rel_rms(emulated(q, k, v, heads, p_mode), ref)
    assert rpe >= 2 * re, (rpe, re)                    # the condition on the inputs: the offset does cost the plain quantiser
    o = ops.attention_fp8(q, k, v, heads, p_mode=p_mode, smooth_k=True)
    rp = rel_rms(ops.attention_fp8(q, k, v, heads, p_mode=p_mode), ref)
    r = rel_rms(o, ref)
    name = f"attention_fp8_smooth_offset_keys[{p_mode}-b{b}-h{heads}x{dh}-lq{lq}-lk{lk}-{str(dtype)[6:]}]"
    print(f"{name}: smoothed kernel {r:.4f}  smoothed emulation {re:.4f}  plain kernel {rp:.4f}  plain emulation {rpe:.4f}")
    record(name, f"rel_rms vs fp32 SDPA (smoothed emulation {re:.4f}; plain kernel {rp:.4f}, plain emulation {rpe:.4f})", r,
           1.2 * re + 2e-3)
    assert torch.isfinite(o.float()).all() and r < 1.2 * re + 2e-3, (r, re)


# ------------------------------------------------------------------ 4. N(0, 1) keys: nothing lost
@pytest.mark.parametrize("b,heads,lq,lk", [(1, 2, 256, 256), (2, 3, 300, 1000), (1, 8, 1000, 777)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("p_mode", ["exp2", "ramp"])
def test_standard_normal_keys_keep_the_bounds_of_the_plain_path(variant, p_mode, dtype, b, heads, lq, lk):
    from frameino_amd import ops
    dh, heads = variant, _heads(heads, variant)
    d = heads * dh
    g = torch.Generator(device=DEV).manual_seed(lq + lk + heads)
    q = torch.randn(b, lq, d, device=DEV, generator=g).to(dtype)
    kv = torch.randn(b, lk, 2 * d + 64, device=DEV, generator=g).to(dtype)          # row-strided k | v views
    k, v = kv[:, :, :d], kv[:, :, d:2 * d]
    out = torch.zeros(b, lq + 7, d, device=DEV, dtype=dtype)
    o = ops.attention_fp8(q, k, v, heads, out=out[:, :lq], p_mode=p_mode, smooth_k=True)
    assert torch.isfinite(o.float()).all() and not out[:, lq:].any()
    ref = sdpa(q, k, v, heads)
    r, re = rel_rms(o, ref), rel_rms(emulated(q, k, v, heads, p_mode, smooth_k=True), ref)
    record(f"attention_fp8_smooth[{p_mode}-b{b}-h{heads}x{dh}-lq{lq}-lk{lk}-{str(dtype)[6:]}]",
           f"rel_rms vs fp32 SDPA (smoothed emulation: {re:.4f})", r, 8e-2)
    assert r < 8e-2 and r < 1.2 * re + 2e-3, (r, re)
    o1 = ops.attention_fp8(q, k, torch.ones_like(v), heads, p_mode=p_mode, smooth_k=True)
    assert (o1.float() - 1).abs().max().item() < 4e-3


# ------------------------------------------------------------------ 5. the same inputs, the same bits
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_two_calls_give_the_same_bits(variant, dtype):
    from frameino_amd import ops
    dh, heads = variant, _heads(3, variant)
    q, k, v = offset_inputs(2, heads, 300, 1000, dh, dtype, DEV)
    first = ops.attention_fp8(q, k, v, heads, smooth_k=True).clone()
    assert torch.equal(ops.attention_fp8(q, k, v, heads, smooth_k=True), first)


# ------------------------------------------------------------------ 6. models and the denoise loop
# bounds against the model's own bf16 forward: the ones tests/test_fullsize_oracle_gpu.py states for `enable_fp8_attention()`
# (Wan: 1.5e-2, test_wan_two_layer_forward_full_size_with_fp8_attention_vs_oracle_on_device; CogVideoX: FP8_ATTN_BOUND = 6e-2)
WAN_FP8_BOUND, COG_FP8_BOUND = 1.5e-2, 6e-2


def _check_switch(name, m, run, bound):
    ref = run()
    m.enable_fp8_attention()
    assert m.fp8_attention and m.fp8_smooth_k is False
    default = run()
    m.enable_fp8_attention(smooth_k=False)
    assert torch.equal(run(), default)                                # without the argument: the plain path, bit for bit
    m.enable_fp8_attention(smooth_k=True)
    assert m.fp8_smooth_k is True
    smooth = run()
    assert torch.equal(run(), smooth) and not torch.equal(smooth, default)            # (the switch does reach the kernel)
    r, rp = rel_rms(smooth, ref.float()), rel_rms(default, ref.float())
    print(f"{name}: fp8 attention vs own bf16 forward rel-RMS: smooth K {r:.4e}  plain {rp:.4e}")
    record(f"{name}[fp8-attention-smooth-k-vs-own-bf16]", f"rel_rms (plain fp8 attention: {rp:.4e})", r, bound)
    assert torch.isfinite(smooth.float()).all() and r < bound, (r, rp)
    m.enable_fp8_attention(False)
    assert torch.equal(run(), ref)


def test_wan_model_with_smooth_k_vs_own_bf16_and_the_default_stays_plain():
    from tests.test_mxfp6_gpu import _wan_tiny
    m, _, _, run = _wan_tiny()
    _check_switch("wan_tiny", m, run, WAN_FP8_BOUND)
    # a large constant on to_k's bias: whether it survives norm_k + RoPE on a tiny grid is not known -- recorded, no order asserted
    with torch.no_grad():
        for blk in m.blocks:
            blk.attn1.to_k.bias.data += 4.0
    m.reset_caches()
    ref = run()
    errs = {}
    for smooth_k in (False, True):
        m.enable_fp8_attention(smooth_k=smooth_k)
        errs[smooth_k] = rel_rms(run(), ref.float())
    print(f"wan_tiny, to_k.bias + 4: fp8 attention vs own bf16 rel-RMS: plain {errs[False]:.4e}  smooth K {errs[True]:.4e}")
    record("wan_tiny[to_k.bias+4, fp8-attention-smooth-k-vs-own-bf16]", f"rel_rms (plain: {errs[False]:.4e}); recorded only", errs[True], 1.0)


def test_cog_model_with_smooth_k_vs_own_bf16_and_the_default_stays_plain(golden):
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


def test_wan_denoise_with_smooth_k_hip_graph_replay_equals_eager(golden):
    from tests.test_wan_pipeline_gpu import _pipe, _run
    pipe, a = _pipe(golden)
    pipe.transformer.enable_fp8_attention(smooth_k=True)
    pipe.use_hip_graph = False
    eager = _run(pipe, a)
    pipe.use_hip_graph = True                  # (True makes a failed capture an error)
    graphed = _run(pipe, a)
    assert torch.isfinite(eager.float()).all() and torch.equal(eager, graphed)
