"""MXFP6 (e2m3) linear path: the quantiser bit for bit against the torch restatement of the rule (tests/mxfp6_ref.py), the
scaled-MFMA GEMM against fp32 matmul on the DECODED operands (exact up to fp32 summation order and output rounding), the
end-to-end error against the model-dtype GEMM it replaces and against MXFP8 on the same operands, and the models with
`enable_mxfp6_linears()` against their own bf16 and MXFP8 forwards."""
import pytest
import torch

from tests import mxfp6_ref as R
from tests.parity import rel_rms

pytestmark = pytest.mark.gpu
DEV = "cuda"


def decoded(q, s, rows, cols):
    return R.decode(*R.unpack(q, s, rows, cols))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("rows,cols", [(300, 256), (77, 1024), (512, 3072), (24640, 3072)])
def test_quantize_equals_the_rule_bit_for_bit(rows, cols, dtype):
    from frameino_amd import ops
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(rows, cols, generator=g) * torch.exp2(torch.randint(-6, 6, (rows, 1), generator=g).float())).to(dtype)
    x[0, :32] = 0                                                     # an all-zero block
    q, s = ops.quantize_mxfp6(x.to(DEV))
    codes, e = R.unpack(q, s, rows, cols)
    codes_ref, e_ref = R.quantize_ref(x)
    assert torch.equal(e, e_ref)
    assert torch.equal(codes, codes_ref)


def test_quantize_strided_rows_and_scale_boundaries():
    """a row-strided view quantises like its contiguous copy, and block maxima exactly at and next to 7.5 * 2^k take the
    exponent the rule gives (the boundary an approximate reciprocal would move)"""
    from frameino_amd import ops
    g = torch.Generator().manual_seed(4)
    big = torch.randn(40, 640, generator=g).bfloat16()
    for k, col in zip((-9, -1, 0, 6), (0, 32, 64, 96)):
        big[:, col:col + 32] *= 0.1 * 2.0 ** k
        big[1, col] = 7.5 * 2.0 ** k
        big[2, col] = -7.75 * 2.0 ** k
        big[3, col] = 3.75 * 2.0 ** k
    view = big.to(DEV)[:, 128:512]
    q, s = ops.quantize_mxfp6(view)
    codes, e = R.unpack(q, s, 40, 384)
    codes_ref, e_ref = R.quantize_ref(big[:, 128:512])
    assert torch.equal(e, e_ref) and torch.equal(codes, codes_ref)
    big0 = big.to(DEV)[:, :128].contiguous()
    codes, e = R.unpack(*ops.quantize_mxfp6(big0), 40, 128)
    codes_ref, e_ref = R.quantize_ref(big[:, :128])
    assert torch.equal(e, e_ref) and torch.equal(codes, codes_ref)
    assert e[1, :4].tolist() == [-9, -1, 0, 6] and e[2, :4].tolist() == [-8, 0, 1, 7] and e[3, :4].tolist() == [-10, -2, -1, 5]


FIVE = [(256, 256, 128, 0), (300, 520, 384, 0), (1000, 768, 1024, 1), (513, 256, 2048, 3), (2048, 3072, 3072, 2)]


def _operands(m, n, k, epi, dtype, seed=2):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(m, k, generator=g).to(dtype).to(DEV)
    w = (torch.randn(n, k, generator=g) * 0.05).to(dtype).to(DEV)
    bias = torch.randn(n, generator=g).to(dtype).to(DEV)
    res = torch.randn(m, n, generator=g).to(dtype).to(DEV) if epi >= 2 else None
    gate = torch.randn(2, n, generator=g).to(DEV) if epi >= 3 else None
    sel = (torch.arange(m) % 2).to(torch.int32).to(DEV) if epi >= 3 else None
    return a, w, bias, res, gate, sel


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("m,n,k,epi", FIVE)
def test_gemm_mxfp6_vs_decoded_fp32(m, n, k, epi, dtype):
    from frameino_amd import ops
    from tests.test_kernels_gpu import gemm_ref
    a, w, bias, res, gate, sel = _operands(m, n, k, epi, dtype)
    aq, sa = ops.quantize_mxfp6(a)
    wq, sw = ops.quantize_mxfp6(w)
    out = ops.gemm_mxfp6(aq, sa, wq, sw, bias, epi, res, gate, sel, out_dtype=dtype)
    assert out.dtype == dtype and out.shape == (m, n)
    ref = gemm_ref(decoded(aq, sa, m, k).to(DEV), decoded(wq, sw, n, k).to(DEV), bias, epi, res, gate, sel)
    r = rel_rms(out, ref.float())
    print(f"[{m}x{n}x{k} epi {epi} {dtype}] mxfp6 GEMM vs fp32 matmul of the decoded operands: rel-RMS {r:.3e}")
    assert r < 2.0 ** -7                                              # output rounding and fp32 summation order only


def _mx_cases(n, seed):
    import random
    rng = random.Random(seed)
    return [(rng.choice([rng.randint(1, 700), 256 * rng.randint(1, 5), 256 * rng.randint(1, 5) + 3]),
             8 * rng.randint(1, 200), 128 * rng.randint(1, 20), rng.randint(0, 4)) for _ in range(n)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", _mx_cases(16, 606), ids=lambda c: "m%d_n%d_k%d_e%d" % c)
def test_gemm_mxfp6_random_shapes(case, dtype):
    from frameino_amd import ops
    from tests.test_kernels_gpu import gemm_ref
    m, n, k, epi = case
    g = torch.Generator(device=DEV).manual_seed(sum(case))
    a = torch.randn(m, k, device=DEV, generator=g).to(dtype)
    w = (torch.randn(n, k, device=DEV, generator=g) * 0.05).to(dtype)
    bias = torch.randn(n, device=DEV, generator=g).to(dtype)
    res = torch.randn(m, n, device=DEV, generator=g).to(dtype) if epi >= 2 else None
    gate = torch.randn(2, n, device=DEV, generator=g) if epi >= 3 else None
    sel = torch.randint(0, 2, (m,), device=DEV, generator=g).to(torch.int32) if epi >= 3 else None
    aq, sa = ops.quantize_mxfp6(a)
    wq, sw = ops.quantize_mxfp6(w)
    out = ops.gemm_mxfp6(aq, sa, wq, sw, bias, epi, res, gate, sel, out_dtype=dtype)
    ref = gemm_ref(decoded(aq, sa, m, k).to(DEV), decoded(wq, sw, n, k).to(DEV), bias, epi, res, gate, sel)
    r = rel_rms(out, ref.float())
    print(f"[{m}x{n}x{k} epi {epi} {dtype}] rel-RMS {r:.3e}")
    assert r < 2.0 ** -7


@pytest.mark.parametrize("m,n,k,epi", FIVE)
def test_gemm_mxfp6_vs_the_gemm_it_replaces_and_vs_mxfp8(m, n, k, epi):
    from frameino_amd import ops
    a, w, bias, res, gate, sel = _operands(m, n, k, epi, torch.bfloat16)
    out6 = ops.gemm_mxfp6(*ops.quantize_mxfp6(a), *ops.quantize_mxfp6(w), bias, epi, res, gate, sel)
    out8 = ops.gemm_mxfp8(*ops.quantize_mxfp8(a), *ops.quantize_mxfp8(w), bias, epi, res, gate, sel)
    full = ops.gemm(a, w, bias, epi, res, gate, sel)
    r6, r8 = rel_rms(out6, full.float()), rel_rms(out8, full.float())
    print(f"[{m}x{n}x{k} epi {epi}] vs bf16 GEMM: mxfp6 rel-RMS {r6:.4f}  mxfp8 rel-RMS {r8:.4f}  ratio {r6 / r8:.3f}")
    assert r6 < 0.06
    assert r6 <= 1.15 * r8


# ------------------------------------------------------------------------------------------------------------ models
def _wan_tiny():
    from oracle import wan_dit as W
    from tests.parity import hip_wan_model
    cfg = dict(W.WAN22_5B_CFG, num_attention_heads=4, attention_head_dim=128, in_channels=16, out_channels=8,
               text_dim=256, ffn_dim=1024, num_layers=3)
    sd = W.wan_random_state_dict(cfg, seed=7, dtype=torch.float32, std=0.04)
    g = torch.Generator().manual_seed(8)
    x = torch.randn(1, 16, 5, 16, 20, generator=g).to(DEV).bfloat16()
    txt = torch.randn(1, 77, 256, generator=g).to(DEV).bfloat16()
    ts = torch.full((1, 5 * 8 * 10), 811.0)
    ts[0, :80] = 0.0
    m = hip_wan_model(cfg, sd, DEV)
    return m, cfg, sd, (lambda: m(x, ts.to(DEV), txt, return_dict=False)[0])


def _check_model_errors(name, e6, e8):
    from tests.parity import record
    print(f"{name}: mxfp6-linears vs own bf16 rel-RMS {e6:.4f}  mxfp8-linears {e8:.4f}  ratio {e6 / e8:.3f}")
    record(f"{name}[mxfp6-vs-own-bf16]", "rel_rms", e6, 1.5 * e8)
    record(f"{name}[mxfp8-vs-own-bf16]", "rel_rms", e8, 1.0)
    assert 1e-4 < e6 <= 1.5 * e8


def test_wan_model_with_mxfp6_linears_vs_own_bf16_and_vs_mxfp8():
    m, _, _, run = _wan_tiny()
    ref = run()
    m.enable_mxfp6_linears()
    assert len(m._fp8) == 6 * 3 and m._mx_fmt == 6
    out6 = run()
    with pytest.raises(ValueError, match="enable_mxfp6_linears"):
        m.enable_mxfp8_linears()                                      # one reduced precision at a time
    m.enable_mxfp6_linears(False)
    assert torch.equal(run(), ref)                                    # back to the model dtype, bit for bit
    m.enable_mxfp8_linears()
    out8 = run()
    with pytest.raises(ValueError, match="enable_mxfp8_linears"):
        m.enable_mxfp6_linears()
    m.enable_mxfp6_linears(False)                                     # the other switch: leaves MXFP8 on
    assert torch.equal(run(), out8)
    m.enable_mxfp8_linears(False)
    assert torch.equal(run(), ref)
    assert not torch.equal(out6, out8)
    _check_model_errors("wan_tiny", rel_rms(out6, ref.float()), rel_rms(out8, ref.float()))


def test_cog_model_with_mxfp6_linears_vs_own_bf16_and_vs_mxfp8(golden):
    from frameino_amd.cogvideox_transformer_3d import CogVideoXTransformer3DModel
    from tests.test_oracle_golden import _cog_cfg
    cfg, sd, a = golden("cog_dit_tiny")
    cfg = _cog_cfg(cfg)
    m = CogVideoXTransformer3DModel(**cfg).to(DEV)
    m.load_reference_state_dict(sd, dtype=torch.bfloat16)
    m = m.eval()
    run = lambda: m(hidden_states=a["x_def"].to(DEV).bfloat16(), encoder_hidden_states=a["txt_def"].to(DEV).bfloat16(),   # noqa: E731
                    timestep=a["ts_def"].to(DEV), image_rotary_emb=(a["cos_def"].to(DEV), a["sin_def"].to(DEV)),
                    return_dict=False)[0]
    ref = run()
    m.enable_mxfp6_linears()
    out6 = run()
    with pytest.raises(ValueError, match="enable_mxfp6_linears"):
        m.enable_mxfp8_linears()
    m.enable_mxfp6_linears(False)
    assert torch.equal(run(), ref)
    m.enable_mxfp8_linears()
    out8 = run()
    with pytest.raises(ValueError, match="enable_mxfp8_linears"):
        m.enable_mxfp6_linears()
    m.enable_mxfp8_linears(False)
    assert torch.equal(run(), ref)
    _check_model_errors("cog_dit_tiny", rel_rms(out6, ref.float()), rel_rms(out8, ref.float()))


def test_lora_merge_requantises_the_mxfp6_weights():
    from tests.test_lora_wan_gpu import diffusers_keys, make_adapter
    m, _, sd, run = _wan_tiny()
    m.enable_mxfp6_linears()
    before = run()
    ad = {}
    for fam in ("attn1_qkv", "attn2_out", "ffn_up", "ffn_down"):
        ad.update(make_adapter(sd, fam))
    m.load_lora_adapter(diffusers_keys(ad))
    merged = run()
    assert m._fp8 and m._mx_fmt == 6                                  # still on the MXFP6 path
    assert not torch.equal(merged, before)                            # the merge reached the quantised weights
    m.enable_mxfp6_linears(False)
    m.enable_mxfp6_linears()                                          # quantised afresh from the merged parameters
    assert torch.equal(run(), merged)


def test_moving_the_model_keeps_the_mxfp6_path():
    m, _, _, run = _wan_tiny()
    m.enable_mxfp6_linears()
    out = run()
    m.to("cpu")
    assert not m._fp8 and m._fp8_pending
    m.to(DEV)
    assert torch.equal(run(), out) and m._fp8 and m._mx_fmt == 6


def test_token_sharded_branch_uses_the_mxfp6_projections():
    import torch.distributed as dist
    from frameino_amd import _lib
    from frameino_amd.configs import WAN22_5B_CFG
    from frameino_amd.parallel import TokenShard
    from frameino_amd.random_init import random_wan_model
    cfg = dict(WAN22_5B_CFG, num_attention_heads=2, num_layers=2, ffn_dim=512, text_dim=128, in_channels=8,
               out_channels=4)
    m = random_wan_model(cfg, torch.device(DEV), seed=5).enable_mxfp6_linears()
    g = torch.Generator(device=DEV).manual_seed(6)
    x = torch.randn(1, 8, 3, 16, 16, device=DEV, generator=g).bfloat16()
    txt = torch.randn(1, 32, 128, device=DEV, generator=g).bfloat16()
    ts = torch.tensor([500.0], device=DEV)
    base = m(hidden_states=x, timestep=ts, encoder_hidden_states=txt, return_dict=False)[0]
    own_group = not dist.is_initialized()
    if own_group:
        dist.init_process_group("gloo", store=dist.HashStore(), rank=0, world_size=1)
    try:
        m.parallel = TokenShard(0, 1, None, force=True)
        sharded = m(hidden_states=x, timestep=ts, encoder_hidden_states=txt, return_dict=False)[0]
        assert (0, "kv") in m._fp8 and (0, "q") in m._fp8           # the sharded projections were quantised ...
        assert m._fp8[(0, "kv")][0].numel() == _lib.lib().fino_mxfp6_bytes(2 * m.inner_dim, m.inner_dim)   # ... as e2m3
    finally:
        m.parallel = None
        if own_group:
            dist.destroy_process_group()
    r = rel_rms(sharded, base.float())
    print(f"token-sharded mxfp6 forward vs unsharded mxfp6 forward: rel-RMS {r:.2e}")
    assert r < 2e-3, r


def test_first_block_cache_at_threshold_zero_equals_mxfp6_without_the_cache():
    from frameino_amd.step_cache import FirstBlockCacheConfig
    from oracle import wan_dit as W
    from tests.parity import hip_wan_model
    cfg = dict(W.WAN22_5B_CFG, num_attention_heads=4, attention_head_dim=128, in_channels=16, out_channels=8, text_dim=256,
               ffn_dim=1024, num_layers=3)
    sd = W.wan_random_state_dict(cfg, seed=11, dtype=torch.float32, std=0.04)
    g = torch.Generator().manual_seed(12)
    x = torch.randn(1, 16, 5, 16, 20, generator=g)
    dx = torch.randn(1, 16, 5, 16, 20, generator=g)
    txt = torch.randn(1, 77, 256, generator=g).to(DEV).bfloat16()
    ts = torch.tensor([811.0]).to(DEV)
    plain = hip_wan_model(cfg, sd, DEV).enable_mxfp6_linears()
    cached = hip_wan_model(cfg, sd, DEV)
    cached.enable_cache(FirstBlockCacheConfig(threshold=0.0))
    cached.enable_mxfp6_linears()

    def fwd(m, xi):
        with m.cache_context("c"):
            return m(xi.to(DEV).bfloat16(), ts, txt, return_dict=False)[0]

    for i in range(2):
        assert torch.equal(fwd(cached, x + 0.2 * i * dx), fwd(plain, x + 0.2 * i * dx))
    assert [e[3] for e in cached.cache_log] == [True, True]


def test_wan5b_two_layer_forward_full_size_mxfp6_vs_own_bf16_and_vs_mxfp8():
    """two layers of Wan2.2-5B at L = 12320 tokens (49 frames 704 x 1280): the shapes the step runs, ragged last tile row"""
    from frameino_amd.configs import WAN22_5B_CFG
    from frameino_amd.random_init import random_wan_model
    cfg = dict(WAN22_5B_CFG, num_layers=2)
    m = random_wan_model(cfg, torch.device(DEV), 0, dtype=torch.bfloat16)
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(1, 96, 14, 44, 80, device=DEV, generator=g).bfloat16()
    pe = torch.randn(1, 512, cfg["text_dim"], device=DEV, generator=g).bfloat16()
    sel = torch.ones(12320, dtype=torch.int32, device=DEV)
    sel[:880] = 0
    rows = (torch.tensor([0.0, 737.0], device=DEV), sel)

    def run():
        with torch.no_grad(), m.cache_context("cond"):
            return m(hidden_states=x, timestep=None, encoder_hidden_states=pe, return_dict=False, timestep_rows=rows)[0]

    ref = run()
    m.enable_mxfp8_linears()
    out8 = run()
    m.enable_mxfp8_linears(False)
    m.enable_mxfp6_linears()
    out6 = run()
    m.enable_mxfp6_linears(False)
    assert torch.isfinite(out6.float()).all() and torch.equal(run(), ref)
    _check_model_errors("wan5b_two_layer_full_size", rel_rms(out6, ref.float()), rel_rms(out8, ref.float()))
