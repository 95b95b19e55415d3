"""Block-Hadamard rotation of the MXFP6 linears on the GPU: `fino_quantize_mxfp6_rot` bit for bit against the torch restatement
(tests/mxfp6_rot_ref.py), `fino_quantize_mxfp6` untouched beside it, the unchanged GEMM on rotated operands against the product
of the decoded restatement and against the full-precision product (the gain on outlier channels, the tensors pinned by
tests/test_mxfp6_rot_cpu.py), and both DiTs with `enable_mxfp6_linears(rotate=True)`."""
import pytest
import torch

from tests import mxfp6_ref as R
from tests import mxfp6_rot_ref as RR
from tests.parity import rel_rms

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])


def _x(rows, cols, dtype, seed=1):
    """rows of very different magnitude, a heavy-tailed row block and an all-zero MX block"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g) * torch.exp2(torch.randint(-6, 6, (rows, 1), generator=g).float())
    x[:, 5::37] *= 24
    x = x.to(dtype)
    x[0, :32] = 0
    return x


# ------------------------------------------------------------------------------------------------------------- quantiser
@DTYPES
@pytest.mark.parametrize("rows,cols", [(1, 128), (37, 256), (300, 384)])
def test_rotated_quantiser_equals_the_restatement_bit_for_bit_and_the_plain_entry_is_what_it_was(rows, cols, dtype):
    from frameino_amd import ops
    x = _x(rows, cols, dtype)
    xd = x.to(DEV)
    strided = torch.zeros(rows, cols + 64, dtype=dtype, device=DEV)
    strided[:, 32:32 + cols] = xd                                     # ldx > cols, the view starts 64 bytes into a row
    view = strided[:, 32:32 + cols]
    got = {}
    for mode in RR.MODES:
        q, s = ops.quantize_mxfp6(xd, rotate=mode)
        codes, e = got[mode] = R.unpack(q, s, rows, cols)
        codes_ref, e_ref = RR.quantize_ref(x, mode)
        assert torch.equal(e, e_ref), f"{mode}: block exponents"
        assert torch.equal(codes, codes_ref), f"{mode}: codes"
        qv, sv = ops.quantize_mxfp6(view, rotate=mode)
        cv, ev = R.unpack(qv, sv, rows, cols)
        assert torch.equal(cv, codes) and torch.equal(ev, e), f"{mode}: strided input"
    assert torch.equal(got["act"][0], got["weight"][0])               # the codes of the two modes are the same
    ea, ew = got["act"][1], got["weight"][1]
    assert torch.equal(ew, (ea - 5).clamp(min=-127)) and int(ea[0, 0]) == -127 and int(ew[0, 0]) == -127
    assert bool((ea[ea > -127] > -100).all())                         # nothing near the clamp but the zero block
    # the unrotated entry, called between the rotated ones, still writes the image of the unrotated rule
    codes, e = R.unpack(*ops.quantize_mxfp6(xd), rows, cols)
    codes_ref, e_ref = R.quantize_ref(x)
    assert torch.equal(e, e_ref) and torch.equal(codes, codes_ref)
    codes_kw, e_kw = R.unpack(*ops.quantize_mxfp6(xd, rotate=None), rows, cols)
    assert torch.equal(codes_kw, codes) and torch.equal(e_kw, e)
    assert not torch.equal(codes, got["act"][0])


@DTYPES
def test_scale_boundaries_are_hit_exactly(dtype):
    """a block with one non-zero element c rotates to +-c in all 32 places: c = 7.5 * 2^k keeps exponent k, the next
    representable value above it takes k + 1; an all-zero block stores byte 0 in both modes"""
    from frameino_amd import ops
    ks = (-9, -1, 0, 6)
    x = torch.zeros(3, 128, dtype=dtype)
    for b, k in enumerate(ks):
        top = torch.tensor(7.5 * 2.0 ** k, dtype=dtype)
        x[0, 32 * b + 3 + 7 * b] = top                                # another position in every block
        x[1, 32 * b + 31 - b] = -(top.view(torch.int16) + 1).view(dtype)                  # one ulp above, negative
    for mode, shift in (("act", 0), ("weight", 5)):
        q, s = ops.quantize_mxfp6(x.to(DEV), rotate=mode)
        codes, e = R.unpack(q, s, 3, 128)
        assert e[0].tolist() == [k - shift for k in ks] and e[1].tolist() == [k + 1 - shift for k in ks]
        assert e[2].tolist() == [-127] * 4 and bool((codes[2] == 0).all())
        assert s.numel() == 256 * 4 and int(s.view(4, 16, 16)[0, 2, 0]) == 0              # the stored byte itself: 0
        assert bool(((codes[0] & 31) == 31).all())                    # every element is the largest magnitude, 7.5
        c_ref, e_ref = RR.quantize_ref(x, mode)
        assert torch.equal(codes, c_ref) and torch.equal(e, e_ref)


def test_wrong_mode_and_shape_are_refused():
    from frameino_amd import _lib, ops
    lib = _lib.lib()
    t = torch.zeros(8, 128, device=DEV, dtype=torch.bfloat16)
    q, s = ops.quantize_mxfp6(t)
    before = (q.clone(), s.clone())
    for mode in (0, 3):
        assert lib.fino_quantize_mxfp6_rot(t.data_ptr(), q.data_ptr(), s.data_ptr(), 8, 128, 128, ops.BF16, mode, 0) == -1
        assert f"fino_quantize_mxfp6_rot: mode {mode}".encode() in lib.fino_last_error()
    torch.cuda.synchronize()
    assert torch.equal(q, before[0]) and torch.equal(s, before[1])    # nothing was launched
    with pytest.raises(ValueError, match="multiple of 128"):
        ops.quantize_mxfp6(torch.zeros(8, 96, device=DEV, dtype=torch.bfloat16), rotate="act")


# ------------------------------------------------------------------------------------------------------------------ GEMM
def _gemm_case(dtype, epi, keep):
    from frameino_amd import ops
    from tests.test_kernels_gpu import gemm_ref
    m, n, k = RR.GEMM_MNK
    a, w = RR.gemm_operands(dtype)
    g = torch.Generator().manual_seed(5)
    bias = torch.randn(n, generator=g).to(dtype).to(DEV)
    res = torch.randn(m, n, generator=g).to(dtype).to(DEV) if epi >= 2 else None
    gate = torch.randn(2, n, generator=g).to(DEV) if epi >= 3 else None
    sel = (torch.arange(m) % 2).to(torch.int32).to(DEV) if epi >= 3 else None
    ad, wd = a.to(DEV), w.to(DEV)
    aq, sa = ops.quantize_mxfp6(ad, rotate="act")
    wq, sw = ops.quantize_mxfp6(wd, rotate="weight")
    kw = {}
    if keep:
        kw["keep"] = torch.empty(m, n, dtype=dtype, device=DEV)
    out = ops.gemm_mxfp6(aq, sa, wq, sw, bias, epi, res, gate, sel, out_dtype=dtype, **kw)
    a_ref, w_ref = RR.decode(*RR.quantize_ref(a, "act")), RR.decode(*RR.quantize_ref(w, "weight"))
    ref = gemm_ref(a_ref.to(DEV), w_ref.to(DEV), bias, epi, res, gate, sel)
    r = rel_rms(out, ref.float())
    print(f"[{dtype} epi {epi} keep {keep}] rotated mxfp6 GEMM vs fp32 matmul of the decoded restatement: rel-RMS {r:.3e}")
    assert r < 2.0 ** -7                                              # output rounding and fp32 summation order only
    if keep:
        none = ops.gemm_mxfp6(aq, sa, wq, sw, bias, ops.EPI_NONE, out_dtype=dtype)
        assert torch.equal(kw["keep"], none)
        assert torch.equal(out, ops.gemm_mxfp6(aq, sa, wq, sw, bias, epi, res, gate, sel, out_dtype=dtype))
    # against the full-precision product: the rotation's gain on these outlier channels, measured here on both paths
    full = a.double() @ w.double().T
    rot = ops.gemm_mxfp6(aq, sa, wq, sw, out_dtype=dtype)
    plain = ops.gemm_mxfp6(*ops.quantize_mxfp6(ad), *ops.quantize_mxfp6(wd), out_dtype=dtype)
    e_rot, e_plain = RR.rel_err(rot.cpu(), full), RR.rel_err(plain.cpu(), full)
    print(f"[{dtype}] vs the fp64 product: mxfp6 {e_plain:.4f}  rotated {e_rot:.4f}  ratio {e_rot / e_plain:.3f}")
    assert e_rot <= 0.85 * e_plain
    return e_plain, e_rot


@DTYPES
def test_gemm_on_rotated_operands_equals_the_decoded_product_and_gains_on_outlier_channels(dtype):
    from tests.parity import record
    e_plain, e_rot = _gemm_case(dtype, 0, False)
    record(f"mxfp6_rot_gemm[{dtype}]", "rel_rms_ratio", e_rot / e_plain, 0.85)


def test_gemm_on_rotated_operands_through_keep():
    from frameino_amd import ops
    _gemm_case(torch.bfloat16, ops.EPI_RESIDUAL, True)


def test_gemm_on_rotated_operands_with_a_gated_residual_epilogue():
    from frameino_amd import ops
    _gemm_case(torch.float16, ops.EPI_GATED_RESIDUAL, False)


# ---------------------------------------------------------------------------------------------------------------- models
def _model_checks(name, m, run, load_lora):
    from tests.parity import record
    ref = run()
    m.enable_mxfp8_linears()
    out8 = run()
    m.enable_mxfp8_linears(False)
    m.enable_mxfp6_linears()
    n_weights = len(m._fp8)
    out6 = run()
    m.enable_mxfp6_linears(True, rotate=True)                         # another value while on: re-quantised
    assert m.mxfp6_rotate and len(m._fp8) == n_weights > 0
    rot = run()
    assert torch.isfinite(rot.float()).all() and not torch.equal(rot, out6)
    e6r, e6, e8 = rel_rms(rot, ref.float()), rel_rms(out6, ref.float()), rel_rms(out8, ref.float())
    print(f"{name}: vs own bf16 rel-RMS: mxfp6 rotated {e6r:.4f}  mxfp6 {e6:.4f}  mxfp8 {e8:.4f}  rotated / mxfp8 {e6r / e8:.3f}")
    record(f"{name}[mxfp6-rotated-vs-own-bf16]", "rel_rms", e6r, 1.5 * e8)
    record(f"{name}[mxfp8-vs-own-bf16]", "rel_rms", e8, 1.0)
    assert 1e-4 < e6r <= 1.5 * e8
    m.enable_mxfp6_linears(True, rotate=False)
    assert not m.mxfp6_rotate and torch.equal(run(), out6)            # on -> off: the unrotated MXFP6 run, bit for bit
    m.enable_mxfp6_linears(rotate=True)
    assert torch.equal(run(), rot)
    m.to("cpu")
    assert not m._fp8 and m._fp8_pending and m.mxfp6_rotate
    m.to(DEV)
    assert torch.equal(run(), rot) and m._fp8 and m.mxfp6_rotate      # a .to() round trip keeps the rotated output
    load_lora(m)
    merged = run()
    assert m.mxfp6_rotate and not torch.equal(merged, rot)            # the merge reached the rotated weights
    m.unload_lora()
    assert m.mxfp6_rotate and torch.equal(run(), rot)                 # and the unmerge restored them
    m.enable_mxfp6_linears(False)
    assert not m.mxfp6_rotate and not m._fp8 and torch.equal(run(), ref)                  # back to the model dtype


def test_wan_model_with_rotated_mxfp6_linears():
    from tests.test_lora_wan_gpu import diffusers_keys, make_adapter
    from tests.test_mxfp6_gpu import _wan_tiny
    m, _, sd, run = _wan_tiny()

    def load_lora(model):
        ad = {}
        for fam in ("attn1_qkv", "attn2_out", "ffn_up", "ffn_down"):
            ad.update(make_adapter(sd, fam))
        model.load_lora_adapter(diffusers_keys(ad))

    _model_checks("wan_tiny", m, run, load_lora)


def test_cog_model_with_rotated_mxfp6_linears(golden):
    from tests import test_lora_cog_gpu as L
    cfg, sd, a, model = L._setup(golden)
    m = model()

    def load_lora(mm):
        ad = {}
        for fam in ("attn_qkv", "attn_out", "ff"):
            ad.update(L._adapter(sd, cfg, fam, gain=1.0))
        mm.load_lora_adapter(L._keys(ad))

    _model_checks("cog_dit_tiny", m, lambda: L._run(m, a), load_lora)


def test_token_sharded_branch_with_rotation_vs_the_unsharded_rotated_forward():
    import torch.distributed as dist
    from frameino_amd import _lib
    from frameino_amd.configs import WAN22_5B_CFG
    from frameino_amd.parallel import TokenShard
    from frameino_amd.random_init import random_wan_model
    cfg = dict(WAN22_5B_CFG, num_attention_heads=2, num_layers=2, ffn_dim=512, text_dim=128, in_channels=8, out_channels=4)
    m = random_wan_model(cfg, torch.device(DEV), seed=5).enable_mxfp6_linears(rotate=True)
    g = torch.Generator(device=DEV).manual_seed(6)
    x = torch.randn(1, 8, 3, 16, 16, device=DEV, generator=g).bfloat16()
    txt = torch.randn(1, 32, 128, device=DEV, generator=g).bfloat16()
    ts = torch.tensor([500.0], device=DEV)
    fwd = lambda: m(hidden_states=x, timestep=ts, encoder_hidden_states=txt, return_dict=False)[0]      # noqa: E731
    base = fwd()
    own_group = not dist.is_initialized()
    if own_group:
        dist.init_process_group("gloo", store=dist.HashStore(), rank=0, world_size=1)
    try:
        m.parallel = TokenShard(0, 1, None, force=True)
        sharded = fwd()
        assert (0, "kv") in m._fp8 and (0, "q") in m._fp8 and m.mxfp6_rotate
        # the lazily quantised row block is the rotated WEIGHT image of those rows of the fused weight
        w_kv = m._fp8[(0, "kv")]
        assert w_kv[0].numel() == _lib.lib().fino_mxfp6_bytes(2 * m.inner_dim, m.inner_dim)
    finally:
        m.parallel = None
        if own_group:
            dist.destroy_process_group()
    m.enable_mxfp6_linears(True, rotate=False)
    plain = fwd()
    r = rel_rms(sharded, base.float())
    print(f"token-sharded rotated mxfp6 forward vs unsharded rotated mxfp6 forward: rel-RMS {r:.2e}")
    assert r < 2e-3, r
    assert rel_rms(sharded, plain.float()) > 2e-3                     # (and it is the rotated path that was sharded)


def test_wan_denoise_with_rotation_hip_graph_replay_equals_eager():
    """the tiny Wan DiT of tests/test_mxfp6_gpu.py (every MX linear has K % 128 == 0) through the FrameINO denoise loop, 3 Euler
    steps, CFG 5: the rotation adds nothing that is not static on the device, so the graph loop equals the eager loop"""
    from frameino_amd.pipeline_wan_i2v_motion_frameino import WanImageToVideoPipeline
    from frameino_amd.schedulers import FlowMatchEulerDiscreteScheduler
    from tests.test_mxfp6_gpu import _wan_tiny
    m, cfg, _, _ = _wan_tiny()
    pipe = WanImageToVideoPipeline(scheduler=FlowMatchEulerDiscreteScheduler(shift=5.0), transformer=m, expand_timesteps=True)
    c, fg, nid, h, w = cfg["out_channels"], 3, 1, 16, 20
    g = torch.Generator().manual_seed(77)
    rnd = lambda *s: torch.randn(*s, generator=g).to(DEV)          # noqa: E731
    mask = torch.ones(1, 1, fg, h, w)
    mask[:, :, 0] = 0
    args = (rnd(1, c, fg, h, w), rnd(1, c, 1, h, w), rnd(1, c, fg + nid, h, w), rnd(1, c, nid, h, w), mask.to(DEV),
            rnd(1, 77, cfg["text_dim"]).bfloat16(), rnd(1, 77, cfg["text_dim"]).bfloat16(), 5.0, 3)
    pipe.use_hip_graph = False
    m.enable_mxfp6_linears()
    plain = pipe.denoise(*args)
    m.enable_mxfp6_linears(True, rotate=True)
    eager = pipe.denoise(*args)
    pipe.use_hip_graph = True                  # (True makes a failed capture an error)
    graphed = pipe.denoise(*args)
    assert torch.isfinite(eager.float()).all() and torch.equal(eager, graphed)
    assert m.mxfp6_rotate and len(m._fp8) == 6 * 3 and not torch.equal(eager, plain)
