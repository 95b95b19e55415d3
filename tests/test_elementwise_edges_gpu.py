"""The DiT's HBM-bound kernels (csrc/fino_elementwise.hip) through the C ABI, in bf16 and fp16, at the edges where their code
branches: every pass count of `dispatch_np` with partial last passes, row counts around the 4-row workgroup, strided views,
in-place calls, null parameters, fp16 overflow.  Restatements and the bar: tests/kernel_check.py."""
import pytest
import torch

from tests.kernel_check import U32, check_close, check_exact, round64, ulp

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
# rows of up to 4096 channels: a lane sums <= 64 values, then 6 butterfly levels.  The statistics' forward error, in units of
# the fp32 unit roundoff, stated with a margin of ~2x over that count.
LN_K = 160.0


@pytest.fixture(scope="module")
def ops():
    from frameino_amd import ops as o
    return o


def rnd(*shape, dtype, seed, scale=1.0, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + offset).to(dtype).to(DEV)


def f32(v):
    """a Python float as the kernel receives it (a C float)"""
    return torch.tensor(v, dtype=torch.float32).item()


def ln64(x, eps):
    """LayerNorm statistics in fp64 and the forward-error bound of the kernel's fp32 normalised value n = (x - mean) * rstd"""
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    var = (x - mean).pow(2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + f32(eps))
    n = (x - mean) * rstd
    dn = LN_K * U32 * (x.abs().mean(-1, keepdim=True) * rstd + n.abs())
    return n, dn


def ln_ref(mode, x, w, b, shift, scale, eps, dtype):
    """the three modes of ln_modulate_kernel, rounded where its header says; returns (reference, bound)"""
    n, dn = ln64(x, eps)
    w64 = n.new_ones(n.shape[-1]) if w is None else w.double()
    b64 = n.new_zeros(n.shape[-1]) if b is None else b.double()
    if mode == 0:     # T(LN(x) * (1 + scale) + shift): fp32 math, one rounding; 1 + scale is itself an fp32 op
        s = (1.0 + scale).double()
        o = n * s + shift.double()
        return round64(o, dtype), dn * s.abs() + 3 * U32 * ((n * s).abs() + shift.double().abs())
    t = n * w64 + b64
    dt = dn * w64.abs() + 3 * U32 * ((n * w64).abs() + b64.abs())
    if mode == 1:     # T(LN(x) * w + b)
        return round64(t, dtype), dt
    # mode 2: T(T(T(LN(x) * w + b) * T(1 + scale)) + shift), scale / shift T-representable as the reference's T tensors
    tt = round64(t, dtype)
    s = (1.0 + scale).to(dtype).double()
    p = round64(tt * s, dtype)
    o = round64(p + shift.double(), dtype)
    # where the kernel's first rounding lands one ulp away (its fp32 statistic straddles a rounding point), that ulp times the
    # scale propagates through the two later roundings
    bound = (ulp(tt, dtype) + dt) * s.abs() + 2 * ulp(p, dtype) + 2 * ulp(o, dtype)
    return o, bound


DIMS = [8, 48, 504, 520, 1032, 3072, 4088, 4096]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", DIMS)
def test_layernorm_family_at_every_pass_count(ops, dtype, dim):
    rows = 1001
    x = rnd(rows, dim, dtype=dtype, seed=dim, offset=0.3)
    w = rnd(dim, dtype=torch.float32, seed=dim + 1, scale=0.2, offset=1.0)
    b = rnd(dim, dtype=torch.float32, seed=dim + 2, scale=0.5)
    tab = rnd(3, 2, dim, dtype=torch.float32, seed=dim + 3, scale=0.5).to(dtype).float()      # T-representable
    sel = (torch.arange(rows, device=DEV) % 3).to(torch.int32)
    shift, scale = tab[:, 0], tab[:, 1]
    # mode 0, with and without the selector (no selector: row 0 of the table)
    check_close(ops.adaln_modulate(x, shift, scale, sel, eps=1e-6), *ln_ref(0, x, None, None, shift[sel.long()],
                                                                              scale[sel.long()], 1e-6, dtype))
    check_close(ops.adaln_modulate(x, shift, scale, None, eps=1e-6), *ln_ref(0, x, None, None, shift[0], scale[0], 1e-6,
                                                                               dtype))
    # mode 1, each of w / b null or set
    for ww, bb in ((w, b), (w, None), (None, b), (None, None)):
        check_close(ops.layernorm(x, ww, bb, eps=1e-5), *ln_ref(1, x, ww, bb, None, None, 1e-5, dtype))
    # mode 2 (T-representable affine parameters, as the reference's T tensors)
    wt, bt = w.to(dtype).float(), b.to(dtype).float()
    check_close(ops.layernorm_zero(x, wt, bt, shift, scale, sel, 1e-5),
                *ln_ref(2, x, wt, bt, shift[sel.long()], scale[sel.long()], 1e-5, dtype))
    check_close(ops.layernorm_zero(x, None, None, shift, scale, None, 1e-5),
                *ln_ref(2, x, None, None, shift[0], scale[0], 1e-5, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [0, 1, 3, 4, 5, 1001])
def test_layernorm_family_row_counts_and_strided_views(ops, dtype, rows):
    dim, pad = 1032, 24
    big = rnd(rows, dim + pad, dtype=dtype, seed=rows + 7, scale=2.0, offset=-0.5)
    x = big[:, :dim]
    tab = rnd(2, 2, dim, dtype=torch.float32, seed=rows + 8, scale=0.5).to(dtype).float()
    sel = ((torch.arange(rows, device=DEV) * 7) % 2).to(torch.int32)
    w = rnd(dim, dtype=dtype, seed=rows + 9, scale=0.1, offset=1.0).float()
    for mode in (0, 1, 2):
        dst = torch.full((rows, dim + 2 * pad), 5.0, dtype=dtype, device=DEV)
        y = dst[:, pad:pad + dim]
        if mode == 0:
            ops.adaln_modulate(x, tab[:, 0], tab[:, 1], sel, eps=1e-6, out=y)
            ref = ln_ref(0, x, None, None, tab[:, 0][sel.long()], tab[:, 1][sel.long()], 1e-6, dtype)
        elif mode == 1:
            ops.layernorm(x, w, None, eps=1e-6, out=y)
            ref = ln_ref(1, x, w, None, None, None, 1e-6, dtype)
        else:
            ops.layernorm_zero(x, w, w - 1.0, tab[:, 0], tab[:, 1], sel, 1e-6, out=y)
            ref = ln_ref(2, x, w, w - 1.0, tab[:, 0][sel.long()], tab[:, 1][sel.long()], 1e-6, dtype)
        if rows:
            check_close(y, *ref)
        assert torch.all(dst[:, :pad] == 5.0) and torch.all(dst[:, pad + dim:] == 5.0), "written outside the view"


def test_layernorm_fp16_shift_overflows_to_inf(ops):
    dim, rows = 520, 9
    x = rnd(rows, dim, dtype=torch.float16, seed=11)
    shift = torch.zeros(dim, device=DEV)
    shift[::3] = 70000.0
    shift[1::3] = -70000.0
    scale = torch.zeros(dim, device=DEV)
    y = ops.adaln_modulate(x, shift, scale, None, eps=1e-6)
    ref, bound = ln_ref(0, x, None, None, shift, scale, 1e-6, torch.float16)
    assert torch.isinf(ref[:, ::3]).all() and torch.isinf(ref[:, 1::3]).all()
    check_close(y, ref, bound)
    tab = torch.zeros(2, dim, device=DEV)
    tab[0, 5] = 65504.0                       # T-representable shifts at the ends of the fp16 range: finite exactly where the
    tab[0, 6] = -65504.0                      # reference is
    y = ops.layernorm_zero(x, None, None, tab[0], tab[1], None, 1e-6)
    check_close(y, *ln_ref(2, x, None, None, tab[0], tab[1], 1e-6, torch.float16))


def test_layernorm_argument_errors(ops):
    from frameino_amd import _lib
    x = torch.zeros(4, 4104, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match=r"\(-3\)"):          # FINO_ERR_UNSUPPORTED: dim > 8 passes of 512
        ops.layernorm(x, None, None)
    assert _lib.lib().fino_layernorm(x.data_ptr(), x.data_ptr(), 4, 4100, 4104, 4104, None, None, 1e-6, ops.BF16, None) == -1
    with pytest.raises(RuntimeError, match=r"\(-1\)"):          # FINO_ERR_ARG: dim % 8 != 0
        ops.layernorm(torch.zeros(4, 44, dtype=torch.float16, device=DEV), None, None)
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        ops.adaln_modulate(torch.zeros(4, 44, dtype=torch.float16, device=DEV), torch.zeros(44, device=DEV),
                           torch.zeros(44, device=DEV))


# ---------------------------------------------------------------------------------------------------------- gated residual
@pytest.mark.parametrize("dtype", DTYPES)
def test_gated_residual_plain_gated_staged_strided_in_place(ops, dtype):
    """no reduction: bit-identical to the fp32 restatement (T(x + y*g), T(x + T(y*g)), T(x + y))"""
    rows, dim = 301, 1032
    bx = rnd(rows, dim + 16, dtype=dtype, seed=20)
    by = rnd(rows, dim + 8, dtype=dtype, seed=21, scale=3.0)
    x, y = bx[:, 8:8 + dim], by[:, :dim]
    tab = rnd(3, 2, dim, dtype=torch.float32, seed=22)
    sel = ((torch.arange(rows, device=DEV) * 5) % 3).to(torch.int32)
    g = tab[:, 1][sel.long()]
    xf, yf = x.float(), y.float()
    want = {"plain": (xf + yf).to(dtype), "gated": (xf + yf * g).to(dtype),
            "staged": (xf + (yf * g).to(dtype).float()).to(dtype), "gated0": (xf + yf * tab[0, 1]).to(dtype)}
    check_exact(ops.gated_residual(x, y), want["plain"])
    check_exact(ops.gated_residual(x, y, tab[:, 1], sel), want["gated"])
    check_exact(ops.gated_residual(x, y, tab[:, 1], sel, staged=True), want["staged"])
    check_exact(ops.gated_residual(x, y, tab[0, 1]), want["gated0"])
    for kind in ("plain", "gated", "staged"):
        b2 = bx.clone()
        xv = b2[:, 8:8 + dim]
        gate = None if kind == "plain" else tab[:, 1]
        ops.gated_residual(xv, y, gate, None if kind == "plain" else sel, out=xv, staged=kind == "staged")
        check_exact(xv, want[kind])
        check_exact(b2[:, :8], bx[:, :8])
        check_exact(b2[:, 8 + dim:], bx[:, 8 + dim:])
    if dtype == torch.float16:                                   # saturation: T(60000 + 60000) = inf
        big = torch.full((4, 8), 60000.0, dtype=dtype, device=DEV)
        big[1] = -60000.0
        check_exact(ops.gated_residual(big, big), (big.float() * 2).to(dtype))


# ---------------------------------------------------------------------------------------------------------- RMSNorm + RoPE
def rope_pairs(o, cos, sin, head_dim):
    """RoPE on adjacent channel pairs as rmsnorm_rope_row computes it in fp32 (x1 c - x2 s, x1 s + x2 c)"""
    rows, dim = o.shape
    v = o.view(rows, dim // head_dim, head_dim // 2, 2)
    x1, x2 = v[..., 0], v[..., 1]
    c, s = cos[:, None], sin[:, None]
    return torch.stack((x1 * c - x2 * s, x1 * s + x2 * c), -1).reshape(rows, dim)


def rms_restate(x, rrms, w, cos, sin, head_dim, out_scale, dtype):
    """rmsnorm_rope_row in fp32 given the kernel's own statistic: T(T(x * rrms) * w) [-> RoPE] -> x out_scale -> T"""
    o = x.float()
    if w is not None:
        o = ((o * rrms[:, None]).to(dtype).float() * w.float()).to(dtype).float()
    if cos is not None:
        o = rope_pairs(o, cos, sin, head_dim)
    return (o * f32(out_scale)).to(dtype)


def rrms64(x, eps):
    return 1.0 / torch.sqrt(x.double().pow(2).mean(-1) + f32(eps))


def tables(rows, head_dim, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    ang = torch.rand(rows, head_dim // 2, device=DEV, generator=g) * 6.28
    return ang.cos().contiguous(), ang.sin().contiguous()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("head_dim", [64, 128])
@pytest.mark.parametrize("dim", [128, 640, 1152, 3072, 4096])
def test_rmsnorm_rope_and_row_rrms(ops, dtype, head_dim, dim):
    """row_rrms within a stated fp32 bound of the fp64 statistic; rmsnorm_rope_ bit-identical to its fp32 restatement on that
    statistic (so both use the same bits); no weight = RoPE alone; out_scale != 1 is one rounding"""
    rows, pad = 203, 16
    big = rnd(rows, dim + pad, dtype=dtype, seed=dim + head_dim, scale=1.5)
    x = big[:, pad:]
    w = rnd(dim, dtype=dtype, seed=dim + 1, scale=0.1, offset=1.0)
    cos, sin = tables(rows, head_dim, dim)
    rr = ops.row_rrms(x, 1e-6)
    want = rrms64(x, 1e-6)
    check_close(rr, want, bound=LN_K * U32 * want)
    c = head_dim ** -0.5 * ops.LOG2E
    for ww, cs, sc in ((w, True, 1.0), (w, True, c), (w, False, 1.0), (None, True, 1.0), (None, True, c)):
        b2 = big.clone()
        ops.rmsnorm_rope_(b2[:, pad:], ww, 1e-6, cos if cs else None, sin if cs else None, head_dim if cs else 0,
                          out_scale=sc)
        check_exact(b2[:, pad:], rms_restate(x, rr, ww, cos if cs else None, sin if cs else None, head_dim, sc, dtype))
        check_exact(b2[:, :pad], big[:, :pad])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("head_dim", [64, 128])
def test_qkv_rmsnorm_rope_segments_in_place_and_scattered(ops, dtype, head_dim):
    """one launch over q | k (in place) or q | k | v (scattered by head): each segment with its own weight, eps, out_scale and
    RoPE flag, against the single-segment restatement"""
    rows, heads = 77, 5
    dim = heads * head_dim
    qkv = rnd(rows, 3 * dim, dtype=dtype, seed=head_dim, scale=2.0)
    wq = rnd(dim, dtype=dtype, seed=31, scale=0.1, offset=1.0)
    wk = rnd(dim, dtype=dtype, seed=32, scale=0.1, offset=1.0)
    cos, sin = tables(rows, head_dim, 33)
    c = head_dim ** -0.5 * ops.LOG2E
    q, k, v = qkv[:, :dim], qkv[:, dim:2 * dim], qkv[:, 2 * dim:]
    want_q = rms_restate(q, ops.row_rrms(q, 1e-6), wq, cos, sin, head_dim, c, dtype)
    want_k = rms_restate(k, ops.row_rrms(k, 1e-5), wk, cos, sin, head_dim, 1.0, dtype)
    # scattered: [3, heads, rows, head_dim + 8], every head with a padded row stride
    ld = head_dim + 8
    out = torch.full((3, heads, rows, ld), 9.0, dtype=dtype, device=DEV)
    head_off = (torch.arange(3 * heads, device=DEV, dtype=torch.int64) * rows * ld).contiguous()
    head_ld = torch.full((heads,), ld, dtype=torch.int64, device=DEV)
    before = qkv.clone()
    ops.qkv_rmsnorm_rope_(qkv, dim, wq, 1e-6, wk, 1e-5, cos, sin, head_dim, q_out_scale=c, out=out, head_off=head_off,
                          head_ld=head_ld)
    check_exact(qkv, before)
    for s, want in enumerate((want_q, want_k, v)):
        check_exact(out[s, :, :, :head_dim], want.reshape(rows, heads, head_dim).transpose(0, 1))
    assert torch.all(out[..., head_dim:] == 9.0)
    # in place: q and k only, v untouched
    ops.qkv_rmsnorm_rope_(qkv, dim, wq, 1e-6, wk, 1e-5, cos, sin, head_dim, q_out_scale=c)
    check_exact(qkv[:, :dim], want_q)
    check_exact(qkv[:, dim:2 * dim], want_k)
    check_exact(qkv[:, 2 * dim:], before[:, 2 * dim:])
    # rmsnorm_rope_scatter, one segment, no RoPE, out_scale != 1
    out2 = torch.full((1, heads, rows, ld), 9.0, dtype=dtype, device=DEV)
    ops.rmsnorm_rope_scatter(before[:, dim:2 * dim], wk, 1e-5, None, None, head_dim, out2, head_off[:heads], head_ld,
                             out_scale=0.75)
    want = rms_restate(before[:, dim:2 * dim], ops.row_rrms(before[:, dim:2 * dim], 1e-5), wk, None, None, head_dim, 0.75,
                       dtype)
    check_exact(out2[0, :, :, :head_dim], want.reshape(rows, heads, head_dim).transpose(0, 1))


# ---------------------------------------------------------------------------------------------------------- per-head LN + RoPE
def headnorm_ref(x, w, b, eps, cos, sin, row0, out_scale, dtype):
    """headnorm_rope_kernel on x [B, rows, heads, head_dim]: T(LN_head(x) * w + b) (fp64, one rounding), RoPE of that on rows
    >= row0 as the kernel computes it in fp32 (xr c - xi s, xi c + xr s on interleaved pairs), x out_scale, one rounding.
    Returns (reference, bound): where the kernel's normalised value is one ulp away (or cancels), that difference propagated"""
    bsz, rows, heads, hd = x.shape
    if w is not None:
        n, dn = ln64(x, eps)
        t = round64(n * w.double() + b.double(), dtype)
        dt = ulp(t, dtype) + dn * w.double().abs() + 3 * U32 * ((n * w.double()).abs() + b.double().abs())
    else:
        t, dt = x, torch.zeros(x.shape, dtype=torch.float64, device=x.device)
    o, do = t.float(), dt
    if cos is not None:
        tr = o[:, row0:].reshape(bsz, rows - row0, heads, hd // 2, 2)
        c = cos.view(1, rows - row0, 1, hd // 2, 2)
        s = sin.view(1, rows - row0, 1, hd // 2, 2)
        xr, xi = tr[..., 0], tr[..., 1]
        rr = torch.stack((xr * c[..., 0] + (-xi) * s[..., 0], xi * c[..., 1] + xr * s[..., 1]), -1)
        o = torch.cat((o[:, :row0], rr.reshape(bsz, rows - row0, heads, hd)), 1)
        dp = dt[:, row0:].reshape(tr.shape)
        cd, sd = c.double().abs(), s.double().abs()
        drr = torch.stack((dp[..., 0] * cd[..., 0] + dp[..., 1] * sd[..., 0], dp[..., 1] * cd[..., 1] + dp[..., 0] * sd[..., 1]), -1)
        do = torch.cat((dt[:, :row0], drr.reshape(bsz, rows - row0, heads, hd)), 1)
    want = (o * f32(out_scale)).to(dtype)
    return want, do * out_scale + 2 * ulp(want, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("head_dim", [16, 32, 64, 128])
def test_headnorm_rope(ops, dtype, head_dim):
    """LayerNorm per head (fp32 statistics over head_dim / 8 lanes), rounded to T, then RoPE on rows >= rope_row0 and out_scale,
    rounded once: 1 ulp against headnorm_ref, or its bound.  Without w / b there is no normalisation and the result is
    bit-identical.  batch > 1 with a padded batch stride and row stride: nothing outside the view is written."""
    bsz, rows, heads, lt = 3, 45, 3, 6
    d = heads * head_dim
    big = rnd(bsz, rows + 3, d + 8, dtype=dtype, seed=head_dim, scale=1.5, offset=0.2)
    w = rnd(head_dim, dtype=dtype, seed=41, scale=0.2, offset=1.0)
    bi = rnd(head_dim, dtype=dtype, seed=42, scale=0.3)
    g = torch.Generator(device=DEV).manual_seed(43)
    for row0, norm, rope, sc in ((lt, True, True, 1.0), (0, True, True, head_dim ** -0.5 * 1.4426950408889634),
                                 (lt, True, False, 1.0), (lt, False, True, 0.5), (0, False, True, 1.0)):
        ang = torch.rand(rows - row0, head_dim, device=DEV, generator=g) * 6.28
        cos, sin = (ang.cos().contiguous(), ang.sin().contiguous()) if rope else (None, None)
        b2 = big.clone()
        x = b2[:, :rows, :d]
        x0 = x.clone().view(bsz, rows, heads, head_dim)
        ops.headnorm_rope_(x, heads, head_dim, w if norm else None, bi if norm else None, 1e-6, cos, sin, rope_row0=row0,
                           out_scale=sc)
        want, bound = headnorm_ref(x0, w if norm else None, bi, 1e-6, cos, sin, row0, sc, dtype)
        got = x.view(bsz, rows, heads, head_dim)
        if norm:
            check_close(got, want, bound)
        else:
            check_exact(got, want)
        check_exact(b2[:, rows:], big[:, rows:])
        check_exact(b2[:, :rows, d:], big[:, :rows, d:])


# ---------------------------------------------------------------------------------------------------------- patchify / inputs
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("patch", [(1, 2, 2), (2, 2, 2), (1, 1, 1)])
def test_patchify_unpatchify_with_padded_leading_dimensions(ops, dtype, patch):
    c, f, h, w, cout = 6, 4, 8, 12, 5
    pt, ph, pw = patch
    x = rnd(c, f, h, w, dtype=dtype, seed=50)
    L, n = (f // pt) * (h // ph) * (w // pw), c * pt * ph * pw
    ref = x.view(c, f // pt, pt, h // ph, ph, w // pw, pw).permute(1, 3, 5, 0, 2, 4, 6).reshape(L, n)
    big = torch.full((L, n + 24), 3.0, dtype=dtype, device=DEV)
    ops.patchify(x, patch, out=big[:, :n])
    check_exact(big[:, :n], ref)
    assert torch.all(big[:, n:] == 3.0)
    m = pt * ph * pw * cout
    ybig = rnd(L, m + 16, dtype=dtype, seed=51)
    y = ybig[:, :m]
    out = ops.unpatchify(y, cout, f, h, w, patch)
    want = y.reshape(f // pt, h // ph, w // pw, pt, ph, pw, cout).permute(6, 0, 3, 1, 4, 2, 5).reshape(cout, f, h, w)
    check_exact(out, want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nid", [0, 2])
def test_wan_model_input(ops, dtype, nid):
    c, fg, h, w = 4, 3, 5, 6
    lat = rnd(c, fg, h, w, dtype=torch.float32, seed=60, scale=3.0)
    cond = rnd(c, 1, h, w, dtype=torch.float32, seed=61, scale=3.0)
    idl = rnd(c, nid, h, w, dtype=torch.float32, seed=62) if nid else None
    traj = rnd(c, fg + nid, h, w, dtype=torch.float32, seed=63)
    if dtype == torch.float16:
        traj[0, 0, 0, :2] = torch.tensor([1e5, -1e5])              # saturates to +-inf as the reference's cast does
    x = ops.wan_model_input(lat, cond, idl, traj, dtype)
    blend = torch.cat((cond, lat[:, 1:]), 1)
    parts = [blend] + ([idl] if nid else [])
    want = torch.cat((torch.cat(parts, 1), traj), 0).to(dtype)
    check_exact(x, want)


# ---------------------------------------------------------------------------------------------------------- sampler steps
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("has_uncond", [True, False])
def test_cfg_euler_step(ops, dtype, has_uncond):
    c, fg, ft, h, w = 4, 3, 4, 5, 6
    lat = rnd(c, fg, h, w, dtype=torch.float32, seed=70)
    pc, pu = rnd(c, ft, h, w, dtype=dtype, seed=71), rnd(c, ft, h, w, dtype=dtype, seed=72)
    dt = torch.tensor([-0.037], device=DEV)
    g = 5.0
    n = pc[:, :fg]
    if has_uncond:       # every op in T (the pipeline's noise_pred arithmetic)
        u = pu[:, :fg].float()
        n = (u + (g * (n.float() - u).to(dtype).float()).to(dtype).float()).to(dtype)
    for round_out in (True, False):
        l2 = lat.clone()
        ops.cfg_euler_step_(l2, pc, pu if has_uncond else None, g, dt, round_out=round_out)
        want = lat + dt * n.float()
        check_exact(l2, want.to(dtype).float() if round_out else want)


def _cfg_v(pred, fg, g, has_uncond):
    p = pred.float()[:, :fg]
    return p[0] + g * (p[1] - p[0]) if has_uncond else p[0]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("has_uncond", [True, False])
def test_cfg_vpred_step(ops, dtype, has_uncond):
    """v = u + g (c - u) in fp32;  x0 = T(sa x) - sb v;  x' = T(T(ca x) + cb x0)"""
    f, ft, c, h, w = 3, 4, 2, 5, 6
    lat = rnd(f, c, h, w, dtype=dtype, seed=80, scale=2.0)
    pred = rnd(2 if has_uncond else 1, ft, c, h, w, dtype=dtype, seed=81)
    coef = torch.tensor([0.83, 0.55, 0.91, 0.12, 6.0], device=DEV)
    l2 = lat.clone()
    ops.cfg_vpred_step_(l2, pred, coef, has_uncond)
    v = _cfg_v(pred, f, coef[4], has_uncond)
    x = lat.float()
    x0 = (coef[0] * x).to(dtype).float() - coef[1] * v
    check_exact(l2, ((coef[2] * x).to(dtype).float() + coef[3] * x0).to(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("has_uncond", [True, False])
@pytest.mark.parametrize("use_old", [0.0, 1.0])
def test_cfg_dpm_step(ops, dtype, has_uncond, use_old):
    """v as above;  x0 = T(sa x) - sb v;  d = use_old ? m3 x0 - m4 x0_old : x0;  x' = T(T(m1 x) - m2 d + T(mn noise));
    x0_old <- x0"""
    f, ft, c, h, w = 3, 4, 2, 5, 6
    lat = rnd(f, c, h, w, dtype=dtype, seed=90, scale=2.0)
    pred = rnd(2 if has_uncond else 1, ft, c, h, w, dtype=dtype, seed=91)
    noise = rnd(f, c, h, w, dtype=dtype, seed=92)
    x0_old = rnd(f, c, h, w, dtype=torch.float32, seed=93)
    coef = torch.tensor([0.83, 0.55, 0.97, 0.31, 1.7, 0.6, 0.05, 4.5, use_old], device=DEV)
    l2, o2 = lat.clone(), x0_old.clone()
    ops.cfg_dpm_step_(l2, pred, o2, noise, coef, has_uncond)
    v = _cfg_v(pred, f, coef[7], has_uncond)
    x = lat.float()
    x0 = (coef[0] * x).to(dtype).float() - coef[1] * v
    d = coef[4] * x0 - coef[5] * x0_old if use_old else x0
    nz = (coef[6] * noise.float()).to(dtype).float()
    check_exact(l2, ((coef[2] * x).to(dtype).float() - coef[3] * d + nz).to(dtype))
    check_exact(o2, x0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("has_uncond", [True, False])
def test_cfg_unipc_step_bit_identical(ops, dtype, has_uncond):
    """v = T(u + T(g T(c - u)));  m_t = x - T(sigma v) (torch's device product: fp16 rounds the exact product once);  x_c = use_corr ? Cx last + C0 m0 + C1 m1 + Ct m_t : x;
    x' = Px x_c + P0 m_t + P1 m0 -- fp32, left to right"""
    c, fg, ft, h, w = 4, 3, 4, 5, 6
    pc, pu = rnd(c, ft, h, w, dtype=dtype, seed=100), rnd(c, ft, h, w, dtype=dtype, seed=101)
    x, last, m0, m1 = (rnd(c, fg, h, w, dtype=torch.float32, seed=102 + i) for i in range(4))
    for use_corr in (0.0, 1.0):
        k = torch.tensor([5.0, 0.83, use_corr, 0.9, 0.31, -0.07, 0.12, 0.8, 0.25, -0.05], device=DEV)
        v = pc[:, :fg].float()
        if has_uncond:
            u = pu[:, :fg].float()
            v = (u + (k[0] * (v - u).to(dtype).float()).to(dtype).float()).to(dtype).float()
        mt = x - (v.to(dtype) * k[1].item()).float()        # T tensor x fp32 scalar on the device, as the sampler
        xc = k[3] * last + k[4] * m0 + k[5] * m1 + k[6] * mt if use_corr else x
        xn = k[7] * xc + k[8] * mt + k[9] * m0
        bx, bl, b0, b1 = (t.clone() for t in (x, last, m0, m1))
        ops.cfg_unipc_step_(bx, bl, b0, b1, pc, pu if has_uncond else None, k)
        check_exact(bx, xn)
        check_exact(bl, xc)
        check_exact(b0, mt)
        check_exact(b1, m0)
