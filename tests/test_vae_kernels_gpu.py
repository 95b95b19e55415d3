"""The VAE glue kernels (csrc/fino_vae.hip, csrc/fino_vae_cog.hip) through the C ABI in bf16, fp16 and (where the entry takes
it) fp32, at the edges where their code branches: the lanes-per-row branches of rmsnorm_silu_cl, padded channels, partial
rows of a workgroup, the 16-byte and the scalar-gather paths of dup_up3d_add, odd and even frame counts.  Restatements and the
bar: tests/kernel_check.py; the rearrangements are restated from the reference's own view / permute / interpolate semantics,
not from the kernels' index arithmetic."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.kernel_check import U32, check_close, check_exact, round64, ulp

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT16 = [torch.bfloat16, torch.float16]
DT3 = [torch.bfloat16, torch.float16, torch.float32]
# forward error of a row / group statistic summed in fp32 (<= 1024 channels: <= 16 terms per lane, then 6 butterfly levels;
# GroupNorm: per-channel partials over the rows of a workgroup, combined in fp64), in units of the fp32 unit roundoff
STAT_K = 64.0


@pytest.fixture(scope="module")
def ops():
    from frameino_amd import ops as o
    return o


def rnd(*shape, dtype, seed, scale=1.0, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + offset).to(dtype).to(DEV)


def silu64(t):
    return t / (1.0 + torch.exp(-t))


# ---------------------------------------------------------------------------------------------------------- WanRMS_norm + SiLU
def wan_rms64(x, gamma, c_valid):
    """x / max(||x||_2, 1e-12) * sqrt(C) * gamma over the row, fp64"""
    x = x.double()
    nrm = x.pow(2).sum(-1, keepdim=True).sqrt().clamp_min(1e-12)
    return x / nrm * math.sqrt(c_valid) * gamma.double()


def cl_input(rows, c_valid, c_pad, dtype, seed):
    x = torch.zeros(rows, c_pad, dtype=dtype, device=DEV)
    x[:, :c_valid] = rnd(rows, c_valid, dtype=dtype, seed=seed, scale=2.0, offset=0.1)
    gamma = torch.zeros(c_pad, device=DEV)
    gamma[:c_valid] = rnd(c_valid, dtype=torch.float32, seed=seed + 1, scale=0.3, offset=1.0)
    return x, gamma


@pytest.mark.parametrize("dtype", DT16)
@pytest.mark.parametrize("c_pad,c_valid", [(64, 64), (64, 40), (128, 96), (256, 256), (192, 160), (320, 320), (384, 360),
                                           (512, 512), (1024, 1000), (16, 12)])
def test_rmsnorm_silu_cl_every_lane_group(ops, dtype, c_pad, c_valid):
    """c_pad / 8 lanes per row when that is a power of two <= 64 (8, 16, 32, 64 lanes: 8, 4, 2, 1 rows per wave), one row per
    wave otherwise (192, 320, 384 channels); rows not a multiple of a workgroup's rows; pad channels stay exactly 0.  One
    rounding of the fp32 result: 1 ulp against fp64 (__expf's error is far below it)."""
    rows = 4 * (64 // min(64, max(1, c_pad // 8))) * 3 + 5
    x, gamma = cl_input(rows, c_valid, c_pad, dtype, seed=c_pad + c_valid)
    for silu in (True, False):
        y = ops.rmsnorm_silu_cl(x, gamma, c_valid, silu=silu)
        t = wan_rms64(x, gamma, c_valid)
        want = round64(silu64(t) if silu else t, dtype)
        check_close(y[:, :c_valid], want[:, :c_valid])
        assert not y[:, c_valid:].any(), "pad channels must stay exactly zero"


@pytest.mark.parametrize("c_pad,c_valid", [(64, 48), (256, 256), (384, 360), (1024, 1000)])
def test_rmsnorm_silu_cl_f32_and_its_split_planes(ops, c_pad, c_valid):
    """fp32 output within (STAT_K + STAT_K |t|) fp32 eps of the fp64 value (the |t| term: the exponent's argument error in
    SiLU); the split planes written in the same pass are exactly split_bf16's planes of that fp32 output (hi = bf16(x),
    mid = bf16(x - hi), lo = bf16(x - hi - mid)) and sum back to it"""
    from frameino_amd import _lib
    rows = 37
    x, gamma = cl_input(rows, c_valid, c_pad, torch.float32, seed=c_pad)
    for silu in (True, False):
        y = ops.rmsnorm_silu_cl_f32(x, gamma, c_valid, silu=silu)
        t = wan_rms64(x, gamma, c_valid)
        want = silu64(t) if silu else t
        bound = STAT_K * U32 * (1.0 + t.abs()) * want.abs() + 1e-37
        check_close(y, want, bound)
        hi = y.bfloat16()
        r1 = y - hi.float()
        mid = r1.bfloat16()
        lo = (r1 - mid.float()).bfloat16()
        planes = (hi, mid, lo)
        for split, nplanes, idx in (("planes", 3, (0, 1, 2)), ("planes", 2, (0, 1)), ("W", 2, (0, 1, 0)), ("A", 2, (0, 0, 1))):
            sp = ops.rmsnorm_silu_cl_f32(x, gamma, c_valid, silu=silu, split=split, nplanes=nplanes)
            for s, q in enumerate(idx):
                check_exact(sp[:, s * c_pad:(s + 1) * c_pad], planes[q])
        one = torch.empty(rows, c_pad, dtype=torch.bfloat16, device=DEV)           # nseg 1: one plane alone (plane 2)
        _lib.check(_lib.lib().fino_rmsnorm_silu_cl_f32(x.data_ptr(), one.data_ptr(), rows, c_valid, c_pad, gamma.data_ptr(),
                                                       int(silu), 1, 2, ops._stream()), "fino_rmsnorm_silu_cl_f32")
        check_exact(one, lo)
        back = hi.double() + mid.double() + lo.double()
        assert torch.equal(back, y.double()), "the three planes must sum back to the fp32 value"


# ---------------------------------------------------------------------------------------------------------- softmax rows
@pytest.mark.parametrize("dtype", DT3)
@pytest.mark.parametrize("n,scale", [(1, 1.0), (37, 0.125), (64, 1.0), (200, 0.3), (515, 0.05), (96, 40.0)])
def test_softmax_rows(ops, dtype, n, scale):
    """in place, ld > n: columns past n untouched.  The exponent's argument (x - max) * scale is restated in fp32 as the
    kernel forms it; 16-bit rows take __expf = exp2 of the fp32 product with log2(e) (restated too); fp32 rows expf and a
    division.  Bound: the fp32 sum's order and the exp / division roundings (16-bit rows: plus |a| fp32 eps for __expf)."""
    rows, ld = 13, n + 24
    s = rnd(rows, ld, dtype=dtype, seed=n, scale=3.0)
    s[3, :n] = s[3, 0].item()                                        # a row of equal values
    s0 = s.clone()
    ops.softmax_rows_(s, n, scale)
    x = s0[:, :n].float()
    a = (x - x.max(-1, keepdim=True).values) * torch.tensor(scale, dtype=torch.float32)
    if dtype == torch.float32:
        e = torch.exp(a.double())
    else:
        e = torch.exp2((a * torch.tensor(1.4426950408889634, dtype=torch.float32)).double())
    p = e / e.sum(-1, keepdim=True)
    bound = (n / 64.0 + 16.0 + (0.0 if dtype == torch.float32 else a.double().abs())) * U32 * p
    bound = bound + (1e-40 if dtype == torch.float32 else 2.0 ** -126)      # __expf returns 0 below the fp32 normal range
    check_close(s[:, :n], p if dtype == torch.float32 else round64(p, dtype), bound,
                tiny=0.0 if dtype == torch.float32 else 2.0 ** -126)
    check_exact(s[:, n:], s0[:, n:])


# ---------------------------------------------------------------------------------------------------------- DupUp3D / AvgDown3D
def cl_tensor(t, h, w, c, c_pad, dtype, seed, scale=1.0):
    x = torch.zeros(t, h, w, c_pad, dtype=dtype, device=DEV)
    x[..., :c] = rnd(t, h, w, c, dtype=dtype, seed=seed, scale=scale)
    return x


def dup_up3d_ref(x, c_in, c_out, ft, fs):
    """DupUp3D (first chunk): repeat_interleave over channels, view (C_out, ft, fs, fs, T, H, W), interleave into time and
    space, drop the first ft - 1 frames.  channels-last in and out"""
    t, h, w, _ = x.shape
    factor = ft * fs * fs
    xc = x[..., :c_in].permute(3, 0, 1, 2)                           # [C_in, T, H, W]
    xc = xc.repeat_interleave(c_out * factor // c_in, dim=0)
    xc = xc.reshape(c_out, ft, fs, fs, t, h, w).permute(0, 4, 1, 5, 2, 6, 3).reshape(c_out, t * ft, h * fs, w * fs)
    return xc[:, ft - 1:].permute(1, 2, 3, 0)


@pytest.mark.parametrize("dtype", DT3)
@pytest.mark.parametrize("t_in,c_in,c_in_pad,c_out,c_out_pad,ft,fs", [
    (3, 64, 64, 64, 72, 2, 2),        # equal widths: the 16-byte path, plus main's pad channels
    (1, 64, 64, 64, 64, 2, 2),        # one input frame
    (2, 36, 40, 36, 40, 1, 2),        # c_out % 8 != 0: the last partial chunk gathers scalars
    (3, 96, 96, 48, 56, 2, 2),        # unequal widths: rep = c_out * 8 / c_in
    (2, 32, 32, 64, 64, 2, 1),        # time only
])
def test_dup_up3d_add(ops, dtype, t_in, c_in, c_in_pad, c_out, c_out_pad, ft, fs):
    """no reduction: out = T(main + dup(x)), bit-identical; main's pad channels pass through unchanged"""
    h, w = 3, 5
    x = cl_tensor(t_in, h, w, c_in, c_in_pad, dtype, seed=t_in + c_in)
    main = rnd(1 + (t_in - 1) * ft, h * fs, w * fs, c_out_pad, dtype=dtype, seed=c_out)
    out = ops.dup_up3d_add(main, x, c_in, c_out, ft, fs)
    want = main.clone()
    want[..., :c_out] = (main[..., :c_out].float() + dup_up3d_ref(x, c_in, c_out, ft, fs).float()).to(dtype)
    check_exact(out, want)


def avg_down3d_ref(x, c_in, c_out, ft, fs):
    """AvgDown3D: zero frames in front up to a multiple of ft, view (C_in, T/ft, ft, H/fs, fs, W/fs, fs), the (ft, fs, fs)
    taps behind each channel, groups of `group` rearranged channels averaged -- summed in the kernel's order (g ascending,
    fp32), divided by group.  channels-last in, fp32 [T', H', W', C_out] out"""
    t, h, w, _ = x.shape
    pad_t = (ft - t % ft) % ft
    xc = x[..., :c_in].permute(3, 0, 1, 2).float()
    xc = torch.cat((torch.zeros(c_in, pad_t, h, w, device=DEV), xc), 1)
    tt = (t + pad_t) // ft
    xc = xc.reshape(c_in, tt, ft, h // fs, fs, w // fs, fs).permute(0, 2, 4, 6, 1, 3, 5)
    group = c_in * ft * fs * fs // c_out
    xc = xc.reshape(c_out, group, tt, h // fs, w // fs)
    s = xc[:, 0].clone()
    for g in range(1, group):
        s = s + xc[:, g]
    return (s / float(group)).permute(1, 2, 3, 0)


@pytest.mark.parametrize("dtype", DT3)
@pytest.mark.parametrize("t_in,c_in,c_in_pad,c_out,c_out_pad,ft,fs", [
    (4, 16, 16, 64, 64, 2, 2),        # even T, group 1
    (5, 16, 16, 64, 72, 2, 2),        # odd T: one zero frame in front; main's pad channels
    (3, 64, 64, 64, 64, 1, 2),        # ft 1: group 4
    (4, 40, 48, 40, 48, 2, 1),        # fs 1: group 2
    (6, 32, 32, 32, 32, 2, 2),        # group 8
])
def test_avg_down3d_add(ops, dtype, t_in, c_in, c_in_pad, c_out, c_out_pad, ft, fs):
    """the group's sum restated in the kernel's order, so the result is bit-identical: out = T(main + T_32(sum / group))"""
    h, w = 4, 6
    x = cl_tensor(t_in, h, w, c_in, c_in_pad, dtype, seed=t_in * 7 + c_in)
    tt = (t_in + (ft - t_in % ft) % ft) // ft
    main = rnd(tt, h // fs, w // fs, c_out_pad, dtype=dtype, seed=c_out + 1)
    out = ops.avg_down3d_add(main, x, c_in, c_out, ft, fs)
    want = main.clone()
    want[..., :c_out] = (main[..., :c_out].float() + avg_down3d_ref(x, c_in, c_out, ft, fs)).to(dtype)
    check_exact(out, want)


# ---------------------------------------------------------------------------------------------------------- VAE patchify
@pytest.mark.parametrize("dtype", DT3)
@pytest.mark.parametrize("patch,c_pad", [(1, 8), (2, 16), (2, 64)])
def test_vae_patchify_and_unpatchify_clamp(ops, dtype, patch, c_pad):
    """(c, r, q) channel order of `b c f (h q) (w r) -> b (c r q) f h w`; pad channels exactly 0; the decoder's tail clamps to
    [-1, 1] after the rearrangement (inputs well beyond +-1)"""
    c, t, h, w = 3, 3, 4, 5
    x = rnd(c, t, h * patch, w * patch, dtype=torch.float32, seed=patch, scale=2.0)
    y = ops.vae_patchify(x, c_pad, patch, dtype)
    want = torch.zeros(t, h, w, c_pad, dtype=dtype, device=DEV)
    want[..., :c * patch * patch] = x.view(c, t, h, patch, w, patch).permute(1, 2, 4, 0, 5, 3).reshape(t, h, w, -1).to(dtype)
    check_exact(y, want)
    yy = rnd(t, h, w, c_pad, dtype=dtype, seed=patch + 10, scale=2.0)
    out = ops.vae_unpatchify_clamp(yy, c, patch)
    ref = yy[..., :c * patch * patch].reshape(t, h, w, c, patch, patch).permute(3, 0, 1, 5, 2, 4)
    check_exact(out, ref.reshape(c, t, h * patch, w * patch).float().clamp(-1.0, 1.0))
    assert (yy.float().abs() > 1).any()


# ---------------------------------------------------------------------------------------------------------- CogVideoX VAE glue
@pytest.mark.parametrize("dtype", DT16)
@pytest.mark.parametrize("t_in", [2, 3, 4, 5])
def test_avg_pool_time2(ops, dtype, t_in):
    """frame pairs averaged, T((a + b) / 2); the first frame of an odd count kept as is -- bit-identical"""
    x = rnd(t_in, 3, 5, 24, dtype=dtype, seed=t_in, scale=4.0)
    if dtype == torch.float16:
        x[-2:, 0, 0, :2] = 60000.0                                   # a + b overflows fp16, not the kernel's fp32 sum
    y = ops.avg_pool_time2(x)
    xf = x.float()
    if t_in % 2:
        want = torch.cat((x[:1], ((xf[1::2] + xf[2::2]) * 0.5).to(dtype)), 0)
    else:
        want = ((xf[0::2] + xf[1::2]) * 0.5).to(dtype)
    check_exact(y, want)


def _nearest(z, size):
    return F.interpolate(z, size=size, mode="nearest")


@pytest.mark.parametrize("dtype", DT16)
@pytest.mark.parametrize("t,tz", [(1, 1), (4, 2), (5, 3), (3, 2)])
@pytest.mark.parametrize("silu", [False, True])
def test_groupnorm_cl_with_spatial_modulation(ops, dtype, t, tz, silu):
    """GroupNorm(32) -> T, then CogVideoXSpatialNorm3D's T(T(. * Y[z]) + B[z]) with z nearest-interpolated the reference's way
    (the first frame of an odd count on its own), then T(silu).  The normalised value within 1 ulp of fp64 or the statistic's
    fp32 bound where a x + b cancels; a one-ulp step there propagated through the later roundings."""
    h, w, c, c_pad, groups = 6, 10, 96, 128, 32
    hz, wz = 3, 5
    x = cl_tensor(t, h, w, c, c_pad, dtype, seed=t * 10 + tz, scale=1.5)
    x[..., :c] += torch.linspace(-1, 1, c, device=DEV).to(dtype)
    gamma = torch.zeros(c_pad, device=DEV)
    beta = torch.zeros(c_pad, device=DEV)
    gamma[:c] = rnd(c, dtype=torch.float32, seed=3, scale=0.2, offset=1.0)
    beta[:c] = rnd(c, dtype=torch.float32, seed=4, scale=0.5)
    my = cl_tensor(tz, hz, wz, c, c_pad, dtype, seed=5, scale=0.5)
    mb = cl_tensor(tz, hz, wz, c, c_pad, dtype, seed=6, scale=0.5)
    y = ops.groupnorm_cl(x, c, groups, gamma, beta, 1e-6, mod=(my, mb), silu=silu)
    # fp64 GroupNorm over (C/G channels x T x H x W)
    xc = x[..., :c].double().reshape(t * h * w, groups, c // groups)
    mean = xc.mean((0, 2), keepdim=True)
    var = (xc - mean).pow(2).mean((0, 2), keepdim=True)
    rstd = 1.0 / torch.sqrt(var + torch.tensor(1e-6, dtype=torch.float32).item())
    n = ((xc - mean) * rstd).reshape(t, h, w, c)
    dn = (STAT_K * U32 * (xc.abs().mean((0, 2), keepdim=True) * rstd + ((xc - mean) * rstd).abs())).reshape(t, h, w, c)
    g64, b64 = gamma[:c].double(), beta[:c].double()
    o = round64(n * g64 + b64, dtype)
    a_c = rstd.reshape(1, groups, 1).expand(1, groups, c // groups).reshape(c) * g64        # a x + b: fp32 cancellation
    d = ulp(o, dtype) + dn * g64.abs() + 4 * U32 * ((x[..., :c].double() * a_c).abs() + (mean.reshape(groups, 1).expand(
        groups, c // groups).reshape(c) * a_c).abs() + b64.abs())
    # z nearest-interpolated to (t, h, w) the reference's way
    zy, zb = (m[..., :c].permute(3, 0, 1, 2)[None] for m in (my, mb))
    if t > 1 and t % 2:
        zy, zb = (torch.cat((_nearest(z[:, :, :1], (1, h, w)), _nearest(z[:, :, 1:], (t - 1, h, w))), 2) for z in (zy, zb))
    else:
        zy, zb = (_nearest(z, (t, h, w)) for z in (zy, zb))
    zy, zb = (z[0].permute(1, 2, 3, 0).double() for z in (zy, zb))
    p = round64(o.double() * zy, dtype)
    d = d * zy.abs() + 2 * ulp(p, dtype)
    q = round64(p.double() + zb, dtype)
    d = d + 2 * ulp(q, dtype)
    if silu:
        q = round64(silu64(q.double()), dtype)
        d = 1.1 * d + 2 * ulp(q, dtype)
    check_close(y[..., :c], q, d)
    assert not y[..., c:].any()


@pytest.mark.parametrize("dtype", DT16)
@pytest.mark.parametrize("axis,extent,ha,wa,hb,wb", [(0, 3, 5, 6, 4, 6), (1, 4, 5, 6, 5, 7), (0, 9, 5, 6, 4, 6), (1, 2, 3, 2, 3, 5)])
def test_vae_blend_tiles(ops, dtype, axis, extent, ha, wa, hb, wb):
    """diffusers' blend_v / blend_h in T: b[y] = a[-e + y] * (1 - y / e) + b[y] * (y / e), each product rounded to T, then the
    sum; the extent clamped to both tiles.  No reduction: bit-identical"""
    t, c_pad = 3, 16
    a = rnd(t, ha, wa, c_pad, dtype=dtype, seed=axis * 10 + extent, scale=2.0)
    b = rnd(t, hb, wb, c_pad, dtype=dtype, seed=axis * 10 + extent + 1, scale=2.0)
    want = b.clone()
    e = min(extent, ha if axis == 0 else wa, hb if axis == 0 else wb)
    for y in range(e):
        if axis == 0:
            want[:, y] = a[:, ha - e + y] * (1 - y / e) + want[:, y] * (y / e)
        else:
            want[:, :, y] = a[:, :, wa - e + y] * (1 - y / e) + want[:, :, y] * (y / e)
    ops.vae_blend_tiles_(a, b, extent, axis)
    check_exact(b, want)
