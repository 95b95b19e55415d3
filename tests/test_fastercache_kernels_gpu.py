"""FasterCache's two kernels (ops.fastercache_delta / ops.fastercache_apply) against tests/fastercache_ref.py.

The low-pass bound: max |DL - DL64| of the kernel is at most 32 x the same error of the CPU's fp32 torch.fft restatement on
the same input, both against the fp64 restatement.  32: a direct fp32 sum over H W terms loses about sqrt(HW) / log2(HW)
(5 - 7 at these sizes) more than a butterfly, doubled for the two transforms; a misplaced or missing bin moves the result by
about sigma / sqrt(HW) >= 1.7e-2 sigma, four orders above the bound."""
import pytest
import torch

from frameino_amd import ops
from tests import fastercache_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
SHAPES = [(3, 4, 6), (2, 5, 7), (5, 10, 10), (2, 16, 9), (2, 9, 16), (720, 44, 80), (1, 128, 128)]
MARGIN = 32
_REF = {}


def _case(shape, dtype):
    """inputs and the two CPU restatements of one case, computed once"""
    key = (shape, dtype)
    if key not in _REF:
        g = torch.Generator().manual_seed(sum(shape) + (1 if dtype == torch.float16 else 0))
        u, c = torch.randn(shape, generator=g).to(dtype), torch.randn(shape, generator=g).to(dtype)
        d, dl64 = R.delta_ref(u, c, torch.float64)
        err32 = float((R.lowpass(d, torch.float32).double() - dl64).abs().max())
        _REF[key] = (u, c, d, dl64, err32)
    return _REF[key]


def _bound(err32):
    return MARGIN * err32


def test_bin_counts():
    assert [R.bin_count(h, w) for h, w in ((44, 80), (4, 6), (5, 7), (10, 10))] == [197, 1, 5, 13]


def test_supported():
    assert ops.fastercache_supported(720, 44, 80) and ops.fastercache_supported(1, 128, 128) and ops.fastercache_supported(1, 1, 16384)
    assert not ops.fastercache_supported(1, 128, 129) and not ops.fastercache_supported(0, 4, 4)
    assert not ops.fastercache_supported(1, 0, 4) and not ops.fastercache_supported(1, 4, 0)
    with pytest.raises(ValueError, match="not supported"):
        ops.fastercache_delta(torch.zeros(1, 128, 129, dtype=torch.bfloat16, device=DEV),
                              torch.zeros(1, 128, 129, dtype=torch.bfloat16, device=DEV))


@DTYPES
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_delta(shape, dtype):
    u, c, d, dl64, err32 = _case(shape, dtype)
    ud, cd = u.to(DEV), c.to(DEV)
    dl, dh = ops.fastercache_delta(ud, cd)
    assert dl.dtype == dh.dtype == torch.float32 and dl.shape == dh.shape == ud.shape
    # DH is the kernel's own D - DL, bit for bit (D is never assumed: it is the restatement's fp32 subtraction)
    assert torch.equal(dh, (ud.float() - cd.float()) - dl)
    err = float((dl.cpu().double() - dl64).abs().max())
    print(f"{shape} {dtype}: kernel max|DL - DL64| = {err:.3e}, torch.fft fp32 = {err32:.3e}, ratio {err / max(err32, 1e-300):.2f}")
    assert err <= _bound(err32)
    dl2, dh2 = ops.fastercache_delta(ud, cd)                       # the same bits on a second run
    assert torch.equal(dl2, dl) and torch.equal(dh2, dh)
    if shape[1:] == (4, 6):                                        # r = 0: DL is the plane mean
        mean = d.double().mean(dim=(-2, -1), keepdim=True).expand_as(d)
        assert float((dl64 - mean).abs().max()) <= 1e-12          # (the restatement: what the bound above compares with)


@DTYPES
def test_equal_inputs_give_exact_zeros(dtype):
    for shape in ((2, 5, 7), (3, 10, 10), (2, 44, 80)):
        u = torch.randn(shape, generator=torch.Generator().manual_seed(3)).to(dtype).to(DEV)
        dl, dh = ops.fastercache_delta(u, u.clone())
        assert bool((dl == 0).all()) and bool((dh == 0).all())


def _cosine(h, w, fy, fx):
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    return torch.cos(2 * torch.pi * (fy * yy / h + fx * xx / w))


@DTYPES
@pytest.mark.parametrize("h,w,inside,outside", [(10, 10, (2, 0), (2, 1)), (10, 10, (-1, 1), (0, 3)), (5, 7, (1, 0), (1, 1))],
                         ids=["10x10_r2_a", "10x10_r2_b", "5x7_r1"])
def test_mask_probes(h, w, inside, outside, dtype):
    """a unit cosine on the disk's edge comes back whole in DL, one just outside as zero in DL and whole in DH: `<=` against
    `<`, and the centre convention on even and odd axes"""
    spread = 2.0 ** -8                                             # rounding the cosine to T leaks at most this into other bins
    for (fy, fx), kept in ((inside, True), (outside, False)):
        u = _cosine(h, w, fy, fx).to(dtype)[None]                  # (the rounded cosine is the input: D = float(u) exactly)
        c = torch.zeros_like(u)
        d, dl64 = R.delta_ref(u, c, torch.float64)
        err32 = float((R.lowpass(d, torch.float32).double() - dl64).abs().max())
        # the probe itself, on the restatement alone: whole in DL or absent from it, far beyond the bound below
        if kept:
            assert float((dl64 - d).abs().max()) <= spread and float(dl64.abs().max()) >= 0.9
        else:
            assert float(dl64.abs().max()) <= spread
        ud, cd = u.to(DEV), c.to(DEV)
        dl, dh = ops.fastercache_delta(ud, cd)
        err = float((dl.cpu().double() - dl64).abs().max())
        print(f"{h}x{w} ({fy}, {fx}) {dtype}: kernel {err:.3e}, torch.fft fp32 {err32:.3e}")
        assert err <= _bound(err32)
        assert torch.equal(dh, (ud.float() - cd.float()) - dl)     # ... and DH holds the rest, whole or zero with it


@DTYPES
@pytest.mark.parametrize("n", [1, 7, 8, 4097, 720 * 44 * 80])
def test_apply(n, dtype):
    g = torch.Generator().manual_seed(n % 1000)
    c = torch.randn(n, generator=g).to(dtype).to(DEV)
    dl, dh = torch.randn(n, generator=g).to(DEV), torch.randn(n, generator=g).to(DEV)
    for al, ah in ((1.0, 1.0), (1.1, 1.21), (0.0, 0.0)):
        out = ops.fastercache_apply(c, dl, dh, al, ah)
        assert out.dtype == dtype and torch.equal(out, R.apply_ref(c, dl, dh, R.f32(al), R.f32(ah))), (al, ah)
        if al == 0.0:
            assert torch.equal(out, c)
    same = c.clone()
    ops.fastercache_apply(same, dl, dh, 1.1, 1.21, out=same)        # in place
    assert torch.equal(same, R.apply_ref(c, dl, dh, R.f32(1.1), R.f32(1.21)))
