"""fino_lora_merge (ops.lora_merge_) against (W.float() + sum_a s_a * B_a.float() @ A_a.float()).to(dtype): at most 1 ulp of
the output dtype anywhere and >= 99.9 % of the elements bit-identical (the only freedom is the order of the fp32 sums)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from frameino_amd import ops as o
    return o


def rnd(*shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


def reference(w, adapters):
    if w.dtype == torch.float32:                 # fp32 targets: the exact sum, rounded once
        acc = w.double()
        for a, b, s in adapters:
            acc = acc + s * (b.double() @ a.double())
        return acc.float()
    acc = w.float()
    for a, b, s in adapters:
        acc = acc + s * (b.double() @ a.double()).float()
    return acc.to(w.dtype)


def _ordered(t):
    """the bit pattern as a monotone integer (neighbouring floats differ by 1; +0 and -0 both map to 0)"""
    i = t.contiguous().view(torch.int16).long()
    mag = i & 0x7FFF
    return torch.where(i < 0, -mag, mag)


def _fp32_bound(w, adapters):
    """the forward-error bound of the kernel's fp32 sums (rank products, then W + delta) against the exact sum"""
    mag = w.double().abs()
    for a, b, s in adapters:
        mag = mag + abs(s) * (b.double().abs() @ a.double().abs())
    rmax = max([a.shape[0] for a, _, _ in adapters] + [1])
    return (rmax + 2) * 2.0 ** -24 * mag


def check(out, ref, w, adapters):
    """<= 1 ulp of the output dtype, except where the rank terms cancel so far that the fp32 sums' own order matters more
    (there: within the fp32 forward-error bound); >= 99.9 % of the elements bit-identical (16-bit outputs)"""
    err = (out.double() - ref.double()).abs()
    within = err <= _fp32_bound(w, adapters)
    if out.dtype == torch.float32:                 # fp32 targets: an fp32 result has no coarser rounding to hide in
        assert bool(within.all()), float(err.max())
        return
    d = (_ordered(out) - _ordered(ref)).abs()
    assert bool(((d <= 1) | within).all()), f"max {int(d[~within].max())} ulp outside the fp32 bound"
    same = (out.contiguous().view(torch.int16) == ref.contiguous().view(torch.int16)).float().mean().item()
    assert same >= 0.999, f"only {same:.5f} of the elements bit-identical"


def make(n, k, ranks, dtype, seed=0, scales=None):
    w = rnd(n, k, dtype=dtype, seed=seed, scale=0.05)
    ads = []
    for i, r in enumerate(ranks):
        a = rnd(r, k, dtype=dtype, seed=seed + 10 + i, scale=r ** -0.5)
        b = rnd(n, r, dtype=dtype, seed=seed + 20 + i, scale=0.02)
        ads.append((a, b, (scales or [0.75] * len(ranks))[i]))
    return w, ads


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("shape", [(13, 7), (1000, 3072), (3 * 3072, 3072), (14336, 3072), (3072, 14336)])
def test_shapes(ops, dtype, shape):
    w, ads = make(*shape, [64], dtype, seed=1)
    ref = reference(w, ads)
    out = ops.lora_merge_(w.clone(), ads)
    check(out, ref, w, ads)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("rank", [1, 3, 16, 64, 128])
def test_ranks(ops, dtype, rank):
    w, ads = make(1000, 3072, [rank], dtype, seed=2)
    check(ops.lora_merge_(w.clone(), ads), reference(w, ads), w, ads)
    w, ads = make(77, 150, [rank], dtype, seed=3)              # ragged in both dimensions
    check(ops.lora_merge_(w.clone(), ads), reference(w, ads), w, ads)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_two_adapters_out_of_place_and_leading_dimension(ops, dtype):
    w, ads = make(333, 520, [5, 48], dtype, seed=4, scales=[1.5, -0.4])
    ref = reference(w, ads)
    out = torch.full_like(w, 7.0)
    w0 = w.clone()
    ops.lora_merge_(w, ads, out=out)
    assert torch.equal(w, w0)                                  # out of place: the base is untouched
    check(out, ref, w, ads)
    check(ops.lora_merge_(w.clone(), ads), ref, w, ads)                # in place
    # leading dimensions larger than K (weight, output and factors), odd ones included (scalar edge path)
    for pad in (8, 3):
        big = torch.zeros(333, 520 + pad, dtype=dtype, device=DEV)
        big[:, :520] = w
        a_big = torch.zeros(5, 520 + pad, dtype=dtype, device=DEV)
        a_big[:, :520] = ads[0][0]
        b_big = torch.zeros(333, 5 + pad, dtype=dtype, device=DEV)
        b_big[:, :5] = ads[0][1]
        ads_v = [(a_big[:, :520], b_big[:, :5], ads[0][2]), ads[1]]
        dst = torch.full((333, 520 + 2 * pad), 3.0, dtype=dtype, device=DEV)
        ops.lora_merge_(big[:, :520], ads_v, out=dst[:, :520])
        check(dst[:, :520], ref, w, ads)
        assert torch.all(dst[:, 520:] == 3.0)                  # nothing written past K
        ops.lora_merge_(big[:, :520], ads_v)
        check(big[:, :520], ref, w, ads)
        assert torch.all(big[:, 520:] == 0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_zero_scale_is_the_identity(ops, dtype):
    w, ads = make(1000, 3072, [64], dtype, seed=5, scales=[0.0])
    assert torch.equal(ops.lora_merge_(w.clone(), ads), w)
    assert torch.equal(ops.lora_merge_(w.clone(), []), w)


def test_fp16_overflow_goes_to_inf(ops):
    w = torch.full((40, 96), 60000.0, dtype=torch.float16, device=DEV)
    w[1::2] = -60000.0
    a = torch.ones(16, 96, dtype=torch.float16, device=DEV)
    b = torch.full((40, 16), 400.0, dtype=torch.float16, device=DEV)
    b[1::2] = -400.0
    out = ops.lora_merge_(w.clone(), [(a, b, 1.0)])
    ref = reference(w, [(a, b, 1.0)])
    assert torch.isinf(ref).all()
    assert torch.equal(out, ref)


def test_argument_errors(ops):
    w, ads = make(64, 64, [4], torch.bfloat16, seed=6)
    with pytest.raises(ValueError):
        ops.lora_merge_(w, [(ads[0][0].half(), ads[0][1].half(), 1.0)])
    with pytest.raises(ValueError):
        ops.lora_merge_(w, [(ads[0][1], ads[0][0], 1.0)])
