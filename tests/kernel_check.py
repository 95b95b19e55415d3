"""Element-level checks of the HBM-bound kernels (normalisations, RoPE, residuals, sampler steps, VAE glue) against a plain
torch restatement of the same operation.

The restatement computes in fp64 and rounds to the storage dtype at exactly the points the kernel's header comment names
(`round64`: one correct rounding, no double rounding through fp32).  Where a kernel is pure fp32 arithmetic without a
reduction, the restatement repeats that fp32 arithmetic op for op instead (the elementwise kernels are built with
-ffp-contract=off, and eager torch runs each tensor op as its own fp32 rounding), and the result must be bit-identical:
`check_exact`.  Where a kernel reduces a row in fp32, its statistic differs from the fp64 one by the fp32 summation error
alone: `check_close`."""
import torch

U32 = 2.0 ** -24                                   # fp32 unit roundoff
MANT = {torch.bfloat16: 8, torch.float16: 11, torch.float32: 24}   # significant bits
INT_VIEW = {2: torch.int16, 4: torch.int32}


def round64(t, dtype):
    """an fp64 tensor correctly rounded (nearest, ties to even) to `dtype`.  torch converts fp64 -> bf16 / fp16 through fp32,
    which can round twice; rounding to fp32 toward zero with a sticky last bit (round to odd) first makes the second rounding
    exact."""
    t = t.double()
    if dtype == torch.float64:
        return t
    f = t.float()
    if dtype == torch.float32:
        return f
    over = f.double().abs() > t.abs()
    f = torch.where(over, torch.nextafter(f, torch.zeros_like(f)), f)
    sticky = (f.double() != t) & torch.isfinite(f)
    bits = f.view(torch.int32)
    f = torch.where(sticky, bits | 1, bits).view(torch.float32)
    return f.to(dtype)


def ulp(x, dtype):
    """the spacing of `dtype` at |x| (fp64; subnormal spacing below the normal range)"""
    x = x.double().abs()
    p = MANT[dtype]
    emin = {torch.bfloat16: -126, torch.float16: -14, torch.float32: -126}[dtype]
    e = torch.floor(torch.log2(torch.where(x > 0, x, torch.ones_like(x))))
    e = torch.clamp(e, min=emin)
    return torch.pow(2.0, e - (p - 1))


def ordered(t):
    """the bit pattern as a monotone integer (neighbouring floats differ by 1; +0 and -0 both map to 0)"""
    i = t.contiguous().view(INT_VIEW[t.element_size()]).long()
    mag = i & ((1 << (8 * t.element_size() - 1)) - 1)
    return torch.where(i < 0, -mag, mag)


def _where(mask, what):
    idx = mask.nonzero()
    return f"{int(mask.sum())} {what}, first at {tuple(idx[0].tolist())}" if len(idx) else ""


def check_nonfinite(out, ref):
    """where the reference is +-inf or nan the kernel gives the same value, and it gives no other non-finite value"""
    o, r = out.double(), ref.double()
    bad = torch.isnan(o) != torch.isnan(r)
    inf = (torch.isinf(o) | torch.isinf(r)) & ~torch.isnan(r)
    bad |= inf & (o != r)
    assert not bad.any(), _where(bad, "elements whose non-finite value differs from the reference")


def check_exact(out, ref):
    """bit-identical (nan in the same elements)"""
    assert out.dtype == ref.dtype and out.shape == ref.shape, (out.dtype, ref.dtype, out.shape, ref.shape)
    o, r = out.contiguous(), ref.contiguous()
    diff = (o != r) & ~(torch.isnan(o) & torch.isnan(r))
    if diff.any():
        i = tuple(diff.nonzero()[0].tolist())
        raise AssertionError(f"{_where(diff, 'elements differ')}: got {o[i].item()!r}, want {r[i].item()!r}")


def check_close(out, ref, bound=None, min_same=0.999, tiny=0.0):
    """A kernel whose only freedom is the order of its fp32 sums.

    16-bit outputs (`ref` rounded to the same dtype): every element within 1 ulp of the reference, or within `bound` (fp64,
    absolute; the stated forward-error bound of the kernel's fp32 arithmetic where the output cancels, or the propagated
    bound where an intermediate rounding may flip); at least `min_same` of the elements bit-identical (of fewer than 1000
    elements, all but one; elements whose reference is below `tiny` -- e.g. the fp32 normal range a fast exp flushes -- are
    not counted); non-finite values where and only where the reference has them.
    fp32 outputs (`ref` an fp64 tensor): every element within `bound` of the fp64 value (required)."""
    assert out.shape == ref.shape, (out.shape, ref.shape)
    if out.dtype == torch.float32:
        assert bound is not None, "an fp32 output needs its stated bound"
        check_nonfinite(out, ref)
        fin = torch.isfinite(ref)
        err = (out.double() - ref.double()).abs()
        bad = fin & ~(err <= bound)
        assert not bad.any(), (f"{_where(bad, 'elements outside the fp32 bound')}; worst err/bound "
                               f"{float((err[fin] / bound.expand_as(err)[fin].clamp_min(1e-300)).max()):.3g}")
        return
    assert out.dtype == ref.dtype, (out.dtype, ref.dtype)
    check_nonfinite(out, ref)
    fin = torch.isfinite(ref.double())
    d = (ordered(out) - ordered(ref)).abs()
    ok = d <= 1
    if bound is not None:
        ok |= (out.double() - ref.double()).abs() <= bound
    bad = fin & ~ok
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{_where(bad, 'elements more than 1 ulp off and outside the bound')}: got {out[i].item()!r}, "
                             f"want {ref[i].item()!r}; max {int(d[bad].max())} ulp")
    counted = ref.double().abs() >= tiny
    differ = (out.contiguous().view(INT_VIEW[2]) != ref.contiguous().view(INT_VIEW[2])) & counted
    n, nd = int(counted.sum()), int(differ.sum())
    assert nd <= max(1.0, (1.0 - min_same) * n), f"only {1 - nd / max(n, 1):.5f} of the elements bit-identical (need {min_same})"
