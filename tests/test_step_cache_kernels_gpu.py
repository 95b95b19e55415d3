"""fino_step_cache_probe / fino_step_cache_residual (ops.step_cache_probe / step_cache_residual) against the torch formula of
first-block caching: r bit-exact, the per-segment means within 1 ulp of torch's mean (fp32: within the fp32 summation bound
of the fp64 sum), the decisions equal wherever the diff is more than 2 ulp from the threshold, bit-identical reruns."""
import math

import pytest
import torch

from frameino_amd import ops
from frameino_amd.step_cache import decide
from tests.kernel_check import U32, check_exact, check_nonfinite, ordered

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16, torch.float32]


def _rows(rows, d, dtype, g, pad=0, scale=1.0):
    """a [rows, d] tensor; pad > 0: a row-strided view into a wider buffer"""
    t = (torch.randn(rows, d + pad, generator=g, device=DEV) * scale).to(dtype)
    return t[:, :d] if pad else t


def _check_sums(sums, h0, h1, p, dtype):
    """sums == (sum |T(r - p)|, sum |p|): 16-bit -- T(S / N) within 1 ulp of torch's mean; fp32 -- S within the fp32
    summation bound of the fp64 sum"""
    r = h1 - h0
    dl = r - p if p is not None else r
    n = r.numel()
    for got, t in ((sums[0], dl.abs()), (sums[1], p.abs() if p is not None else torch.zeros_like(r))):
        if dtype == torch.float32:
            exact = t.double().sum().item()
            per_thread = (-(-r.shape[0] // 1024)) * r.shape[1]        # longest sequential run of one thread, plus the trees
            assert abs(got - exact) <= (per_thread + 24) * U32 * exact + 1e-30, (got, exact)
        else:
            mine = (torch.tensor(got, dtype=torch.float32) / n).to(dtype)
            want = t.mean().cpu()
            assert abs(int(ordered(mine.view(1))[0]) - int(ordered(want.view(1))[0])) <= 1, (mine.item(), want.item())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,d,pad,nseg", [(1, 8, 0, 1), (37, 64, 0, 2), (1000, 264, 8, 1), (1500, 512, 16, 2),
                                            (3, 3072, 0, 2)])
def test_probe_matches_torch(dtype, rows, d, pad, nseg):
    g = torch.Generator(device=DEV).manual_seed(rows + d + nseg)
    segs = []
    for s in range(nseg):
        rs = rows + 13 * s                                   # ragged: the segments differ in length
        h0, h1 = _rows(rs, d, dtype, g, pad), _rows(rs, d, dtype, g, pad)
        p = _rows(rs, d, dtype, g, pad, scale=1.5)
        segs.append((h0, h1, p, torch.empty(rs, d + pad, dtype=dtype, device=DEV)[:, :d],
                     torch.empty(rs, d, dtype=dtype, device=DEV)))
    sums = ops.step_cache_probe(*[[sg[i] for sg in segs] for i in range(5)]).cpu()
    for s, (h0, h1, p, r, c) in enumerate(segs):
        check_exact(r, h1 - h0)
        check_exact(c, h1)
        _check_sums(sums[s].tolist(), h0, h1, p, dtype)
        # the decision: equal to torch's wherever the diff is more than 2 ulp from the threshold
        want = float((r - p).abs().mean() / p.abs().mean())
        diff, _ = decide(*sums[s].tolist(), r.numel(), dtype, 0.0)
        ulp = 2.0 ** (math.frexp(want)[1] - {torch.bfloat16: 8, torch.float16: 11, torch.float32: 24}[dtype])
        for thr in (want * 0.5, want - 3 * ulp, want + 3 * ulp, want * 2):
            assert (diff > thr) == (want > thr), (diff, want, thr)
    again = ops.step_cache_probe(*[[sg[i] for sg in segs] for i in range(5)]).cpu()
    assert torch.equal(again, sums)                                 # reproducible bit for bit


@pytest.mark.parametrize("dtype", DTYPES)
def test_probe_without_and_with_zero_previous_residual(dtype):
    g = torch.Generator(device=DEV).manual_seed(5)
    h0, h1 = _rows(300, 128, dtype, g), _rows(300, 128, dtype, g)
    r = torch.empty_like(h0)
    s_null = ops.step_cache_probe(h0, h1, None, r).cpu()[0].tolist()        # p NULL: read as zeros, no h1 copy
    check_exact(r, h1 - h0)
    zero = torch.zeros_like(h0)
    s_zero = ops.step_cache_probe(h0, h1, zero, torch.empty_like(h0)).cpu()[0].tolist()
    assert s_null == s_zero and s_zero[1] == 0.0 and s_zero[0] > 0
    _check_sums(s_zero, h0, h1, zero, dtype)
    diff, compute = decide(*s_zero, h0.numel(), dtype, 0.1)                  # x / 0 = inf: compute
    assert diff == math.inf and compute
    same = ops.step_cache_probe(h0, h0, zero, torch.empty_like(h0)).cpu()[0].tolist()   # r = 0, p = 0: 0 / 0 = nan: skip
    diff, compute = decide(*same, h0.numel(), dtype, 0.1)
    assert math.isnan(diff) and not compute


@pytest.mark.parametrize("dtype", DTYPES)
def test_probe_propagates_non_finite_values(dtype):
    g = torch.Generator(device=DEV).manual_seed(6)
    h0, h1, p = _rows(64, 64, dtype, g), _rows(64, 64, dtype, g), _rows(64, 64, dtype, g)
    h0[3, 5], h1[3, 5] = math.inf, math.inf                 # inf - inf = nan
    h1[7, 9] = -math.inf
    r = torch.empty_like(h0)
    s = ops.step_cache_probe(h0, h1, p, r).cpu()[0].tolist()
    check_nonfinite(r, h1 - h0)
    check_exact(r, h1 - h0)
    assert math.isnan(s[0]) and math.isfinite(s[1])
    f0, f1 = _rows(64, 64, dtype, g), _rows(64, 64, dtype, g)
    p[10, 0] = -math.inf
    s2 = ops.step_cache_probe(f0, f1, p, torch.empty_like(r)).cpu()[0].tolist()
    assert s2[0] == math.inf and s2[1] == math.inf          # |r - (-inf)| = |-inf| = inf in both sums


def test_probe_full_size_branches_bf16():
    """two CFG branches of Wan2.2-5B at 49 frames 704x1280 (L = 12320 with the ID frame, D = 3072)"""
    g = torch.Generator(device=DEV).manual_seed(7)
    L, d = 12320, 3072
    h0, h1 = _rows(2 * L, d, torch.bfloat16, g), _rows(2 * L, d, torch.bfloat16, g)
    p = _rows(2 * L, d, torch.bfloat16, g)
    r, c = torch.empty_like(h0), torch.empty_like(h0)
    segs = [(0, L), (L, 2 * L)]
    args = [[t[a:b] for a, b in segs] for t in (h0, h1, p, r, c)]
    sums = ops.step_cache_probe(*args).cpu()
    check_exact(r, h1 - h0)
    check_exact(c, h1)
    for s, (a, b) in enumerate(segs):
        _check_sums(sums[s].tolist(), h0[a:b], h1[a:b], p[a:b], torch.bfloat16)
    assert torch.equal(ops.step_cache_probe(*args).cpu(), sums)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,d,pad", [(1, 8, 0), (777, 200, 8), (4096, 3072, 0)])
def test_residual_add_and_subtract_are_torch_bit_for_bit(dtype, rows, d, pad):
    g = torch.Generator(device=DEV).manual_seed(rows)
    a, b = _rows(rows, d, dtype, g, pad, scale=100.0), _rows(rows, d, dtype, g, pad)
    check_exact(ops.step_cache_residual(a, b, subtract=True), a - b)
    check_exact(ops.step_cache_residual(a, b, subtract=False), a + b)
    want = a + b
    ops.step_cache_residual(a, b, out=b, subtract=False)          # in place, as the skipped step writes x
    check_exact(b, want)
    if dtype == torch.float16:
        big = torch.full((4, 8), 60000.0, dtype=dtype, device=DEV)
        check_exact(ops.step_cache_residual(big, big, subtract=False), big + big)      # overflow to inf as torch
