"""fino_magcache_calibrate (ops.magcache_calibrate) against the fp64 restatement of MagCache's calibration quantity
(tests/magcache_ref.py): r_new bit-equal to ops.step_cache_residual, the two means to relative 1e-5, bit-identical reruns,
untouched rows and columns beyond the operands, r_new aliasing r_prev or not.

The tolerance.  A row's three fp32 sums run over the row's squares / products: a lane adds its ceil(vpr / 64) vectors of E
elements in sequence, then six butterfly levels, so a sum of positive terms carries at most n_seq = ceil(vpr / 64) * E + 6
roundings, (n_seq) * 2^-24 relative -- at most 54 * 6e-8 = 3.3e-6 at D = 3072 as a worst case, a few 1e-7 as errors go in
practice; the square root halves it, the quotient of two norms adds them and two more roundings: the per-row ratio is within
(n_seq + 3) * 2^-24 of exact, below 3.5e-6.  The sums over rows are fp64.  So 1e-5 relative is above the worst case and more than
ten times what rounding errors of random sign leave.  The cosine distance has an absolute error of at most
2 * (n_seq + 3) * 2^-24 per row (the dot product's error is relative to sum |a b| <= ||a|| ||b||), so the test first asserts, on
the CPU, that its inputs' mean cosine distance is large enough for 1e-5 relative to cover that."""
import math

import pytest
import torch

from frameino_amd import ops
from tests import magcache_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
ROWS = [1, 2, 63, 64, 65, 257, 1188]
U32 = 2.0 ** -24
SENTINEL = 7.0


def _dims(dtype):
    return [4 if dtype == torch.float32 else 8, 24, 136, 3072]


def _inputs(rows, d, dtype, seed):
    """(x_out, x_in, r_prev) on the CPU: N(0, 1) times a per-row scale in [1/4, 4], r_prev's rows scaled on their own, so the
    per-row ratio varies across rows"""
    g = torch.Generator().manual_seed(seed)
    s_new = 4.0 ** (2 * torch.rand(rows, 1, generator=g) - 1)
    s_prev = 4.0 ** (2 * torch.rand(rows, 1, generator=g) - 1)
    x_out = (torch.randn(rows, d, generator=g) * s_new).to(dtype)
    x_in = (torch.randn(rows, d, generator=g) * s_new).to(dtype)
    r_prev = (torch.randn(rows, d, generator=g) * s_prev).to(dtype)
    return x_out, x_in, r_prev


def _strided(t, pad, extra_rows=0):
    """t on the device as a view of a [rows + extra_rows, D + pad] buffer filled with a sentinel"""
    buf = torch.full((t.shape[0] + extra_rows, t.shape[1] + pad), SENTINEL, dtype=t.dtype, device=DEV)
    buf[:t.shape[0], :t.shape[1]] = t.to(DEV)
    return buf, buf[:t.shape[0], :t.shape[1]]


def _per16(dtype):
    return 4 if dtype == torch.float32 else 8


def _run(x_out, x_in, r_prev, alias, pad):
    """-> (r_new on the CPU, stats on the CPU, whether everything beyond the operand is untouched)"""
    _, xo = _strided(x_out, pad)
    _, xi = _strided(x_in, 2 * pad)
    pbuf, rp = _strided(r_prev, pad, extra_rows=3)
    nbuf, rn = (pbuf, rp) if alias else _strided(torch.zeros_like(r_prev), 3 * pad, extra_rows=3)
    stats = torch.full((2,), -1.0, dtype=torch.float64, device=DEV)
    out = ops.magcache_calibrate(xo, xi, rp, rn, stats)
    assert out is rn
    rows, d = r_prev.shape
    clean = bool((nbuf[rows:] == SENTINEL).all()) and bool((nbuf[:, d:] == SENTINEL).all())
    if not alias:
        clean = clean and torch.equal(rp.cpu(), r_prev)          # the input is only read
    return rn.cpu(), stats.cpu(), clean


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("rows", ROWS)
def test_calibrate_matches_the_restatement(rows, dtype):
    for d in _dims(dtype):
        x_out, x_in, r_prev = _inputs(rows, d, dtype, seed=1000 * rows + d)
        want_r = x_out - x_in                                    # torch's subtraction in T: one fp32 operation, one rounding
        ratio, cos = R.calibration(want_r, r_prev)
        # conditions on the inputs, checked on the CPU: the mean of the ratios is not the ratio of the mean norms (a kernel
        # that averaged norms would fail), and the cosine distance is large enough for the relative tolerance (see above)
        if rows > 1:
            assert abs(ratio - R.mean_norm_ratio(want_r, r_prev)) > 1e-3 * ratio, (rows, d)
        n_seq = math.ceil(d / _per16(dtype) / 64) * _per16(dtype) + 6
        assert cos * 1e-5 >= 2 * (n_seq + 3) * U32, (rows, d, cos)
        residual = ops.step_cache_residual(x_out.to(DEV), x_in.to(DEV), subtract=True).cpu()
        assert torch.equal(residual, want_r)
        first = None
        for alias in (False, True):
            for pad in (0, 2 * _per16(dtype)):                   # contiguous rows, and views of wider buffers
                r_new, stats, clean = _run(x_out, x_in, r_prev, alias, pad)
                assert torch.equal(r_new, residual), (d, alias, pad)
                assert clean, (d, alias, pad)
                assert abs(stats[0].item() - ratio) <= 1e-5 * ratio, (d, alias, pad, stats[0].item(), ratio)
                assert abs(stats[1].item() - cos) <= 1e-5 * cos, (d, alias, pad, stats[1].item(), cos)
                # the same inputs give the same bits: every launch of this shape, aliased or not, strided or not
                first = stats if first is None else first
                assert torch.equal(stats, first), (d, alias, pad)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
def test_two_launches_give_the_same_bits(dtype):
    x_out, x_in, r_prev = _inputs(1188, 3072, dtype, seed=3)
    xo, xi, rp = x_out.to(DEV), x_in.to(DEV), r_prev.to(DEV)
    outs = []
    for _ in range(2):
        rn, stats = torch.empty_like(rp), torch.zeros(2, dtype=torch.float64, device=DEV)
        ops.magcache_calibrate(xo, xi, rp, rn, stats)
        outs.append((rn.cpu(), stats.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert outs[0][1].dtype == torch.float64 and bool(torch.isfinite(outs[0][1]).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
def test_a_zero_previous_row_follows_the_formula(dtype):
    """an all-zero r_prev row: ratio = ||r_new|| / 1e-8 and cosine distance 1 - 0 / 1e-8 = 1, both finite"""
    rows, d = 5, 136
    x_out, x_in, r_prev = _inputs(rows, d, dtype, seed=4)
    r_prev[2] = 0
    ratio, cos = R.calibration(x_out - x_in, r_prev)
    assert ratio > 1e6                                           # the zero row dominates the mean: it is what is compared
    r_new, stats, _ = _run(x_out, x_in, r_prev, False, 0)
    assert bool(torch.isfinite(stats).all())
    assert abs(stats[0].item() - ratio) <= 1e-5 * ratio and abs(stats[1].item() - cos) <= 1e-5 * cos
    # ... and an all-zero new residual (x_out == x_in): ratio 0, distance 1 on every row
    _, stats, _ = _run(x_in, x_in, r_prev, False, 0)
    assert stats.tolist() == [0.0, 1.0]


def test_the_front_end_checks_its_operands():
    x = torch.zeros(4, 8, dtype=torch.bfloat16, device=DEV)
    stats = torch.zeros(2, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="r_prev is"):
        ops.magcache_calibrate(x, x, x[:2], x, stats)
    with pytest.raises(ValueError, match="x_in"):
        ops.magcache_calibrate(x, x.half(), x, x, stats)
    with pytest.raises(ValueError, match="stats must be"):
        ops.magcache_calibrate(x, x, x, x, stats.float())
    with pytest.raises(ValueError, match="stats must be"):
        ops.magcache_calibrate(x, x, x, x, torch.zeros(3, dtype=torch.float64, device=DEV))
