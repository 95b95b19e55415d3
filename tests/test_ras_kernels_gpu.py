"""The kernels of region-adaptive sampling (csrc/fino_token_select.hip, fino_qkv_rmsnorm_rope_rows) against their restatements in
tests/ras_ref.py and against the kernels whose arithmetic they repeat.

token_score: the fp32 two-pass standard deviation of at most 192 values against float64 -- every fp32 sum of m <= 192 terms
carries a relative error of at most ~m * 2^-24 = 1.1e-5 in the worst case and ~sqrt(m) * 2^-24 = 8e-7 typically, the square
root halves it, expf adds ~1e-7: 2e-5 relative.  Everything else is exact: `torch.equal`."""
import math

import pytest
import torch

from frameino_amd import ops
from tests import ras_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ------------------------------------------------------------------ token_score
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("shape", [(1188, 192), (1188, 5)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_token_score_against_float64(shape, batch, dtype):
    n, cols = shape
    g = torch.Generator().manual_seed(n + cols + batch)
    po = (torch.randn(batch * n, cols, generator=g) * (0.25 + torch.rand(batch * n, 1, generator=g)) + 0.5).to(dtype)
    counters = torch.randint(0, 12, (n,), generator=g, dtype=torch.int32)
    elig = torch.ones(n, dtype=torch.uint8)
    elig[:99], elig[500:507] = 0, 2
    plain = ops.token_score(po.to(DEV), batch=batch).cpu().double()
    want = R.score_ref(po, batch)
    err = float(((plain - want).abs() / want).max())
    print(f"token_score {shape} batch {batch} {dtype}: max relative error {err:.3e} (bound 2e-5)")
    assert err < 2e-5
    got = ops.token_score(po.to(DEV), batch=batch, counters=counters.to(DEV), starvation_scale=0.1, eligible=elig.to(DEV))
    want = R.score_ref(po, batch, counters, 0.1, elig)
    fin = torch.isfinite(want)
    assert torch.equal(got.cpu().double()[~fin], want[~fin]) and int((~fin).sum()) == 106         # -inf / +inf rows, exactly
    assert float(((got.cpu().double()[fin] - want[fin]).abs() / want[fin]).max()) < 2e-5
    again = ops.token_score(po.to(DEV), batch=batch, counters=counters.to(DEV), starvation_scale=0.1, eligible=elig.to(DEV))
    assert torch.equal(got, again)                                                              # the same bits on every launch


def test_token_score_reads_a_row_stride():
    g = torch.Generator().manual_seed(1)
    wide = torch.randn(64, 200, generator=g).bfloat16().to(DEV)
    assert torch.equal(ops.token_score(wide[:, :192]), ops.token_score(wide[:, :192].contiguous()))


# ------------------------------------------------------------------ token_select
@pytest.fixture(scope="module", params=[1188, 65536])
def scores(request):
    n = request.param
    s = R.quantised_scores(n)
    g = torch.Generator().manual_seed(n)
    counters = torch.randint(0, 9, (n,), generator=g, dtype=torch.int32)
    order = sorted(range(n), key=lambda i: (-float(s[i]), i))          # computed once, shared by every k
    return n, s, counters, order


@pytest.mark.parametrize("k", [1, 64, 475, -1, 0], ids=["1", "64", "475", "n-1", "n"])
def test_token_select_is_the_stable_selection(scores, k):
    n, s, counters, order = scores
    k = k if k > 0 else n + k
    want = torch.tensor(sorted(order[:k]), dtype=torch.int32)
    want_counters = counters + 1
    want_counters[want.long()] = 0
    c1, c2 = counters.to(DEV), counters.to(DEV)
    got = ops.token_select(s.to(DEV), k, counters=c1)
    assert got.dtype == torch.int32 and torch.equal(got.cpu(), want)
    assert torch.equal(c1.cpu(), want_counters)
    again = ops.token_select(s.to(DEV), k, counters=c2)                 # two launches: the same bits
    assert torch.equal(again, got) and torch.equal(c1, c2)
    if k < n - int((s == -math.inf).sum()):
        assert not bool((s[got.cpu().long()] == -math.inf).any())       # -inf rows stay off while anything else is left
    if k >= int((s == math.inf).sum()):
        on = torch.zeros(n, dtype=torch.bool)
        on[got.cpu().long()] = True
        assert bool(on[s == math.inf].all())                            # +inf rows are always on


def test_token_select_without_counters_with_nans_and_its_limits():
    s = torch.tensor([0.5, float("nan"), 2.0, -math.inf, 0.5, -0.0, 0.0, 3.0])
    assert ops.token_select(s.to(DEV), 3).tolist() == [0, 2, 7]
    assert ops.token_select(s.to(DEV), 5).tolist() == [0, 2, 4, 5, 7]      # -0 ties with +0: the lower index
    assert ops.token_select(s.to(DEV), 7).tolist() == [0, 1, 2, 4, 5, 6, 7]      # a NaN ranks with -inf: the lower index
    with pytest.raises(RuntimeError, match="fino_token_select failed \\(-3\\).*above 65536"):
        ops.token_select(torch.zeros(65537, device=DEV), 10)
    for k in (0, 9):
        with pytest.raises(RuntimeError, match="fino_token_select failed \\(-1\\)"):
            ops.token_select(s.to(DEV), k)


# ------------------------------------------------------------------ gather / scatter
@pytest.mark.parametrize("row_bytes", [384, 6144, 20])
def test_gather_and_scatter_round_trip_and_clamp(row_bytes):
    n, k = 1188, R.LIST_ROWS
    g = torch.Generator().manual_seed(row_bytes)
    if row_bytes % 8 == 0:
        src = torch.randn(n, row_bytes // 2, generator=g).bfloat16()
    else:
        src = torch.randint(-2 ** 31, 2 ** 31 - 1, (n, row_bytes // 4), generator=g, dtype=torch.int64).to(torch.int32)
    idx = torch.randperm(n, generator=g)[:k].sort().values.to(torch.int32)
    got = ops.gather_rows(src.to(DEV), idx.to(DEV))
    assert torch.equal(got.cpu(), src[idx.long()])
    dst = torch.zeros_like(src).to(DEV)
    ops.scatter_rows(got, idx.to(DEV), dst)
    want = torch.zeros_like(src)
    want[idx.long()] = src[idx.long()]
    assert torch.equal(dst.cpu(), want)                                 # the listed rows came back, nothing else was touched
    # a strided source and destination (rows of a wider buffer)
    wide = torch.cat([src, src], dim=1).to(DEV)
    assert torch.equal(ops.gather_rows(wide[:, :src.shape[1]], idx.to(DEV)).cpu(), src[idx.long()])
    # indices outside [0, n) are clamped: a wrong answer, never an access outside the buffer
    bad = torch.tensor([-5, 0, n - 1, n, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32)
    assert torch.equal(ops.gather_rows(src.to(DEV), bad.to(DEV)).cpu(), src[bad.long().clamp(0, n - 1)])
    guard = torch.zeros(n + 2, src.shape[1], dtype=src.dtype, device=DEV)        # one spare row on either side of the target
    rows = src[:3].to(DEV)
    ops.scatter_rows(rows, torch.tensor([-7, 5, n + 3], dtype=torch.int32, device=DEV), guard[1:n + 1])
    assert not bool(guard[0].any()) and not bool(guard[n + 1].any())
    assert torch.equal(guard[1], rows[0]) and torch.equal(guard[6], rows[1]) and torch.equal(guard[n], rows[2])


# ------------------------------------------------------------------ qkv_rmsnorm_rope_rows
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("heads", [2, 24])
def test_qkv_rmsnorm_rope_rows_is_the_in_place_kernel_plus_the_planes(heads, dtype):
    dh, n, k = 128, 1188, R.LIST_ROWS
    d = heads * dh
    g = torch.Generator().manual_seed(heads)
    qkv = torch.randn(k, 3 * d, generator=g).to(dtype).to(DEV)
    wq, wk = (1 + 0.1 * torch.randn(d, generator=g)).to(dtype).to(DEV), (1 + 0.1 * torch.randn(d, generator=g)).to(dtype).to(DEV)
    ang = torch.rand(k, dh // 2, generator=g) * 6.28
    cos, sin = ang.cos().to(DEV), ang.sin().to(DEV)
    idx = torch.randperm(n, generator=g)[:k].sort().values.to(torch.int32).to(DEV)
    want = ops.qkv_rmsnorm_rope_(qkv.clone(), d, wq, 1e-6, wk, 1e-6, cos, sin, dh)
    planes = torch.randn(2, n, d, generator=g).to(dtype).to(DEV)
    before = planes.clone()
    got = ops.qkv_rmsnorm_rope_rows_(qkv.clone(), d, wq, 1e-6, wk, 1e-6, cos, sin, dh, idx, planes[0], planes[1])
    assert torch.equal(got, want)                                       # q and k in place as the in-place kernel, v untouched
    assert torch.equal(planes[0][idx.long()], want[:, d:2 * d]) and torch.equal(planes[1][idx.long()], want[:, 2 * d:])
    other = torch.ones(n, dtype=torch.bool, device=DEV)
    other[idx.long()] = False
    assert torch.equal(planes[:, other], before[:, other]) and int(other.sum()) == n - k       # every other row untouched
    # without a list row r goes to row r; a folded q scale as the in-place kernel's
    planes2 = before.clone()
    got = ops.qkv_rmsnorm_rope_rows_(qkv.clone(), d, wq, 1e-6, wk, 1e-6, cos, sin, dh, None, planes2[0], planes2[1], q_out_scale=0.1275)
    assert torch.equal(got, ops.qkv_rmsnorm_rope_(qkv.clone(), d, wq, 1e-6, wk, 1e-6, cos, sin, dh, q_out_scale=0.1275))
    assert torch.equal(planes2[0][:k], want[:, d:2 * d]) and torch.equal(planes2[:, k:], before[:, k:])
    # a bad list is clamped into the planes
    guard = before[:, :8].clone()
    bad = torch.tensor([-3, 9, 2 ** 31 - 1, 4], dtype=torch.int32, device=DEV)
    ops.qkv_rmsnorm_rope_rows_(qkv[:4].clone(), d, wq, 1e-6, wk, 1e-6, cos[:4].contiguous(), sin[:4].contiguous(), dh, bad,
                               guard[0, 1:7], guard[1, 1:7])
    assert torch.equal(guard[:, 0], before[:, 0]) and torch.equal(guard[:, 7], before[:, 7])
