"""fino_teacache_probe (ops.teacache_probe) against the fp64 restatement of TeaCache's probe (tests/teacache_ref.py): the stored
plane bit-equal to ops.adaln_modulate, the two sums to relative 1e-5, bit-identical reruns, untouched rows and columns beyond
the operands, the plain mode, `compare=False`, an all-zero previous plane, the front end's operand checks.

The tolerance.  A row's two fp32 sums run over non-negative terms |m - p| and |p| of the rounded values: a term is one fp32
operation (one rounding; |p| none), a lane adds its ceil(vpr / 64) vectors of 8 elements in sequence, then six butterfly levels,
so a row sum carries at most (ceil(vpr / 64) * 8 + 6 + 1) * 2^-24 relative -- 55 * 6e-8 = 3.3e-6 at D = 3072 (vpr = 384), below
3.5e-6, as a worst case; a few 1e-7 as errors of random sign go in practice.  A row sum is exact in fp64 and the sums across rows
are fp64 sums of non-negative numbers, whose own error (2^-53 per addition) is nothing beside that.  So each of the two sums is
within 3.5e-6 relative of exact and 1e-5 is above the worst case.  For that to mean something the distance d = sum|m - p| /
sum|p| of the test's inputs must not be tiny or huge (a sum of near-cancelling differences is still a sum of non-negative terms,
so the bound holds anyway, but a d near 0 would compare noise): the test asserts on the CPU that d lies in [0.05, 2]."""
import math

import pytest
import torch

from frameino_amd import ops
from tests import teacache_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
ROWS = [1, 2, 63, 64, 65, 257, 1188]
DIMS = [8, 24, 136, 192, 3072]
SENTINEL = 7.0
TOL = 1e-5
EPS = 1e-6


def _inputs(rows, d, dtype, seed, two_rows):
    """(x, x_prev, table [R, 2, D] fp32, sel or None) on the CPU: x = N(0, 1) times a per-row scale in [1/4, 4] plus a per-row
    offset, x_prev = x moved by 0.3 of its scale, so the modulated planes differ by a few tenths"""
    g = torch.Generator().manual_seed(seed)
    s = 4.0 ** (2 * torch.rand(rows, 1, generator=g) - 1)
    x = (torch.randn(rows, d, generator=g) * s + torch.randn(rows, 1, generator=g)).to(dtype)
    x_prev = (x.float() + 0.3 * s * torch.randn(rows, d, generator=g)).to(dtype)
    table = 0.5 * torch.randn(2 if two_rows else 1, 2, d, generator=g)
    sel = torch.randint(0, 2, (rows,), generator=g, dtype=torch.int32) if two_rows else None
    if sel is not None and rows > 1:
        sel[0], sel[-1] = 0, 1                                   # mixed, whatever the draw
    return x, x_prev, table, sel


def _strided(t, pad, extra_rows=0):
    """t on the device as a view of a [rows + extra_rows, D + pad] buffer filled with a sentinel"""
    buf = torch.full((t.shape[0] + extra_rows, t.shape[1] + pad), SENTINEL, dtype=t.dtype, device=DEV)
    buf[:t.shape[0], :t.shape[1]] = t.to(DEV)
    return buf, buf[:t.shape[0], :t.shape[1]]


def _mod(table, sel):
    t = table.to(DEV)
    return t[:, 0], t[:, 1], None if sel is None else sel.to(DEV)


def _run(x, prev_plane, table, sel, pad, compare=True, plain=False):
    """-> (plane on the CPU, stats on the CPU, whether everything beyond the operands is untouched and x is only read)"""
    xbuf, xv = _strided(x, pad)
    pbuf, pv = _strided(prev_plane, 2 * pad, extra_rows=3)
    stats = torch.full((2,), -1.0, dtype=torch.float64, device=DEV)
    if plain:
        out = ops.teacache_probe(xv, pv, stats, compare=compare)
    else:
        shift, scale, s = _mod(table, sel)
        out = ops.teacache_probe(xv, pv, stats, shift, scale, s, EPS, compare=compare)
    assert out is pv
    rows, d = x.shape
    clean = bool((pbuf[rows:] == SENTINEL).all()) and bool((pbuf[:, d:] == SENTINEL).all())
    clean = clean and bool((xbuf[:, d:] == SENTINEL).all()) and torch.equal(xv.cpu(), x)
    return pv.cpu(), stats.cpu(), clean


def _close(got, want):
    return abs(got - want) <= TOL * want


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("rows", ROWS)
def test_probe_matches_the_restatement(rows, dtype):
    for d in DIMS:
        for two_rows in (False, True):
            x, x_prev, table, sel = _inputs(rows, d, dtype, 1000 * rows + d + two_rows, two_rows)
            shift, scale, s = _mod(table, sel)
            want_m = ops.adaln_modulate(x.to(DEV), shift, scale, s, EPS).cpu()
            prev = ops.adaln_modulate(x_prev.to(DEV), shift, scale, s, EPS).cpu()
            # the restatement in plain torch agrees with the modulate kernel to the last bit or the one next to it
            ref_m = R.modulated(x, table[:, 0], table[:, 1], sel, EPS)
            assert (want_m.float() - ref_m.float()).abs().max() <= 2.0 ** -7 * ref_m.float().abs().max()
            sa, sq = R.sums(want_m, prev)
            assert 0.05 <= sa / sq <= 2.0, (rows, d, sa / sq)      # a condition on the inputs, checked on the CPU
            vpr = d // 8
            assert (math.ceil(vpr / 64) * 8 + 7) * 2.0 ** -24 < 3.5e-6 < TOL
            first = None
            for pad in (0, 16):                                  # contiguous rows, and views of wider buffers
                plane, stats, clean = _run(x, prev, table, sel, pad)
                assert torch.equal(plane, want_m), (d, two_rows, pad)
                assert clean, (d, two_rows, pad)
                assert _close(stats[0].item(), sa) and _close(stats[1].item(), sq), (d, two_rows, pad, stats.tolist(), sa, sq)
                first = stats if first is None else first
                assert torch.equal(stats, first), (d, two_rows, pad)     # the same inputs: the same bits, strided or not


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_two_launches_give_the_same_bits(dtype):
    x, x_prev, table, sel = _inputs(1188, 3072, dtype, 3, True)
    shift, scale, s = _mod(table, sel)
    xd, prev = x.to(DEV), ops.adaln_modulate(x_prev.to(DEV), shift, scale, s, EPS)
    outs = []
    for _ in range(2):
        plane, stats = prev.clone(), torch.zeros(2, dtype=torch.float64, device=DEV)
        ops.teacache_probe(xd, plane, stats, shift, scale, s, EPS)
        outs.append((plane.cpu(), stats.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert outs[0][1].dtype == torch.float64 and bool(torch.isfinite(outs[0][1]).all()) and bool((outs[0][1] > 0).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("rows,d", [(1, 8), (65, 24), (257, 192), (1188, 136), (63, 3072)])
def test_plain_mode_stores_x_and_measures_it(rows, d, dtype):
    """shift = scale = None: m = x, the measurement a calibrating run takes over the head's output rows"""
    x, x_prev, _, _ = _inputs(rows, d, dtype, 7 * rows + d, False)
    sa, sq = R.sums(x, x_prev)
    assert 0.05 <= sa / sq <= 2.0
    for pad in (0, 8):
        plane, stats, clean = _run(x, x_prev, None, None, pad, plain=True)
        assert torch.equal(plane, x) and clean
        assert _close(stats[0].item(), sa) and _close(stats[1].item(), sq), (pad, stats.tolist(), sa, sq)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_without_compare_the_plane_is_stored_and_not_read(dtype):
    rows, d = 65, 136
    x, _, table, sel = _inputs(rows, d, dtype, 11, True)
    shift, scale, s = _mod(table, sel)
    want_m = ops.adaln_modulate(x.to(DEV), shift, scale, s, EPS).cpu()
    garbage = torch.full((rows, d), float("nan"), dtype=dtype)      # what an unwritten plane may hold
    plane, stats, clean = _run(x, garbage, table, sel, 16, compare=False)
    assert torch.equal(plane, want_m) and clean and stats.tolist() == [0.0, 0.0]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_an_all_zero_previous_plane_gives_the_sum_of_m_and_zero(dtype):
    rows, d = 257, 192
    x, _, table, sel = _inputs(rows, d, dtype, 13, False)
    shift, scale, s = _mod(table, sel)
    want_m = ops.adaln_modulate(x.to(DEV), shift, scale, s, EPS).cpu()
    plane, stats, clean = _run(x, torch.zeros(rows, d, dtype=dtype), table, sel, 0)
    assert torch.equal(plane, want_m) and clean
    assert _close(stats[0].item(), float(want_m.double().abs().sum())) and stats[1].item() == 0.0


def test_the_front_end_checks_its_operands():
    x = torch.zeros(4, 8, dtype=torch.bfloat16, device=DEV)
    plane = torch.zeros_like(x)
    stats = torch.zeros(2, dtype=torch.float64, device=DEV)
    table = torch.zeros(1, 2, 8, device=DEV)
    with pytest.raises(ValueError, match="plane is"):
        ops.teacache_probe(x, plane[:2], stats)
    with pytest.raises(ValueError, match="plane"):
        ops.teacache_probe(x, plane.half(), stats)
    with pytest.raises(TypeError, match="bf16 or fp16"):
        ops.teacache_probe(x.float(), plane.float(), stats)
    with pytest.raises(ValueError, match="stats must be"):
        ops.teacache_probe(x, plane, stats.float())
    with pytest.raises(ValueError, match="stats must be"):
        ops.teacache_probe(x, plane, torch.zeros(3, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="come together"):
        ops.teacache_probe(x, plane, stats, shift=table[:, 0])
    with pytest.raises(ValueError, match="selector needs"):
        ops.teacache_probe(x, plane, stats, sel=torch.zeros(4, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="sel must be"):
        ops.teacache_probe(x, plane, stats, table[:, 0], table[:, 1], torch.zeros(3, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="shift must be"):
        ops.teacache_probe(x, plane, stats, table[:, 0].half(), table[:, 1])
    with pytest.raises(RuntimeError, match="the plane is x itself"):
        ops.teacache_probe(x, x, stats)
    with pytest.raises(ValueError, match="no rows"):
        ops.teacache_probe(x[:0], plane[:0], stats)
