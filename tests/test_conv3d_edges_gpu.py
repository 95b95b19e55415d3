"""fino_conv3d / fino_conv3d_split (the implicit GEMM behind every Wan VAE convolution) at the edges of BOTH of its main
loops, in bf16 and fp16 and as the split-bf16 fp32 product, judged PER ELEMENT against a float64 reference.

THE BOUND (tests/conv_ref.py derives it; tests/test_conv_ref_cpu.py shows that it rejects a dropped 16-byte granule, a
one-pixel shift, a clamped time tap and an unclamped tile base on every geometry below).  Operands are exact in the storage
type (values on the grid bf16 and fp16 share, so one reference serves both), the MFMA accumulates K exact products in fp32:
    |got - ref| <= roundings * u_T * |ref| + 2 * K * 2^-24 * S,      S = conv(|x|, |w|) + |b|,  K = kt*kh*kw*c_in_pad
u_T = 2^-8 (bf16) / 2^-11 (fp16); 2 K 2^-24 S is the recursive-summation bound with a factor 2 for an accumulate that need
not round to nearest.  roundings = 1: gemm_epilogue_t (fino_gemm_common.h) converts the accumulator exactly once, y =
T::from_f32(acc + bias), on its way into the LDS tile, and FINO_EPI_NONE stores those bits.  FINO_EPI_RESIDUAL reads that
T value back, adds r in fp32 and packs again -- so the residual run is held to the BITS of (y.float() + r.float()).to(T) of the
plain run, not to a bound with two roundings.  Split conv (fp32 out): the first term is drop * S with drop = the weight of the
products ops.SPLIT_PRODUCTS leaves out, ~3 * 2^-16 (2 planes) / ~4 * 2^-24 (3 planes), and K counts the 3 / 6 products.
No element is excused: the cap on excluded elements is 0.

EVERY ROW (BM = BN = 256, BK = 64; M = To*Ho*Wo; `default` = the loop conv3d_impl picks with no tune key, which
tests/conv_ref.py::expected_loop restates; every ping-pong row runs a second time on the one-barrier loop, tune key 2 = 1):
  causal-3tiles    3x3x3 pad (2,1,1), (7,9,11), 64 -> 64.  default ping-pong.  M = 693: tiles of 256, 256, 181 rows.  Tile 1
                   starts mid-frame at t_first = 2, base max(0, 0) = 0; tile 2 at t_first = 5, base 3 > 0; cin_chunks = 1.
  causal-midrow    3x3x3 pad (2,1,1), (3,17,19), 128 -> 320.  default ping-pong.  hw = 323 > 256: tile 1 starts at (0, 13, 9)
                   with a base that is negative before the clamp; M = 969, four tiles, last ragged (201).  N tile 1 has 64
                   columns: w_pieces = 2; gemm_load_bias fast on N tile 0, per element on N tile 1.
  many-frames      3x3x3 pad (2,1,1), (70,2,2), 64 -> 64.  default ping-pong.  hw = 4: tile 0 spans 64 frames (t_span = 65);
                   tile 1 has 24 rows at t_first = 64; 5 of the 9 spatial taps of every row are padding.
  one-pixel        3x3x3 pad (2,1,1), (300,1,1), 64 -> 64.  default ONE-BARRIER (t_span = 256 does not fit 8 bits).  M = 300;
                   every non-centre spatial tap is padding.
  time-down        3x1x1 stride (2,1,1), (41,4,5), 64 -> 128.  default ping-pong.  M = 400; tile 1: t_first = 12, base 24.
  space-down       1x3x3 stride (1,2,2) pad 0, (3,20,22) -> (3,10,11), 64 -> 64.  default ping-pong.  One implicit zero row
                   and column at the far edge; M = 330.
  up2x             1x3x3 pad (0,1,1) on the 2x upsample of (3,7,9), 128 -> 256.  default ping-pong.  hi >> 1, wi >> 1 on odd
                   sizes; M = 756 (256, 256, 244); N is exactly one full tile (bias fast branch).
  1x1-nk1          1x1x1, (3,10,11), 64 -> 512.  default ping-pong.  nk = 1: no second prologue stage; two full N tiles.
  1x1-nk3          1x1x1, (3,10,11), 192 -> 64.  default ping-pong.  nk = 3 (odd), cin_chunks = 3.
  time-conv-wideK  3x1x1 pad (2,0,0), (6,7,9), 320 -> 96.  default ping-pong.  cin_chunks = 5, nk = 15, w_pieces = 3; M = 378.
  narrow-N         1x3x3 pad (0,1,1), (2,12,13), 64 -> 72.  default ONE-BARRIER (c_out_pad % 32 != 0); the split conv refuses.

GUARDS.  x is frames [1, T] of a tensor whose frames 0 and T + 1 are NaN, the output rows [G, G + M) of a buffer whose other
rows hold a sentinel: a tap that reads a frame outside [0, T) turns the result into NaN, a store past row M - 1 (or in front
of row 0) changes a sentinel.  Both are ordinary accesses inside an allocation."""
import functools

import pytest
import torch

from tests.conv_ref import (BM, BN, GEOM_BY_ID, GEOMS, SPLIT_NPROD, SPLIT_ROWS, bound, conv_ref64, expected_loop,
                            make_operands, out_thw, taps)

pytestmark = pytest.mark.gpu
DEV = "cuda"
FINO_TUNE_CONV_LOOP = 2
GUARD_ROWS = 300                   # more than one tile of sentinel rows on either side of the output
SENTINEL = -1536.0                 # exact in bf16, fp16 and fp32; far outside the outputs (|y| < 10)
DTYPES = [torch.bfloat16, torch.float16]


@functools.lru_cache(maxsize=None)
def _case(gid):
    """operands on the common bf16 / fp16 grid and the float64 reference: once per geometry, shared by dtypes and loops"""
    g = GEOM_BY_ID[gid]
    x, w, b, cout = make_operands(g)
    ref, s = conv_ref64(x, w, b, g.kernel, g.stride, g.pad, g.up, out_thw(g))
    return x, w, b, cout, ref, s


@functools.lru_cache(maxsize=None)
def _case_f32(gid):
    """plain fp32 operands (the split conv's inputs) and the float64 reference on them, unrounded"""
    g = GEOM_BY_ID[gid]
    x, w, b, cout = make_operands(g, seed=1, exact16=False)
    ref, s = conv_ref64(x, w, b, g.kernel, g.stride, g.pad, g.up, out_thw(g))
    return x, w, b, cout, ref, s


@pytest.fixture
def conv_loop(request):
    """the conv loop under test: 0 = what conv3d_impl picks, 1 = the one-barrier loop (FINO_TUNE_CONV_LOOP)"""
    from frameino_amd import _lib
    _lib.lib().fino_tune_set(FINO_TUNE_CONV_LOOP, request.param)
    try:
        yield request.param
    finally:
        _lib.lib().fino_tune_set(FINO_TUNE_CONV_LOOP, 0)


def _guarded_input(x, dtype):
    """x [T, H, W, C] as the contiguous slice [1 : T + 1] of a tensor with a NaN frame on either side"""
    t = x.shape[0]
    big = torch.full((t + 2,) + tuple(x.shape[1:]), float("nan"), dtype=dtype, device=DEV)
    big[1:t + 1] = x.to(DEV).to(dtype)
    xin = big[1:t + 1]
    assert xin.is_contiguous() and xin.data_ptr() % 16 == 0
    return big, xin


def _guarded_output(shape, dtype):
    m, n = shape[0] * shape[1] * shape[2], shape[3]
    big = torch.full((m + 2 * GUARD_ROWS, n), SENTINEL, dtype=dtype, device=DEV)
    out = big[GUARD_ROWS:GUARD_ROWS + m].view(shape)
    assert out.is_contiguous() and out.data_ptr() % 16 == 0
    return big, out


def _sentinels_untouched(big, m):
    return bool((big[:GUARD_ROWS] == SENTINEL).all()) and bool((big[GUARD_ROWS + m:] == SENTINEL).all())


def _assert_within(got, ref, bnd, what):
    """every element inside the bound (none excused); on failure name the worst one and its tiles"""
    got = got.double().cpu()
    assert got.shape == ref.shape
    assert not torch.isnan(got).any(), f"{what}: NaN in the output -- a tap read a guard frame outside [0, T)"
    diff = (got - ref).abs()
    ratio = torch.where(bnd > 0, diff / bnd.clamp_min(1e-300), torch.where(diff > 0, float("inf"), 0.0).double())
    worst = int(ratio.argmax())
    _, ho, wo, n = ref.shape
    c, row = worst % n, worst // n
    t, h, w = row // (ho * wo), (row // wo) % ho, row % wo
    print(f"{what}: worst |got - ref| / bound = {ratio.max().item():.3g} at (t, h, w, c) = ({t}, {h}, {w}, {c})")
    bad = int((diff > bnd).sum())
    assert bad == 0, (f"{what}: {bad} elements outside the bound; worst at (t, h, w, c) = ({t}, {h}, {w}, {c}), M tile {row // BM}, "
                      f"N tile {c // BN}: got {got.flatten()[worst].item()!r}, ref {ref.flatten()[worst].item()!r}, "
                      f"bound {bnd.flatten()[worst].item()!r}")
    return ratio.max().item()


_CASES = [(g.id, 0) for g in GEOMS] + [(g.id, 1) for g in GEOMS if expected_loop(g) == "pingpong"]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("gid,conv_loop", _CASES, indirect=["conv_loop"],
                         ids=[f"{gid}-{'one_barrier_forced' if f else 'default'}" for gid, f in _CASES])
def test_conv3d_edges_per_element(gid, conv_loop, dtype):
    from frameino_amd import _lib, ops
    g = GEOM_BY_ID[gid]
    assert _lib.lib().fino_tune_get(FINO_TUNE_CONV_LOOP) == conv_loop
    assert expected_loop(g) == g.loop                       # the default loop of this row is the one the docstring names
    loop = expected_loop(g, tune=conv_loop)
    x, w, b, cout, ref, s = _case(gid)
    shape = out_thw(g) + (g.cout_pad,)
    m = shape[0] * shape[1] * shape[2]
    xbig, xin = _guarded_input(x, dtype)
    wd, bd = w.to(DEV).to(dtype), b.to(DEV).to(dtype)
    assert torch.equal(xin.float().cpu(), x) and torch.equal(wd.float().cpu(), w) and torch.equal(bd.float().cpu(), b)

    def run(residual=None):
        big, out = _guarded_output(shape, dtype)
        y = ops.conv3d_cl(xin, wd, bd, g.kernel, g.stride, g.pad, out_thw(g), g.up, residual=residual, out=out)
        torch.cuda.synchronize()
        assert y.data_ptr() == out.data_ptr()
        assert _sentinels_untouched(big, m), f"{gid} {loop}: a store outside output rows [0, {m})"
        return y

    y = run()
    what = f"{gid} {str(dtype).split('.')[1]} {loop}"
    _assert_within(y, ref, bound(ref, s, taps(g) * g.cin_pad, dtype), what)
    assert bool((y[..., cout:] == 0).all()), f"{what}: pad output channels (zero weights and bias) must be exactly 0"
    # residual epilogue: the T-rounded y plus r in fp32, rounded once more -- the bits of the plain run decide
    gen = torch.Generator().manual_seed(7)
    r = torch.randn(shape, generator=gen).to(DEV).to(dtype)
    y_res = run(residual=r)
    assert torch.equal(y_res, (y.float() + r.float()).to(dtype)), f"{what}: residual epilogue"
    assert torch.equal(run(), y), f"{what}: a second launch gives other bits"


# ------------------------------------------------------------------------------------------------ split-bf16 (fp32) conv
def _split_operands(ops, g, x, w, b, planes):
    t = x.shape[0]
    xbig = torch.full((t + 2,) + tuple(x.shape[1:3]) + (planes * g.cin_pad,), float("nan"), dtype=torch.bfloat16, device=DEV)
    xp = ops.split_bf16(x.to(DEV), "planes", planes, out=xbig[1:t + 1])
    assert xp.data_ptr() == xbig[1:t + 1].data_ptr() and bool(torch.isnan(xbig[0]).all()) and bool(torch.isnan(xbig[t + 1]).all())
    w6 = ops.split_bf16(w.reshape(g.cout_pad * taps(g), g.cin_pad).to(DEV).contiguous(), "W", planes).reshape(g.cout_pad, -1)
    return xbig, xp, w6, b.to(DEV)


@pytest.mark.parametrize("planes", [2, 3])
@pytest.mark.parametrize("gid", SPLIT_ROWS)
def test_conv3d_split_edges_per_element(gid, planes):
    from frameino_amd import ops
    g = GEOM_BY_ID[gid]
    assert expected_loop(g, planes) == "pingpong"
    x, w, b, cout, ref, s = _case_f32(gid)
    shape = out_thw(g) + (g.cout_pad,)
    m = shape[0] * shape[1] * shape[2]
    xbig, xp, w6, bd = _split_operands(ops, g, x, w, b, planes)

    def run(residual=None):
        big, out = _guarded_output(shape, torch.float32)
        y = ops.conv3d_split_cl(xp, w6, bd, g.kernel, planes, g.stride, g.pad, out_thw(g), g.up, residual=residual, out=out)
        torch.cuda.synchronize()
        assert y.data_ptr() == out.data_ptr() and y.dtype == torch.float32
        assert _sentinels_untouched(big, m), f"{gid} split{planes}: a store outside output rows [0, {m})"
        return y

    y = run()
    what = f"{gid} split{planes} pingpong"
    _assert_within(y, ref, bound(ref, s, taps(g) * g.cin_pad * SPLIT_NPROD[planes], torch.float32, planes=planes), what)
    assert bool((y[..., cout:] == 0).all()), f"{what}: pad output channels must be exactly 0"
    r = torch.randn(shape, generator=torch.Generator().manual_seed(7)).to(DEV)
    assert torch.equal(run(residual=r), y + r), f"{what}: one fp32 add in the epilogue"
    assert torch.equal(run(), y), f"{what}: a second launch gives other bits"


def test_conv3d_split_refuses_a_narrow_n():
    """the split conv has no one-barrier loop to fall to: c_out_pad % 32 != 0 is an error, not another kernel"""
    from frameino_amd import ops
    g = GEOM_BY_ID["narrow-N"]
    assert expected_loop(g, 3) == "one_barrier"
    x, w, b, _, _, _ = _case_f32(g.id)
    _, xp, w6, bd = _split_operands(ops, g, x, w, b, 3)
    with pytest.raises(RuntimeError, match=r"fino_conv3d_split failed \(-3\).*c_out_pad % 32 != 0"):     # FINO_ERR_UNSUPPORTED
        ops.conv3d_split_cl(xp, w6, bd, g.kernel, 3, g.stride, g.pad, out_thw(g), g.up)


# ------------------------------------------------------------------------------------------------ argument rejections
def _small(cin=64, cout=64, dtype=torch.bfloat16):
    x = torch.zeros(2, 3, 4, cin, dtype=dtype, device=DEV)
    w = torch.zeros(cout, cin, dtype=dtype, device=DEV)
    b = torch.zeros(cout, dtype=dtype, device=DEV)
    return x, w, b


def test_rejects_c_in_pad_96():
    from frameino_amd import ops
    x, w, b = _small(cin=96)
    with pytest.raises(RuntimeError, match=r"fino_conv3d failed \(-1\).*c_in_pad=96 must be a multiple of 64"):
        ops.conv3d_cl(x, w, b, (1, 1, 1))


def test_rejects_c_out_pad_20():
    from frameino_amd import ops
    x, w, b = _small(cout=20)
    with pytest.raises(RuntimeError, match=r"fino_conv3d failed \(-1\).*c_out_pad=20 % 8 != 0"):
        ops.conv3d_cl(x, w, b, (1, 1, 1))


def test_rejects_a_residual_epilogue_without_r():
    from frameino_amd import _lib, ops
    x, w, b = _small()
    out = torch.empty(2, 3, 4, 64, dtype=x.dtype, device=DEV)
    with pytest.raises(RuntimeError, match=r"fino_conv3d failed \(-1\).*epilogue 2 \(NONE or RESIDUAL with r\)"):
        _lib.check(_lib.lib().fino_conv3d(x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), 2, 3, 4, 64, 2, 3, 4, 64,
                                          1, 1, 1, 1, 1, 1, 0, 0, 0, 0, ops.EPI_RESIDUAL, None,
                                          ops.zero_page(x.device).data_ptr(), ops.BF16, None), "fino_conv3d")


def test_rejects_a_misaligned_x():
    from frameino_amd import ops
    _, w, b = _small()
    flat = torch.zeros(2 * 3 * 4 * 64 + 8, dtype=torch.bfloat16, device=DEV)
    x = flat[1:1 + 2 * 3 * 4 * 64].view(2, 3, 4, 64)                   # offset by one element: 2 bytes off the 16-byte grid
    assert x.is_contiguous() and x.data_ptr() % 16 == 2
    with pytest.raises(RuntimeError, match=r"fino_conv3d failed \(-1\).*16-byte alignment required"):
        ops.conv3d_cl(x, w, b, (1, 1, 1))


def test_rejects_a_zero_t_out():
    from frameino_amd import ops
    x, w, b = _small()
    out = torch.empty(2, 3, 4, 64, dtype=x.dtype, device=DEV)          # (a real buffer: the null-pointer check comes first)
    with pytest.raises(RuntimeError, match=r"fino_conv3d failed \(-1\).*bad geometry"):
        ops.conv3d_cl(x, w, b, (1, 1, 1), out_thw=(0, 3, 4), out=out)
