"""The two TaylorSeer kernels (ops.taylor_update / ops.taylor_predict, csrc/fino_step_cache.hip) against the CPU restatement in
tests/taylorseer_ref.py.  Every operation of the update, and of a prediction without a gate, is one fp32 operation and one
rounding that torch repeats on the CPU, so those results must be equal bit for bit.  With a gate the kernel's last step is one
fused multiply-add of the fp32 prediction, correctly rounded and then rounded to T: the result lies within half an ulp of T
(plus the double rounding through fp32, below that) of the float64 value of x + p * gate with the same fp32 p -- bounds
2**-8 |ref| for bf16 and 2**-11 |ref| + 2**-25 for fp16 (the absolute term: fp16 subnormals)."""
import pytest
import torch

from frameino_amd import ops
from tests import taylorseer_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
T_DTYPES = [torch.bfloat16, torch.float16]
SHAPES = [(rows, dim) for rows in (1, 37, 300) for dim in (8, 264, 3072)]      # one row, one vector; odd sizes; several workgroups


def _factor_dtypes(t):
    return [t, torch.float32, torch.float16 if t == torch.bfloat16 else torch.bfloat16]


def _padded(rows, dim, dtype, gen, pad=8, planes=None, scale=1.0):
    """rows of `dim` elements inside a buffer with a padded leading dimension (the padding holds a sentinel)"""
    shape = (rows, dim + pad) if planes is None else (planes, rows, dim + pad)
    buf = torch.full(shape, 77.0, dtype=dtype)
    view = buf[..., :dim]
    view.copy_((torch.randn(view.shape, generator=gen) * scale).to(dtype))
    return buf, view


def _dev(buf, dim):
    d = buf.to(DEV)
    return d, d[..., :dim]


@pytest.fixture
def gen():
    """seeded per test: a test's operands do not depend on which other tests ran before it"""
    return torch.Generator().manual_seed(31)


# ------------------------------------------------------------------ update
@pytest.mark.parametrize("t", T_DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("rows,dim", SHAPES, ids=[f"{r}x{d}" for r, d in SHAPES])
def test_update_equals_the_restatement(gen, t, rows, dim):
    for f in _factor_dtypes(t):
        for n_old in range(4):
            for delta in (1, 3, 5):
                if rows * dim > 50000 and (delta != 3 and n_old not in (0, 3)):
                    continue                                     # the large shape: every n_old at delta 3, the ends at 1 and 5
                ybuf, y = _padded(rows, dim, t, gen)
                fbuf, planes = _padded(rows, dim, f, gen, planes=4)
                want, n_want = R.update_planes_ref(y, planes, n_old, delta)
                dy, dyv = _dev(ybuf, dim)
                df, dfv = _dev(fbuf, dim)
                n_new = ops.taylor_update(dyv, dfv, n_old, delta)
                assert n_new == n_want == min(n_old + 1, 4)
                got = df.cpu()
                assert torch.equal(got[..., :dim], want), (f, n_old, delta)       # planes at and beyond n_new untouched too
                assert torch.equal(got[..., dim:], fbuf[..., dim:]) and torch.equal(dy.cpu(), ybuf)      # padding, y


def test_update_with_fewer_planes_and_an_explicit_n_new(gen):
    """max_order 1 (two planes) saturates at n = 2; n_new below n_old + 1 rewrites fewer planes"""
    ybuf, y = _padded(37, 264, torch.bfloat16, gen)
    fbuf, planes = _padded(37, 264, torch.bfloat16, gen, planes=2)
    for n_old, n_new in ((0, None), (1, None), (2, None), (2, 1)):
        want, n_want = R.update_planes_ref(y, planes, n_old, 2)
        if n_new is not None:
            want, n_want = torch.cat([want[:n_new], planes[n_new:]]), n_new
        _, dfv = _dev(fbuf, 264)
        assert ops.taylor_update(_dev(ybuf, 264)[1], dfv, n_old, 2, n_new) == n_want
        assert torch.equal(dfv.cpu(), want)


def test_update_propagates_inf_and_nan_as_torch(gen):
    for t in T_DTYPES:
        for f in _factor_dtypes(t):
            ybuf, y = _padded(5, 16, t, gen, pad=0)
            fbuf, planes = _padded(5, 16, f, gen, pad=0, planes=3)
            y[0, :4] = torch.tensor([float("inf"), float("-inf"), float("nan"), 0.0]).to(t)
            planes[0, 0, :4] = torch.tensor([float("inf"), 1.0, 1.0, float("nan")]).to(f)
            planes[1, 1, :3] = torch.tensor([float("inf"), float("nan"), float("-inf")]).to(f)
            y[2, 0] = torch.finfo(t).max
            planes[0, 2, 0] = -torch.finfo(f).max if f != torch.float32 else -3e38
            want, _ = R.update_planes_ref(y, planes, 2, 1)
            dfv = fbuf.to(DEV)
            ops.taylor_update(ybuf.to(DEV), dfv, 2, 1)
            got = dfv.cpu()
            assert torch.equal(got.isnan(), want.isnan()) and torch.equal(got.nan_to_num(0.0), want.nan_to_num(0.0)), (t, f)
            assert want.isnan().any() and want.isinf().any()


# ------------------------------------------------------------------ predict
@pytest.mark.parametrize("t", T_DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("rows,dim", SHAPES, ids=[f"{r}x{d}" for r, d in SHAPES])
def test_predict_without_a_gate_equals_the_restatement(gen, t, rows, dim):
    for f in _factor_dtypes(t):
        fbuf, planes = _padded(rows, dim, f, gen, planes=4)
        xbuf, x = _padded(rows, dim, t, gen)
        _, dfv = _dev(fbuf, dim)
        dx, dxv = _dev(xbuf, dim)
        for n, k in ((1, 2), (2, 1), (2, 4), (3, 3), (4, 2), (4, 5)):
            fl = [planes[i] for i in range(4)]
            assert torch.equal(ops.taylor_predict(dfv, n, k, dtype=t).cpu(), R.predict_ref(fl, n, k, t)), (f, n, k)
            out = torch.full((rows + 3, dim + 8), 5.0, dtype=t, device=DEV)         # rows and columns beyond: not written
            ops.taylor_predict(dfv, n, k, dxv, out=out[:rows, :dim])
            assert torch.equal(out[:rows, :dim].cpu(), R.predict_ref(fl, n, k, t, x)), (f, n, k)
            assert bool((out[rows:] == 5.0).all()) and bool((out[:, dim:] == 5.0).all())
        assert torch.equal(dx.cpu(), xbuf)


@pytest.mark.parametrize("t", T_DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("rows,dim", SHAPES, ids=[f"{r}x{d}" for r, d in SHAPES])
def test_predict_with_a_gate_is_within_half_an_ulp_of_float64(gen, t, rows, dim):
    table = torch.randn(3, 2, dim, generator=gen)                         # a [R, 6, D]-like modulation table: strided gate rows
    gate = table[:, 1]
    sel = torch.randint(0, 3, (rows,), generator=gen, dtype=torch.int32)
    dgate, dsel = table.to(DEV)[:, 1], sel.to(DEV)
    for f in _factor_dtypes(t):
        fbuf, planes = _padded(rows, dim, f, gen, planes=4)
        xbuf, x = _padded(rows, dim, t, gen)
        _, dfv = _dev(fbuf, dim)
        _, dxv = _dev(xbuf, dim)
        for n, k in ((1, 1), (2, 4), (4, 3)):
            fl = [planes[i] for i in range(4)]
            p = R.predict_f32(fl, n, k)                                    # the kernel's fp32 p, which the tests above pin
            for g_rows, g_dev, s_dev in ((gate[sel.long()], dgate, dsel), (gate[:1].expand(rows, -1), dgate[0], None)):
                ref = x.double() + p.double() * g_rows.double()
                got = ops.taylor_predict(dfv, n, k, dxv, g_dev, s_dev).cpu().double()
                bound = 2.0 ** -8 * ref.abs() if t == torch.bfloat16 else 2.0 ** -11 * ref.abs() + 2.0 ** -25
                worst = float(((got - ref).abs() / bound.clamp_min(1e-300)).max())
                print(f"{t} F={f} n={n} k={k}: worst |got - ref| / bound = {worst:.3f}")
                assert bool(((got - ref).abs() <= bound).all()), (f, n, k, worst)


@pytest.mark.parametrize("t", T_DTYPES, ids=["bf16", "fp16"])
def test_predict_of_one_plane_is_pab_broadcast_and_out_may_alias_x(gen, t):
    rows, dim = 300, 264
    table = torch.randn(2, 3, dim, generator=gen).to(DEV)
    sel = torch.randint(0, 2, (rows,), generator=gen, dtype=torch.int32).to(DEV)
    fbuf, _ = _padded(rows, dim, t, gen, planes=2)
    xbuf, _ = _padded(rows, dim, t, gen)
    _, dfv = _dev(fbuf, dim)
    for gate, s in ((table[:, 2], sel), (table[0, 2], None), (None, None)):
        _, dxv = _dev(xbuf, dim)
        want = ops.pab_broadcast(dxv, dfv[0], gate, s)
        assert torch.equal(ops.taylor_predict(dfv, 1, 3, dxv, gate, s), want)
        two = ops.taylor_predict(dfv, 2, 3, dxv, gate, s)
        assert ops.taylor_predict(dfv, 2, 3, dxv, gate, s, out=dxv) is dxv and torch.equal(dxv, two)     # in place


def test_argument_errors(gen):
    t = torch.bfloat16
    y = torch.zeros(4, 16, dtype=t, device=DEV)
    f = torch.zeros(3, 4, 16, dtype=t, device=DEV)
    for bad in (lambda: ops.taylor_update(y[:, ::2], f, 0, 1),
                lambda: ops.taylor_update(y, f[:, :3], 0, 1), lambda: ops.taylor_update(y, f.double(), 0, 1),
                lambda: ops.taylor_update(y, f[0], 0, 1), lambda: ops.taylor_update(y, f, 4, 1),
                lambda: ops.taylor_update(y, f, 1, 1, n_new=3), lambda: ops.taylor_update(y, f, 1, 0),
                lambda: ops.taylor_update(y, torch.zeros(5, 4, 16, dtype=t, device=DEV), 0, 1),
                lambda: ops.taylor_predict(f, 0, 1, dtype=t), lambda: ops.taylor_predict(f, 4, 1, dtype=t),
                lambda: ops.taylor_predict(f, 1, 1, y[:3]), lambda: ops.taylor_predict(f, 1, 1, out=y[:, :8]),
                lambda: ops.taylor_predict(f, 1, 1, gate=torch.zeros(16, device=DEV), dtype=t),
                lambda: ops.taylor_predict(f[0], 1, 1, dtype=t)):
        with pytest.raises(ValueError):
            bad()
    for bad in (lambda: ops.taylor_update(y.float(), f, 0, 1), lambda: ops.taylor_predict(f, 1, 1), lambda: ops.taylor_predict(f, 1, 1, dtype=torch.float32),
                lambda: ops.taylor_predict(f, 1, 1, y.half(), out=y)):
        with pytest.raises((TypeError, ValueError)):
            bad()
    with pytest.raises(RuntimeError, match="16-byte"):               # the library's own check: rows that are not 16-byte aligned
        ops.taylor_update(torch.zeros(4, 20, dtype=t, device=DEV)[:, 4:], f, 0, 1)
    with pytest.raises(RuntimeError, match="dim"):
        ops.taylor_predict(torch.zeros(2, 4, 12, dtype=t, device=DEV), 1, 1, dtype=t)


def test_kernel_timer_counts_the_bytes(gen):
    y = torch.zeros(16, 64, dtype=torch.bfloat16, device=DEV)
    f = torch.zeros(3, 16, 64, dtype=torch.float32, device=DEV)
    with ops.KernelTimer({"taylor_update", "taylor_predict"}) as kt:
        ops.taylor_update(y, f, 2, 1)                                # reads y + 2 planes, writes 3
        ops.taylor_predict(f, 3, 2, y, out=y)                        # reads 3 planes + x, writes x
    s = kt.summary()
    assert s["taylor_update"]["launches"] == s["taylor_predict"]["launches"] == 1
    assert kt.bytes["taylor_update"] == 16 * 64 * (2 + 5 * 4) and kt.bytes["taylor_predict"] == 16 * 64 * (3 * 4 + 2 * 2)
