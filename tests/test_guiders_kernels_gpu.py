"""The guider kernels (csrc/fino_guidance.hip) through the C ABI, bf16 and fp16.

`fino_guider_coefs`: {A, B} against `guiders.coefficients()` of the fp64 moments of the same T-typed inputs at rel 1e-6 -- fp32
storage is 6e-8, with a decade of room for the chain fp64 moments (another summation order) -> fp64 formulas -> fp32.  Inputs:
c ~ N(0.1, 1), u = 0.8 c + 0.6 z, so that no variance is ill-conditioned.  Layouts: the Wan strided frames with NaN in the ID
frame, one small and one of >= 3 partial blocks with a ragged last one; the CogVideoX rows with NaN behind n_lat at n_lat 1, 63,
4097; and, for the 16-byte-load path those odd sizes never take, one layout of each kind whose runs are multiples of 8 elements
over more than one block.  Two launches give the same bits; the degenerate inputs give the conventions of
tests/test_guiders_cpu.py.

`fino_guided_*_step`: each against the torch restatement of its plain sibling's test (tests/test_elementwise_edges_gpu.py) with
v formed as mul, mul, add in fp32 from the DEVICE's {A, B}: bit-identical, as those tests are."""
import math

import pytest
import torch

from frameino_amd.guiders import coefficients, kernel_args
from tests import guiders_ref as R
from tests.guiders_ref import CONFIGS, degenerate_cases
from tests.kernel_check import check_exact

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
G = 5.0


@pytest.fixture(scope="module")
def ops():
    from frameino_amd import ops as o
    return o


def _close(got, want, what):
    for name, x, y in zip("AB", got, want):
        assert math.isfinite(x), (what, name, x)
        assert abs(x - y) <= 1e-6 * abs(y), (what, name, x, y)


class _Bufs:
    def __init__(self, ops, n):
        self.ws = torch.empty(ops.guider_workspace_bytes(n), dtype=torch.uint8, device=DEV)
        self.ab = torch.full((2,), float("nan"), device=DEV)
        self.g = torch.tensor([G], device=DEV)
        self.zero = torch.zeros(1, device=DEV)


def _wan_case(c_, fg, nid, h, w, dtype, seed):
    """(pc, pu) [C, Fg + n_id, H, W] of T with NaN in the ID frames, and the sample (c, u) in fp64"""
    c, u = R.family(c_ * fg * h * w, seed, DEV)
    pc = torch.full((c_, fg + nid, h, w), float("nan"), dtype=dtype, device=DEV)
    pu = torch.full_like(pc, float("nan"))
    pc[:, :fg] = c.reshape(c_, fg, h, w).to(dtype)
    pu[:, :fg] = u.reshape(c_, fg, h, w).to(dtype)
    return pc, pu, pc[:, :fg].double(), pu[:, :fg].double()


def _check_all_guiders(launch, c64, u64, bufs, what):
    m, n = R.moments(c64, u64), c64.numel()
    for name, cfg in sorted(CONFIGS.items()):
        for step, flag in ((0, 1.0), (1, 0.0)):
            bufs.zero.fill_(flag)
            bufs.ab.fill_(float("nan"))
            launch(kernel_args(cfg), bufs)
            got = bufs.ab.tolist()
            want = coefficients(cfg, m, n, G, step)
            if want == (0.0, 0.0):
                assert got == [0.0, 0.0], (what, name, got)
            else:
                _close(got, want, (what, name, step))
            first = bufs.ab.clone()
            launch(kernel_args(cfg), bufs)
            assert torch.equal(first, bufs.ab), (what, name, "two launches differ")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(3, 2, 1, 5, 7), (16, 5, 1, 33, 31), (5, 3, 1, 8, 152)],
                         ids=["small", "three_blocks_ragged", "vector_loads"])
def test_coefs_wan_layout(ops, dtype, shape):
    c_, fg, nid, h, w = shape
    pc, pu, c64, u64 = _wan_case(c_, fg, nid, h, w, dtype, seed=11)
    n = c64.numel()
    per_block = 5 * 8                           # five fp64 moments per partial block
    if shape == (16, 5, 1, 33, 31):
        assert ops.guider_workspace_bytes(n) >= 3 * per_block                       # at least three partial blocks,
        assert ops.guider_workspace_bytes(n + 1) == ops.guider_workspace_bytes(n)   # and n is no multiple of the block
    if shape == (5, 3, 1, 8, 152):
        assert (fg * h * w) % 8 == 0 and ((fg + nid) * h * w) % 8 == 0 and ops.guider_workspace_bytes(n) == 2 * per_block
    bufs = _Bufs(ops, n)
    _check_all_guiders(lambda args, b: ops.guider_coefs(pc, pu, fg, args, b.g, b.zero, b.ws, b.ab), c64, u64, bufs, shape)
    # without a flag pointer the zero-init never applies
    cfg = CONFIGS["zero_star"]
    ops.guider_coefs(pc, pu, fg, kernel_args(cfg), bufs.g, None, bufs.ws, bufs.ab)
    _close(bufs.ab.tolist(), coefficients(cfg, R.moments(c64, u64), n, G, 1), (shape, "no flag"))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_lat,pad", [(1, 37), (63, 37), (4097, 37), (16392, 40), (16392, 37)],
                         ids=["1", "63", "4097", "vector_loads_two_blocks", "same_rows_misaligned"])
def test_coefs_cog_layout(ops, dtype, n_lat, pad):
    c, u = R.family(n_lat, 12, DEV)
    pred = torch.full((2, n_lat + pad), float("nan"), dtype=dtype, device=DEV)      # batch_stride = n_lat + pad, NaN behind
    pred[0, :n_lat], pred[1, :n_lat] = u.to(dtype), c.to(dtype)
    bufs = _Bufs(ops, n_lat)
    _check_all_guiders(lambda args, b: ops.guider_coefs_rows(pred, n_lat, args, b.g, b.zero, b.ws, b.ab),
                       pred[1, :n_lat].double(), pred[0, :n_lat].double(), bufs, (n_lat, pad))


@pytest.mark.parametrize("dtype", DTYPES)
def test_coefs_degenerate_inputs(ops, dtype):
    """u = 0, c = 0, c == u, constants, n = 1: finite, and the conventions `coefficients()` states (held to their exact values
    by tests/test_guiders_cpu.py)"""
    for case, (c, u) in degenerate_cases().items():
        n = c.numel()
        pred = torch.stack([u, c]).to(dtype).to(DEV).contiguous()
        bufs = _Bufs(ops, n)
        m = R.moments(pred[1].double(), pred[0].double())
        for name, cfg in sorted(CONFIGS.items()):
            ops.guider_coefs_rows(pred, n, kernel_args(cfg), bufs.g, bufs.zero, bufs.ws, bufs.ab)
            got, want = bufs.ab.tolist(), coefficients(cfg, m, n, G, 1)
            for x, y in zip(got, want):
                assert math.isfinite(x) and abs(x - y) <= 1e-6 * abs(y), (case, name, got, want)
            if case in ("constants", "n=1") and cfg.guidance_rescale > 0:       # f = 1: the rescale changes nothing
                plain = type(cfg)(**{**cfg.__dict__, "guidance_rescale": 0.0})
                ops.guider_coefs_rows(pred, n, kernel_args(plain), bufs.g, bufs.zero, bufs.ws, bufs.ab)
                assert bufs.ab.tolist() == got, (case, name)


def test_coefs_refuses_a_short_workspace_and_bad_arguments(ops):
    pred = torch.zeros(2, 40000, dtype=torch.bfloat16, device=DEV)
    bufs = _Bufs(ops, 40000)
    with pytest.raises(RuntimeError, match="workspace of 80 bytes, need 120"):
        ops.guider_coefs_rows(pred, 40000, (0, 0.0, 1.0, 0.5), bufs.g, None, bufs.ws[:80], bufs.ab)
    with pytest.raises(RuntimeError, match="kind 3"):
        ops.guider_coefs_rows(pred, 40000, (3, 0.0, 1.0, 0.5), bufs.g, None, bufs.ws, bufs.ab)
    with pytest.raises(RuntimeError, match="guidance_rescale=1.5"):
        ops.guider_coefs_rows(pred, 40000, (0, 0.0, 1.0, 1.5), bufs.g, None, bufs.ws, bufs.ab)


# ------------------------------------------------------------------------------------------------------- the guided steps
def rnd(*shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


def _device_ab(ops, pc, pu, fg, name, zero):
    """{A, B} as the device computed them for this pair of predictions"""
    bufs = _Bufs(ops, pc[:, :fg].numel())
    bufs.zero.fill_(1.0 if zero else 0.0)
    ops.guider_coefs(pc, pu, fg, kernel_args(CONFIGS[name]), bufs.g, bufs.zero, bufs.ws, bufs.ab)
    assert bool(torch.isfinite(bufs.ab).all())
    return bufs.ab


AB_CASES = [("apg+rescale", False), ("zero_star", False), ("zero_star", True)]
AB_IDS = ["apg+rescale", "zero_star", "zero_init"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,zero", AB_CASES, ids=AB_IDS)
def test_guided_euler_step(ops, dtype, name, zero):
    c, fg, ft, h, w = 4, 3, 4, 5, 6
    lat = rnd(c, fg, h, w, dtype=torch.float32, seed=70)
    pc, pu = rnd(c, ft, h, w, dtype=dtype, seed=71), rnd(c, ft, h, w, dtype=dtype, seed=72)
    dt = torch.tensor([-0.037], device=DEV)
    ab = _device_ab(ops, pc, pu, fg, name, zero)
    v = (ab[0] * pc[:, :fg].float() + ab[1] * pu[:, :fg].float()).to(dtype)          # mul, mul, add in fp32, then T
    for round_out in (True, False):
        l2 = lat.clone()
        ops.guided_euler_step_(l2, pc, pu, ab, dt, round_out=round_out)
        want = lat + dt * v.float()
        check_exact(l2, want.to(dtype).float() if round_out else want)
        if zero and not round_out:
            assert ab.tolist() == [0.0, 0.0] and torch.equal(l2, lat)               # A = B = 0: lat bit-unchanged


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,zero", AB_CASES, ids=AB_IDS)
def test_guided_unipc_step(ops, dtype, name, zero):
    c, fg, ft, h, w = 4, 3, 4, 5, 6
    pc, pu = rnd(c, ft, h, w, dtype=dtype, seed=100), rnd(c, ft, h, w, dtype=dtype, seed=101)
    x, last, m0, m1 = (rnd(c, fg, h, w, dtype=torch.float32, seed=102 + i) for i in range(4))
    ab = _device_ab(ops, pc, pu, fg, name, zero)
    for use_corr in (0.0, 1.0):
        k = torch.tensor([123.0, 0.83, use_corr, 0.9, 0.31, -0.07, 0.12, 0.8, 0.25, -0.05], device=DEV)   # k[0] (g) is not read
        v = (ab[0] * pc[:, :fg].float() + ab[1] * pu[:, :fg].float()).to(dtype).float()
        mt = x - (v.to(dtype) * k[1].item()).float()
        xc = k[3] * last + k[4] * m0 + k[5] * m1 + k[6] * mt if use_corr else x
        xn = k[7] * xc + k[8] * mt + k[9] * m0
        bx, bl, b0, b1 = (t.clone() for t in (x, last, m0, m1))
        ops.guided_unipc_step_(bx, bl, b0, b1, pc, pu, k, ab)
        check_exact(bx, xn)
        check_exact(bl, xc)
        check_exact(b0, mt)
        check_exact(b1, m0)
        if zero:
            assert torch.equal(b0, x)                                               # A = B = 0: the step records m_t = x


def _cog_ab(ops, pred, n_lat, name, zero):
    bufs = _Bufs(ops, n_lat)
    bufs.zero.fill_(1.0 if zero else 0.0)
    ops.guider_coefs_rows(pred, n_lat, kernel_args(CONFIGS[name]), bufs.g, bufs.zero, bufs.ws, bufs.ab)
    return bufs.ab


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,zero", AB_CASES, ids=AB_IDS)
def test_guided_vpred_step(ops, dtype, name, zero):
    f, ft, c, h, w = 3, 4, 2, 5, 6
    lat = rnd(f, c, h, w, dtype=dtype, seed=80, scale=2.0)
    pred = rnd(2, ft, c, h, w, dtype=dtype, seed=81)
    coef = torch.tensor([0.83, 0.55, 0.91, 0.12, 123.0], device=DEV)                # coef[4] (g) is not read
    ab = _cog_ab(ops, pred, lat.numel(), name, zero)
    l2 = lat.clone()
    ops.guided_vpred_step_(l2, pred, coef, ab)
    p = pred.float()[:, :f]
    v = ab[0] * p[1] + ab[1] * p[0]
    x = lat.float()
    x0 = (coef[0] * x).to(dtype).float() - coef[1] * v
    check_exact(l2, ((coef[2] * x).to(dtype).float() + coef[3] * x0).to(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,zero", AB_CASES, ids=AB_IDS)
@pytest.mark.parametrize("use_old", [0.0, 1.0])
def test_guided_dpm_step(ops, dtype, name, zero, use_old):
    f, ft, c, h, w = 3, 4, 2, 5, 6
    lat = rnd(f, c, h, w, dtype=dtype, seed=90, scale=2.0)
    pred = rnd(2, ft, c, h, w, dtype=dtype, seed=91)
    noise = rnd(f, c, h, w, dtype=dtype, seed=92)
    x0_old = rnd(f, c, h, w, dtype=torch.float32, seed=93)
    coef = torch.tensor([0.83, 0.55, 0.97, 0.31, 1.7, 0.6, 0.05, 123.0, use_old], device=DEV)   # coef[7] (g) is not read
    ab = _cog_ab(ops, pred, lat.numel(), name, zero)
    l2, o2 = lat.clone(), x0_old.clone()
    ops.guided_dpm_step_(l2, pred, o2, noise, coef, ab)
    p = pred.float()[:, :f]
    v = ab[0] * p[1] + ab[1] * p[0]
    x = lat.float()
    x0 = (coef[0] * x).to(dtype).float() - coef[1] * v
    d = coef[4] * x0 - coef[5] * x0_old if use_old else x0
    nz = (coef[6] * noise.float()).to(dtype).float()
    check_exact(l2, ((coef[2] * x).to(dtype).float() - coef[3] * d + nz).to(dtype))
    check_exact(o2, x0)
