"""Plain-torch restatement of the block-Hadamard rotation of `fino_quantize_mxfp6_rot` (include/frameino_hip.h).  No library
call: the tests compare the kernel against this file.

Every block of 32 consecutive K-elements, widened to fp32, is multiplied by the 32-point Walsh-Hadamard matrix H (symmetric,
H H = 32 I) by five in-place butterfly stages with strides 1, 2, 4, 8, 16 in that order -- fp32 adds and subtracts only, so
the kernel is bit-equal -- and the MXFP6 rule of tests/mxfp6_ref.py runs on the result.  Mode "weight" stores the block
exponent e - 5 (clamped at -127): the 1/32 of H H, so the product of the two decoded images is that of the unrotated operands."""
import torch

from tests import mxfp6_ref as R

MODES = ("act", "weight")


def rotate(x):
    """x [rows, cols] (cols % 32 == 0) -> fp32 [rows, cols], every 32-element block times H, by the butterflies of the rule"""
    rows, cols = x.shape
    v = x.detach().cpu().float().reshape(rows, cols // 32, 32).clone()
    s = 1
    while s < 32:
        lo = torch.tensor([i for i in range(32) if not i & s])
        a, b = v[..., lo], v[..., lo + s]
        v[..., lo], v[..., lo + s] = a + b, a - b
        s *= 2
    return v.reshape(rows, cols)


def quantize_ref(x, mode):
    """-> (codes uint8 [rows, cols], e int32 [rows, cols / 32]) as `fino_quantize_mxfp6_rot` stores them in `mode`"""
    assert mode in MODES
    codes, e = R.quantize_ref(rotate(x))
    if mode == "weight":
        e = (e - 5).clamp(min=-127)
    return codes, e


def decode(codes, e):
    return R.decode(codes, e)


GEMM_MNK = (300, 264, 384)


def gemm_operands(dtype, outliers=True, seed=21):
    """the tensors of the GEMM tests (CPU and GPU): A [300, 384] ~ N(0,1) with 12 random columns x 30 (the outlier channels the
    rotation is for), W [264, 384] ~ 0.02 N(0,1)"""
    m, n, k = GEMM_MNK
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(m, k, generator=g)
    w = 0.02 * torch.randn(n, k, generator=g)
    if outliers:
        a[:, torch.randperm(k, generator=g)[:12]] *= 30
    return a.to(dtype), w.to(dtype)


def rel_err(got, ref):
    """rel-RMS in float64"""
    got, ref = got.double(), ref.double()
    return float(((got - ref).pow(2).mean() / ref.pow(2).mean()).sqrt())


def restated_errors(a, w):
    """(unrotated, rotated) rel-RMS of the product of the restatement's decoded operands against the fp64 product of a, w"""
    ref = a.double() @ w.double().T
    plain = R.decode(*R.quantize_ref(a)).double() @ R.decode(*R.quantize_ref(w)).double().T
    rot = decode(*quantize_ref(a, "act")).double() @ decode(*quantize_ref(w, "weight")).double().T
    return rel_err(plain, ref), rel_err(rot, ref)
