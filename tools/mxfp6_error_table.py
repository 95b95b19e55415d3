#!/usr/bin/env python3
"""GEMM error of MXFP8 (e4m3) and MXFP6 (e2m3) operands, quantised by the library's kernels on the GPU: rel-RMS of the fp64
matmul of the dequantised operands against the fp64 matmul of the unquantised ones, M = N = 128, for the operand
distributions a DiT linear sees.  Usage: mxfp6_error_table.py > profiles/mxfp6_error_table.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from frameino_amd import ops  # noqa: E402
from tests import mxfp6_ref as R  # noqa: E402
from tests.test_mxfp8_gpu import dequant as dequant8  # noqa: E402

M = 128


def cases(g):
    n = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    t3 = torch.distributions.StudentT(3.0)
    yield "N(0,1)", 3072, n(M, 3072), n(M, 3072)
    yield "N(0,1)", 14336, n(M, 14336), n(M, 14336)
    torch.manual_seed(3)
    yield "Student-t, 3 dof", 3072, t3.sample((M, 3072)), t3.sample((M, 3072))
    a = n(M, 3072)
    a[:, ::97] *= 30
    yield "N(0,1), every 97th A column x 30", 3072, a, n(M, 3072)
    yield "A = GELU(N(0,1)), W N(0,1)", 14336, torch.nn.functional.gelu(n(M, 14336), approximate="tanh"), n(M, 14336)
    yield "A = N(0,1) (1 + N(0,0.3)) + N(0,0.3) per channel", 3072, n(M, 3072) * (1 + 0.3 * n(1, 3072)) + 0.3 * n(1, 3072), n(M, 3072)
    yield "A = N(0,1) x log-normal(sigma = 1) per channel", 3072, n(M, 3072) * torch.exp(n(1, 3072)), n(M, 3072)


def main():
    g = torch.Generator().manual_seed(0)
    print(f"# {torch.cuda.get_device_name(0)}: operands quantised by fino_quantize_mxfp8 / fino_quantize_mxfp6, M = N = {M}")
    print(f"{'operands (A; W N(0,1) unless said)':52s} {'K':>6s} {'e4m3':>8s} {'e2m3':>8s} {'ratio':>6s}")
    for name, k, a, w in cases(g):
        a, w = a.bfloat16(), w.bfloat16()
        ref = a.double() @ w.double().T

        def err(ad, wd):
            return float(((ad.double() @ wd.double().T - ref).pow(2).mean() / ref.pow(2).mean()).sqrt())

        d8 = [dequant8(*ops.quantize_mxfp8(t.cuda()), M, k) for t in (a, w)]
        d6 = [R.decode(*R.unpack(*ops.quantize_mxfp6(t.cuda()), M, k)) for t in (a, w)]
        r8, r6 = err(*d8), err(*d6)
        print(f"{name:52s} {k:6d} {r8:8.4f} {r6:8.4f} {r6 / r8:6.2f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
