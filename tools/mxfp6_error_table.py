#!/usr/bin/env python3
"""GEMM error of MXFP8 (e4m3) and MXFP6 (e2m3) operands, and of MXFP6 operands whose blocks were rotated by the Walsh-Hadamard
matrix (`ops.quantize_mxfp6(rotate="act" | "weight")`), quantised by the library's kernels on the GPU: rel-RMS of the fp64
matmul of the dequantised operands against the fp64 matmul of the unquantised ones, M = N = 128, for the operand
distributions a DiT linear sees.  --restated: the same table from the torch restatements of the rules (tests/mxfp6_ref.py,
tests/mxfp6_rot_ref.py) on the CPU, no library call; the codes are bit-equal, so the two tables agree.
Usage: mxfp6_error_table.py [--restated] > profiles/mxfp6_rot_error_table.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from tests import mxfp6_ref as R  # noqa: E402
from tests import mxfp6_rot_ref as RR  # noqa: E402

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
    yield "A Student-t, 3 dof", 3072, t3.sample((M, 3072)), n(M, 3072)
    yield "W Student-t, 3 dof", 3072, n(M, 3072), t3.sample((M, 3072))


def main():
    restated = "--restated" in sys.argv[1:]
    g = torch.Generator().manual_seed(0)
    if restated:
        print(f"# CPU: operands quantised by the torch restatements of the rules, M = N = {M}")
    else:
        from frameino_amd import ops
        from tests.test_mxfp8_gpu import dequant as dequant8
        print(f"# {torch.cuda.get_device_name(0)}: operands quantised by fino_quantize_mxfp8 / fino_quantize_mxfp6 / "
              f"fino_quantize_mxfp6_rot, M = N = {M}")
    print(f"{'operands (A; W N(0,1) unless said)':52s} {'K':>6s} {'e4m3':>8s} {'e2m3':>8s} {'ratio':>6s} {'e2m3 rot':>9s} {'ratio':>6s}")
    for name, k, a, w in cases(g):
        a, w = a.bfloat16(), w.bfloat16()
        ref = a.double() @ w.double().T

        def err(ad, wd):
            return float(((ad.double() @ wd.double().T - ref).pow(2).mean() / ref.pow(2).mean()).sqrt())

        if restated:
            d8 = [R.quantize_e4m3_ref(t) for t in (a, w)]
            d6 = [R.decode(*R.quantize_ref(t)) for t in (a, w)]
            d6r = [RR.decode(*RR.quantize_ref(t, mode)) for t, mode in ((a, "act"), (w, "weight"))]
        else:
            d8 = [dequant8(*ops.quantize_mxfp8(t.cuda()), M, k) for t in (a, w)]
            d6 = [R.decode(*R.unpack(*ops.quantize_mxfp6(t.cuda()), M, k)) for t in (a, w)]
            d6r = [R.decode(*R.unpack(*ops.quantize_mxfp6(t.cuda(), rotate=mode), M, k)) for t, mode in ((a, "act"), (w, "weight"))]
        r8, r6, r6r = err(*d8), err(*d6), err(*d6r)
        print(f"{name:52s} {k:6d} {r8:8.4f} {r6:8.4f} {r6 / r8:6.2f} {r6r:9.4f} {r6r / r8:6.2f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
