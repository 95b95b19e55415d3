#!/usr/bin/env python3
"""MXFP6 GEMM against the MXFP8 GEMM (the baseline) and the bf16 ping-pong GEMM at the four Wan block shapes, and the two
activation quantisers against a device copy of the same bytes.  One process, seeded N(0,1) operands (zero-filled operands
read high), device events, the precisions alternated inside every repetition and the whole sequence run twice so the spread
between repetitions is visible.  Usage: gemm_fp6_bench.py [L] > profiles/mxfp6_gemm.txt"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from frameino_amd import ops  # noqa: E402

L = int(sys.argv[1]) if len(sys.argv) > 1 else 24640
D, F = 3072, 14336
REPS, ITERS = 2, 20


def timeit(f, n=ITERS):
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        f()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e-3


def main():
    torch.manual_seed(0)
    dev = "cuda"
    print(f"# {torch.cuda.get_device_name(0)}  L = {L}  {ITERS} launches per figure, {REPS} repetitions")
    ok = True
    for (n, k, epi, nm) in [(3 * D, D, 0, "qkv"), (D, D, 3, "out+gate"), (F, D, 1, "ffn-up+gelu"), (D, F, 3, "ffn-down+gate")]:
        a = torch.randn(L, k, device=dev).bfloat16()
        w = (torch.randn(n, k, device=dev) * 0.02).bfloat16()
        b = torch.randn(n, device=dev).bfloat16()
        out = torch.empty(L, n, device=dev, dtype=torch.bfloat16)
        res = torch.randn(L, n, device=dev).bfloat16() if epi == 3 else None
        gate = torch.randn(2, n, device=dev) if epi == 3 else None
        sel = (torch.arange(L, device=dev) < 880).to(torch.int32) if epi == 3 else None
        a8, w8 = ops.quantize_mxfp8(a), ops.quantize_mxfp8(w)
        a6, w6 = ops.quantize_mxfp6(a), ops.quantize_mxfp6(w)
        fl = 2.0 * L * n * k
        t16, t8, t6 = [], [], []
        for _ in range(REPS):
            t16.append(timeit(lambda: ops.gemm(a, w, b, epi, res, gate, sel, out=out)))
            t8.append(timeit(lambda: ops.gemm_mxfp8(*a8, *w8, b, epi, res, gate, sel, out=out)))
            t6.append(timeit(lambda: ops.gemm_mxfp6(*a6, *w6, b, epi, res, gate, sel, out=out)))
        for r in range(REPS):
            print(f"{nm:14s} {L}x{n}x{k} rep {r}: bf16 {t16[r] * 1e6:7.1f} us {fl / t16[r] / 1e12:5.0f} TF | mxfp8 {t8[r] * 1e6:7.1f} us "
                  f"{fl / t8[r] / 1e12:5.0f} TF | mxfp6 {t6[r] * 1e6:7.1f} us {fl / t6[r] / 1e12:5.0f} TF ({t8[r] / t6[r]:.3f}x mxfp8)")
        spread8 = max(t8) - min(t8)
        gain = min(t8) - max(t6)
        print(f"{nm:14s} mxfp8 spread between repetitions {spread8 * 1e6:.1f} us; slowest mxfp6 is {gain * 1e6:+.1f} us under the "
              f"fastest mxfp8")
        if n == F or k == F:
            ok = ok and gain > spread8
        del a8, w8, a6, w6
    for k in (D, F):
        x = torch.randn(L, k, device=dev).bfloat16()
        o8, o6 = ops.quantize_mxfp8(x), ops.quantize_mxfp6(x)
        # a quantiser reads 2 B and writes 1 + 1/32 (e4m3) or 3/4 + 1/32 (e2m3) B per element; a copy of n bytes moves 2 n
        n8, n6 = int(L * k * (3 + 1 / 32) / 2), int(L * k * (2.75 + 1 / 32) / 2)
        src = torch.randint(0, 255, (n8,), dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        for r in range(REPS):
            tq8 = timeit(lambda: ops.quantize_mxfp8(x, out=o8))
            tc8 = timeit(lambda: dst.copy_(src))
            tq6 = timeit(lambda: ops.quantize_mxfp6(x, out=o6))
            tc6 = timeit(lambda: dst[:n6].copy_(src[:n6]))
            print(f"quantise [{L}, {k}] rep {r}: mxfp8 {tq8 * 1e6:6.1f} us ({2 * n8 / tq8 / 1e9:5.0f} GB/s)  copy of the same bytes "
                  f"{tc8 * 1e6:6.1f} us | mxfp6 {tq6 * 1e6:6.1f} us ({2 * n6 / tq6 / 1e9:5.0f} GB/s)  copy {tc6 * 1e6:6.1f} us")
    print("condition (mxfp6 faster than mxfp8 by more than the mxfp8 spread on both FFN shapes):", "MET" if ok else "NOT MET")
    return 0


if __name__ == "__main__":
    sys.exit(main())
