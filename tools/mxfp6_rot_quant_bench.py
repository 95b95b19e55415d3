#!/usr/bin/env python3
"""The MXFP6 activation quantiser with and without the block-Hadamard rotation (`fino_quantize_mxfp6` against
`fino_quantize_mxfp6_rot`, both modes) at the two activation shapes of the Wan step, bf16, seeded N(0,1) input: one process,
device events, the three launches alternated inside every round, medians over the rounds.
Usage: mxfp6_rot_quant_bench.py [L] [--rounds 9] > profiles/mxfp6_rot_quant.txt"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from frameino_amd import ops  # noqa: E402


def timeit(f, n):
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        f()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3            # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("rows", type=int, nargs="?", default=24640)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    torch.manual_seed(0)
    print(f"# {torch.cuda.get_device_name(0)}  rows = {a.rows}  bf16  {a.iters} launches per figure, {a.rounds} rounds, alternated")
    for k in (3072, 14336):
        x = torch.randn(a.rows, k, device="cuda").bfloat16()
        out = ops.quantize_mxfp6(x)
        variants = {"plain": None, "rot act": "act", "rot weight": "weight"}
        t = {name: [] for name in variants}
        for _ in range(a.rounds):
            for name, rot in variants.items():
                kw = {} if rot is None else {"rotate": rot}
                t[name].append(timeit(lambda: ops.quantize_mxfp6(x, out=out, **kw), a.iters))
        nbytes = a.rows * k * (2 + 0.75 + 1 / 32)                     # read bf16, write e2m3 + one scale byte per 32
        med = {name: statistics.median(v) for name, v in t.items()}
        for name, v in t.items():
            print(f"quantise [{a.rows}, {k}] {name:10s}: median {med[name]:7.1f} us  min {min(v):7.1f}  max {max(v):7.1f}  "
                  f"({nbytes / med[name] / 1e3:5.0f} GB/s)  {med[name] / med['plain']:.3f} x plain")
    return 0


if __name__ == "__main__":
    sys.exit(main())
