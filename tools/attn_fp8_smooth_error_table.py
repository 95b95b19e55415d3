#!/usr/bin/env python3
"""The error of the fp8 attention against fp32 SDPA when K carries a per-channel offset shared by all keys, with and without smooth
K (fino_attn_fwd_fp8_smooth): K = N(0, 1) + c x N(0, 1) per (head, channel), q and v N(0, 1), 2 heads, Lq = 256, Lk = 320, bf16,
c in {0, 2, 8, 32}, head_dim 64 / 128, both P modes.  Columns: the kernel plain / smoothed and the torch emulation of the same
quantisation (tests/attn_fp8_ref.py) plain / smoothed; rel-RMS.  SYNTHETIC operands: quality on real checkpoints is not measured.
Usage: attn_fp8_smooth_error_table.py [--out profiles/attn_fp8_smooth_error.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from tests.attn_fp8_ref import emulated, sdpa  # noqa: E402
from tests.parity import rel_rms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_fp8_smooth_error.txt"))
    a = ap.parse_args()
    from frameino_amd import ops
    dev = torch.device("cuda", 0)
    b, heads, lq, lk = 1, 2, 256, 320
    lines = [f"# tools/attn_fp8_smooth_error_table.py on {torch.cuda.get_device_name(0)}: rel-RMS against fp32 SDPA; K = N(0, 1) + c x N(0, 1) "
             f"per (head, channel), q / v N(0, 1), {heads} heads, Lq = {lq}, Lk = {lk}, bf16.  Synthetic operands: quality on real "
             "checkpoints is not measured.",
             f"{'head_dim':>8s} {'P':>5s} {'c':>3s} | {'kernel plain':>12s} {'kernel smooth':>13s} | {'emul. plain':>11s} {'emul. smooth':>12s}"]
    for dh in (64, 128):
        d = heads * dh
        for p_mode in ("exp2", "ramp"):
            for c in (0, 2, 8, 32):
                g = torch.Generator().manual_seed(100 * dh + c)
                q = torch.randn(b, lq, d, generator=g).bfloat16().to(dev)
                k = (torch.randn(b, lk, d, generator=g) + c * torch.randn(d, generator=g)).bfloat16().to(dev)
                v = torch.randn(b, lk, d, generator=g).bfloat16().to(dev)
                ref = sdpa(q, k, v, heads)
                kp, ks = (rel_rms(ops.attention_fp8(q, k, v, heads, p_mode=p_mode, smooth_k=s), ref) for s in (False, True))
                ep, es = (rel_rms(emulated(q, k, v, heads, p_mode, smooth_k=s), ref) for s in (False, True))
                lines.append(f"{dh:8d} {p_mode:>5s} {c:3d} | {kp:12.4f} {ks:13.4f} | {ep:11.4f} {es:12.4f}")
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
