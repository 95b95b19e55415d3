#!/usr/bin/env python3
"""What smooth Q (fino_attn_fwd_fp8_smooth_q: each 256-row q-block's mean subtracted before q becomes e4m3, qbar . k added back to
the logits from a table) costs and buys.  One process, device events, seeded operands, warm-up, the variants alternated, the
sequence run `--reps` times, the minimum of the repetitions reported:

  calls  ops.attention_fp8 at the Wan2.2-5B bench shape (B = 2, L = 12320, 24 x 128) and at CogVideoX config 5 (B = 2, L = 19126,
         48 x 64), k | v row-strided views of a fused QKV buffer as in the models: smooth_q off, on, and the PRE-PASS ALONE (the
         three launches in front of the main one: tuning knob FINO_TUNE_ATTN_FP8_SQ_PREPASS = 1 stops the call behind them, so
         `prepass` = K / V quantiser + pre-pass and on - prepass = the main launch with smooth Q), plus the yardstick: a device
         copy of K's bytes (strided K -> a contiguous buffer) and of the table's bytes, timed in the same run.  The quantiser's own
         time, which `prepass` contains, is measured by the plain call at lq = 256;
  step   the full-size Wan2.2-5B step (bench.py's workload, eager) with MXFP8 linears + fp8 attention, smooth_q off / on (the
         CogVideoX-5B config-5 step: tools/cog_bench.py --mxfp8 --fp8-attention [--smooth-q]);
  error  rel-RMS against fp32 SDPA with q = N(0, 1) + c x N(0, 1) per (256-row block, head, channel), c in {0, 2, 8, 32}: the kernel
         next to the torch emulation (tests/attn_fp8_smooth_q_ref.py), plain and smoothed.  Synthetic operands: no quality claim.
Usage: attn_fp8_smooth_q_bench.py [calls] [step] [error] [--out profiles/attn_fp8_smooth_q.txt (appended)]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import bench  # noqa: E402
from attn_fp8_smooth_bench import SHAPES, timed  # noqa: E402

FINO_TUNE_ATTN_FP8_SQ_PREPASS = 7            # include/frameino_hip.h
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def calls_part(a, dev):
    from frameino_amd import _lib, ops
    lib = _lib.lib()
    say(f"## ops.attention_fp8, smooth_q off / on / pre-pass alone, and a device copy of K's + the table's bytes (ms per call, device "
        f"events, {a.attn_iters} calls per figure, {a.reps} repetitions, variants alternated)")
    for name, b, L, heads, dh in SHAPES:
        d = heads * dh
        g = torch.Generator(device=dev).manual_seed(1234)
        q = torch.randn(b, L, d, device=dev, generator=g).bfloat16()
        qkv = torch.randn(b, L, 3 * d, device=dev, generator=g).bfloat16()
        k, v = qkv[:, :, d:2 * d], qkv[:, :, 2 * d:]
        o, kc = torch.empty_like(q), torch.empty(b, L, d, device=dev, dtype=torch.bfloat16)
        words = b * heads * (-(-L // 256)) * (-(-L // 64)) * 64
        tab, tab2 = torch.zeros(words, dtype=torch.int32, device=dev), torch.empty(words, dtype=torch.int32, device=dev)

        def prepass_only():
            lib.fino_tune_set(FINO_TUNE_ATTN_FP8_SQ_PREPASS, 1)
            try:
                ops.attention_fp8(q, k, v, heads, out=o, smooth_q=True)
            finally:
                lib.fino_tune_set(FINO_TUNE_ATTN_FP8_SQ_PREPASS, 0)

        def copies():
            kc.copy_(k)
            tab2.copy_(tab)

        # `off` and `on` both contain the K / V quantiser; `prepass` = quantiser + pre-pass, so on - prepass = the SQ main launch
        runs = {"off": lambda: ops.attention_fp8(q, k, v, heads, out=o), "on": lambda: ops.attention_fp8(q, k, v, heads, out=o, smooth_q=True),
                "prepass": prepass_only, "copy": copies}
        for fn in runs.values():
            timed(fn, a.attn_warmup)
        res = {n: [] for n in runs}
        for _ in range(a.reps):
            for n, fn in runs.items():
                res[n].append(timed(fn, a.attn_iters))
        kbytes, tbytes = b * L * d * 2, words * 4
        say(f"{name}: B = {b}, L = {L}, {heads} x {dh}, bf16; K = {kbytes / 1e6:.1f} MB (row stride {3 * d} elements), table = "
            f"{tbytes / 1e6:.1f} MB (4 bytes per entry)")
        for n in runs:
            say(f"  {n:8s} " + "  ".join(f"{t:8.4f}" for t in res[n]) + f"   min {min(res[n]):8.4f} ms")
        off, on, pre, copy = (min(res[n]) for n in ("off", "on", "prepass", "copy"))
        added = on - off
        say(f"  added by smooth Q: {added:+.4f} ms per call ({on / off:.3f} x the call without it)")
        say(f"  `prepass` = K / V quantiser + the three pre-pass launches; the main launch (+ combine) with smooth Q = on - prepass = "
            f"{on - pre:.4f} ms")
        say(f"  copy of K's + the table's bytes: {copy:.4f} ms ({2 * (kbytes + tbytes) / copy / 1e9:.2f} TB/s read + written)")
        del q, qkv, o, kc, tab, tab2
    say()


def quant_part(a, dev):
    """the K / V quantiser alone is what `prepass` shares with `off`: lq = 1 leaves it (and a one-block main launch) of the plain call"""
    from frameino_amd import ops
    say("## the plain call at lq = 256 (the K / V quantiser + one q-block per head): what `prepass` above contains besides the pre-pass")
    for name, b, L, heads, dh in SHAPES:
        d = heads * dh
        g = torch.Generator(device=dev).manual_seed(1234)
        q = torch.randn(b, 256, d, device=dev, generator=g).bfloat16()
        qkv = torch.randn(b, L, 3 * d, device=dev, generator=g).bfloat16()
        k, v = qkv[:, :, d:2 * d], qkv[:, :, 2 * d:]
        o = torch.empty_like(q)
        fn = lambda: ops.attention_fp8(q, k, v, heads, out=o)       # noqa: E731
        timed(fn, a.attn_warmup)
        t = min(timed(fn, a.attn_iters) for _ in range(a.reps))
        say(f"{name}: {t:.4f} ms")
        del q, qkv, o
    say()


def wan_step_part(a, dev):
    from attn_fp8_smooth_v_bench import wan_step_part as step
    import attn_fp8_smooth_v_bench as vb
    vb.MODES = {"plain": dict(), "smooth_q": dict(smooth_q=True), "all three": dict(smooth_k=True, smooth_v=True, smooth_q=True)}
    vb.LINES = LINES
    step(a, dev, list(vb.MODES))


def error_part(a, dev):
    from frameino_amd import ops
    from tests.attn_fp8_smooth_q_ref import Q_BLOCK, emulated, sdpa
    from tests.parity import rel_rms
    b, heads, lq, lk = 2, 2, 300, 320
    say(f"## rel-RMS against fp32 SDPA; q = N(0, 1) + c x N(0, 1) per (256-row block, head, channel), k / v N(0, 1), B = {b}, {heads} "
        f"heads, Lq = {lq}, Lk = {lk}; emulation rounded to the storage dtype.  Synthetic operands: quality on real checkpoints is not "
        f"measured.")
    say(f"{'dtype':>5s} {'head_dim':>8s} {'P':>5s} {'c':>3s} | {'kernel plain':>12s} {'kernel smooth':>13s} | {'emul. plain':>11s} {'emul. smooth':>12s}")
    for dtype in (torch.bfloat16, torch.float16):
        for dh in (64, 128):
            d = heads * dh
            for p_mode in ("exp2", "ramp"):
                for c in (0, 2, 8, 32):
                    g = torch.Generator().manual_seed(100 * dh + c)
                    off = c * torch.randn(-(-lq // Q_BLOCK), d, generator=g)
                    q = (torch.randn(b, lq, d, generator=g) + off.repeat_interleave(Q_BLOCK, 0)[:lq]).to(dtype).to(dev)
                    k = torch.randn(b, lk, d, generator=g).to(dtype).to(dev)
                    v = torch.randn(b, lk, d, generator=g).to(dtype).to(dev)
                    ref = sdpa(q, k, v, heads)
                    kp, ks = (rel_rms(ops.attention_fp8(q, k, v, heads, p_mode=p_mode, smooth_q=s), ref) for s in (False, True))
                    ep, es = (rel_rms(emulated(q, k, v, heads, p_mode, smooth_q=s), ref) for s in (False, True))
                    say(f"{str(dtype)[6:10]:>5s} {dh:8d} {p_mode:>5s} {c:3d} | {kp:12.5f} {ks:13.5f} | {ep:11.5f} {es:12.5f}")
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parts", nargs="*", default=["calls", "step", "error"], choices=["calls", "step", "error"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_fp8_smooth_q.txt"), help="appended to")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--attn-iters", type=int, default=20)
    ap.add_argument("--attn-warmup", type=int, default=3)
    ap.add_argument("--layers", type=int, default=None, help="fewer layers (a quick look; not the step)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    say(f"# tools/attn_fp8_smooth_q_bench.py {' '.join(a.parts)} on {torch.cuda.get_device_name(0)}; measured once, on one box, in one run")
    if "calls" in a.parts:
        calls_part(a, dev)
        quant_part(a, dev)
    if "step" in a.parts:
        wan_step_part(a, dev)
    if "error" in a.parts:
        error_part(a, dev)
    if "step" in a.parts or "calls" in a.parts:
        peak = bench.measured_mfma_peak(dev, 0.0)
        say(f"matrix peak in this run (fino_diag_mfma_peak, bf16 32x32x16): {peak['power_capped_peak']} TFLOP/s")
        say()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(LINES) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
