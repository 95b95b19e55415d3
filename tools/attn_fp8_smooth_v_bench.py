#!/usr/bin/env python3
"""What smooth V (fino_attn_fwd_fp8_smoothed: the value mean subtracted before V becomes e4m3, added back to the output) costs and
buys.  One process, device events, seeded operands, warm-up, the modes alternated, the sequence run `--reps` times:

  calls  ops.attention_fp8 at the Wan2.2-5B bench shape (B = 2, L = 12320, 24 x 128) and at CogVideoX config 5 (B = 2, L = 19126,
         48 x 64), k | v row-strided views of a fused QKV buffer as in the models, in four modes: plain, smooth_k, smooth_v, both
         -- the whole launch sequence (mean passes, quantiser, main kernel, combine);
  step   the full-size Wan2.2-5B step (bench.py's workload, eager) with MXFP8 linears + fp8 attention in the four modes (the
         CogVideoX-5B config-5 step: tools/cog_bench.py --mxfp8 --fp8-attention [--smooth-k] [--smooth-v]);
  error  rel-RMS against fp32 SDPA with V = N(0, 1) + c x N(0, 1) per (batch element, channel), c in {0, 2, 8, 32}: the kernel and
         the torch emulation (tests/attn_fp8_smooth_v_ref.py, rounded to bf16 like the kernel's output), plain and smoothed.
Times of the parent commit come from ITS tree and tools/attn_fp8_smooth_bench.py (plain and smooth_k) in the same session.  For the
main kernel ALONE run `calls --modes plain` and `calls --modes smooth_v` under a kernel tracer, one process each: the kernel's name
is the same in both (the mu epilogue is a run-time branch on a pointer).
Usage: attn_fp8_smooth_v_bench.py [calls] [step] [error] [--out FILE (appended)] [--modes plain,smooth_k,smooth_v,both]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import bench  # noqa: E402
from attn_fp8_smooth_bench import SHAPES, timed  # noqa: E402

MODES = {"plain": dict(), "smooth_k": dict(smooth_k=True), "smooth_v": dict(smooth_v=True), "both": dict(smooth_k=True, smooth_v=True)}
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def calls_part(a, dev, modes):
    from frameino_amd import ops
    say(f"## ops.attention_fp8, whole launch sequence, modes {', '.join(modes)} (ms per call, device events, {a.attn_iters} calls per "
        f"figure, {a.reps} repetitions, modes alternated)")
    for name, b, L, heads, dh in SHAPES:
        d = heads * dh
        g = torch.Generator(device=dev).manual_seed(1234)
        q = torch.randn(b, L, d, device=dev, generator=g).bfloat16()
        qkv = torch.randn(b, L, 3 * d, device=dev, generator=g).bfloat16()
        k, v = qkv[:, :, d:2 * d], qkv[:, :, 2 * d:]
        o = torch.empty_like(q)
        runs = {n: (lambda kw=MODES[n]: ops.attention_fp8(q, k, v, heads, out=o, **kw)) for n in modes}
        for fn in runs.values():
            timed(fn, a.attn_warmup)
        res = {n: [] for n in runs}
        for _ in range(a.reps):
            for n, fn in runs.items():
                res[n].append(timed(fn, a.attn_iters))
        say(f"{name}: B = {b}, L = {L}, {heads} x {dh}, bf16 (row stride {3 * d} elements)")
        for n in runs:
            say(f"  {n:8s} " + "  ".join(f"{t:8.4f}" for t in res[n]) + f"   min {min(res[n]):8.4f}  max {max(res[n]):8.4f} ms"
                + (f"   min - plain min {min(res[n]) - min(res['plain']):+.4f}" if n != "plain" and "plain" in res else ""))
        del q, qkv, o
    say()


def _steps(a, run, enable, modes, what):
    res = {n: [] for n in modes}
    for r in range(a.reps):
        for n in modes:
            enable(**MODES[n])
            res[n].append(run())
            say(f"rep {r}: {n:8s} {res[n][-1]:8.2f} ms per step")
    for n in modes:
        say(f"{what} {n:8s}: min {min(res[n]):8.2f}  max {max(res[n]):8.2f} ms per step"
            + (f"   min - plain min {min(res[n]) - min(res['plain']):+.2f}" if n != "plain" and "plain" in res else ""))
    say()


def wan_step_part(a, dev, modes):
    from frameino_amd.configs import WAN22_5B_CFG
    from frameino_amd.pipeline_wan_i2v_motion_frameino import WanImageToVideoPipeline
    from frameino_amd.schedulers import FlowMatchEulerDiscreteScheduler
    cfg = dict(WAN22_5B_CFG)
    if a.layers:
        cfg["num_layers"] = a.layers
    fg, lh, lw = bench.WORKLOADS["wan2.2-5b-49f-704x1280"]
    C = cfg["out_channels"]
    model = bench.build_model(cfg, dev)
    pipe = WanImageToVideoPipeline(scheduler=FlowMatchEulerDiscreteScheduler(shift=5.0), transformer=model, expand_timesteps=True)
    pipe.use_hip_graph = False
    g = torch.Generator().manual_seed(1234)
    lat = torch.randn(1, C, fg, lh, lw, generator=g).to(dev)
    cond = torch.randn(1, C, 1, lh, lw, generator=g).to(dev)
    traj = torch.randn(1, C, fg + 1, lh, lw, generator=g).to(dev)
    traj[:, :, fg:] = 0
    idl = torch.randn(1, C, 1, lh, lw, generator=g).to(dev)
    mask = torch.ones(1, 1, fg, lh, lw, device=dev)
    mask[:, :, 0] = 0
    pe = torch.randn(1, 512, cfg["text_dim"], generator=g)
    pe[:, 64:] = 0
    ne = torch.randn(1, 512, cfg["text_dim"], generator=g)
    ne[:, 8:] = 0
    total = a.warmup + a.steps
    pipe.scheduler.set_timesteps(max(total, 2), device=dev)
    st = pipe.make_state(lat, cond, traj, idl, mask, pe.to(dev).bfloat16(), ne.to(dev).bfloat16(), 5.0)
    ts, dts = pipe.scheduler.timesteps.to(dev).float(), pipe.scheduler.dts.to(dev)
    lat0 = st.lat.clone()

    def run():
        st.lat.copy_(lat0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.no_grad():
            for i in range(total):
                if i == a.warmup:
                    e0.record()
                j = min(i, ts.numel() - 1)
                st.t_rows[1:2].copy_(ts[j:j + 1])
                st.dt.copy_(dts[j:j + 1])
                pipe._step(st)
            e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps

    model.enable_mxfp8_linears()
    say(f"## Wan2.2-5B step, MXFP8 linears + fp8 attention: layers {cfg['num_layers']}, L = {(fg + 1) * (lh // 2) * (lw // 2)} x 2 (CFG), "
        f"{a.steps} steps after {a.warmup}, eager")
    _steps(a, run, lambda **kw: model.enable_fp8_attention(**kw), modes, "wan")


def error_part(a, dev):
    from frameino_amd import ops
    from tests.attn_fp8_smooth_v_ref import emulated, sdpa
    from tests.parity import rel_rms
    b, heads, lq, lk = 2, 2, 256, 320
    say(f"## rel-RMS against fp32 SDPA; V = N(0, 1) + c x N(0, 1) per (batch element, channel), q / k N(0, 1), B = {b}, {heads} heads, "
        f"Lq = {lq}, Lk = {lk}; emulation rounded to the storage dtype.  Synthetic operands: quality on real checkpoints is not measured.")
    say(f"{'dtype':>5s} {'head_dim':>8s} {'P':>5s} {'c':>3s} | {'kernel plain':>12s} {'kernel smooth':>13s} | {'emul. plain':>11s} {'emul. smooth':>12s}")
    for dtype in (torch.bfloat16, torch.float16):
        for dh in (64, 128):
            d = heads * dh
            for p_mode in ("exp2", "ramp"):
                for c in (0, 2, 8, 32):
                    g = torch.Generator().manual_seed(100 * dh + c)
                    q = torch.randn(b, lq, d, generator=g).to(dtype).to(dev)
                    k = torch.randn(b, lk, d, generator=g).to(dtype).to(dev)
                    v = (torch.randn(b, lk, d, generator=g) + c * torch.randn(b, 1, d, generator=g)).to(dtype).to(dev)
                    ref = sdpa(q, k, v, heads)
                    kp, ks = (rel_rms(ops.attention_fp8(q, k, v, heads, p_mode=p_mode, smooth_v=s), ref) for s in (False, True))
                    ep, es = (rel_rms(emulated(q, k, v, heads, p_mode, smooth_v=s), ref) for s in (False, True))
                    say(f"{str(dtype)[6:10]:>5s} {dh:8d} {p_mode:>5s} {c:3d} | {kp:12.5f} {ks:13.5f} | {ep:11.5f} {es:12.5f}")
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parts", nargs="*", default=["calls", "step", "error"], choices=["calls", "step", "error"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_v.txt"), help="appended to")
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--attn-iters", type=int, default=20)
    ap.add_argument("--attn-warmup", type=int, default=3)
    ap.add_argument("--layers", type=int, default=None, help="fewer layers (a quick look; not the step)")
    a = ap.parse_args()
    modes = [m for m in a.modes.split(",") if m]
    assert all(m in MODES for m in modes), modes
    dev = torch.device("cuda", 0)
    from frameino_amd import _lib
    say(f"# tools/attn_fp8_smooth_v_bench.py {' '.join(a.parts)} on {torch.cuda.get_device_name(0)}, library: {a.label} "
        f"({os.path.basename(_lib.LIB_PATH)}); measured once, on one box, in one run")
    if "calls" in a.parts:
        calls_part(a, dev, modes)
    if "step" in a.parts:
        wan_step_part(a, dev, modes)
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
