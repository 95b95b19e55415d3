#!/usr/bin/env python3
"""What smooth K (fino_attn_fwd_fp8_smooth: the key mean subtracted before K becomes e4m3) costs.  One process, device events,
seeded N(0, 1) operands, warm-up, plain and smoothed calls alternated, the sequence run twice:

  1. ops.attention_fp8 at the Wan2.2-5B bench shape (B = 2, L = 12320, 24 x 128) and at CogVideoX config 5 (B = 2, L = 19126,
     48 x 64), k | v row-strided views of a fused QKV buffer as in the models, smooth_k off and on, and a device copy of K's bytes
     (strided K -> a contiguous buffer) as the yardstick: the mean pass reads K once and writes almost nothing, half of what that
     copy moves, so the added time per call should fit under one copy's time (margin: 2 x, for strided rows and two small launches);
  2. the full-size Wan2.2-5B step (bench.py's workload, eager) with MXFP8 linears + fp8 attention, smooth_k off and on:
     `steps` steps after `warmup`, as tools/mxfp6_step_bench.py; plus the in-run matrix peak (fino_diag_mfma_peak).
Usage: attn_fp8_smooth_bench.py [--out profiles/attn_fp8_smooth.txt] [--no-step] [--layers N]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402

SHAPES = [("wan2.2-5b self-attention", 2, 12320, 24, 128), ("cogvideox-5b config 5", 2, 19126, 48, 64)]
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def attention_part(a, dev):
    from frameino_amd import ops
    say("## ops.attention_fp8, smooth_k off / on, and a device copy of K's bytes (ms per call, device events)")
    for name, b, L, heads, dh in SHAPES:
        d = heads * dh
        g = torch.Generator(device=dev).manual_seed(1234)
        q = torch.randn(b, L, d, device=dev, generator=g).bfloat16()
        qkv = torch.randn(b, L, 3 * d, device=dev, generator=g).bfloat16()
        k, v = qkv[:, :, d:2 * d], qkv[:, :, 2 * d:]
        o, kc = torch.empty_like(q), torch.empty(b, L, d, device=dev, dtype=torch.bfloat16)
        runs = {"plain": lambda: ops.attention_fp8(q, k, v, heads, out=o, smooth_k=False),
                "smooth": lambda: ops.attention_fp8(q, k, v, heads, out=o, smooth_k=True),
                "copy": lambda: kc.copy_(k)}
        for fn in runs.values():
            timed(fn, a.attn_warmup)
        res = {n: [] for n in runs}
        for _ in range(a.reps):
            for n, fn in runs.items():
                res[n].append(timed(fn, a.attn_iters))
        kbytes = b * L * d * 2
        say(f"{name}: B = {b}, L = {L}, {heads} x {dh}, bf16; K = {kbytes / 1e6:.1f} MB (row stride {3 * d} elements)")
        for n in runs:
            say(f"  {n:6s} " + "  ".join(f"{t:8.4f}" for t in res[n]) + f"   min {min(res[n]):8.4f} ms")
        added, copy = min(res["smooth"]) - min(res["plain"]), min(res["copy"])
        say(f"  added by smooth K: {added:.4f} ms per call = {added / copy:.2f} x the copy of K's bytes ({copy:.4f} ms, "
            f"{2 * kbytes / copy / 1e9:.2f} TB/s read + written); K read once in that time = {kbytes / max(added, 1e-9) / 1e9:.2f} TB/s;  "
            f"threshold 2 x the copy: {'within' if added <= 2 * copy else 'EXCEEDED'}")
        del q, qkv, o, kc
    say()


def step_part(a, dev):
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
    say(f"## Wan2.2-5B step, MXFP8 linears + fp8 attention, smooth_k off / on: layers {cfg['num_layers']}, "
        f"L = {(fg + 1) * (lh // 2) * (lw // 2)} x 2 (CFG), {a.steps} steps after {a.warmup}, eager")
    res = {False: [], True: []}
    for r in range(a.reps):
        for smooth in (False, True):
            model.enable_fp8_attention(smooth_k=smooth)
            res[smooth].append(run())
            say(f"rep {r}: smooth_k {str(smooth):5s}  {res[smooth][-1]:8.2f} ms per step")
    for smooth in (False, True):
        say(f"smooth_k {str(smooth):5s}: min {min(res[smooth]):8.2f}  max {max(res[smooth]):8.2f} ms per step")
    say(f"added by smooth K: {min(res[True]) - min(res[False]):.2f} ms per step ({cfg['num_layers']} self-attention calls)")
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_fp8_smooth.txt"))
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--attn-iters", type=int, default=20)
    ap.add_argument("--attn-warmup", type=int, default=3)
    ap.add_argument("--layers", type=int, default=None, help="fewer layers (a quick look; not the step)")
    ap.add_argument("--no-step", action="store_true", help="the attention calls alone")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    say(f"# tools/attn_fp8_smooth_bench.py on {torch.cuda.get_device_name(0)}: synthetic N(0, 1) operands, one process")
    attention_part(a, dev)
    if not a.no_step:
        step_part(a, dev)
    peak = bench.measured_mfma_peak(dev, 0.0)
    say(f"matrix peak in this run (fino_diag_mfma_peak, bf16 32x32x16): {peak['power_capped_peak']} TFLOP/s")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
