#!/usr/bin/env python3
"""Sliding-window self-attention over frames, measured on one box in one run:

  1. the self-attention LAUNCH at the bench shape ([2, 12320, 24 x 128], 14 latent frames x 880 tokens, sinks = first frame +
     ID frame): the dense call as the model makes it (tail split included) against ops.attention_ranges at window_frames 1, 2, 3
     -- time ratio next to tile density; alternated, median of the rounds;
  2. the whole denoise STEP of the bench workload (random Wan2.2-5B weights, CFG batch, eager), dense against window_frames = 2,
     alternated;
  3. the same for the 81-frame workload (22 latent frames).

    python tools/window_attention_bench.py [--rounds 7] [--steps 3] [--skip-81f] [--out profiles/window_attention.txt]

Quality on real checkpoints is NOT measured here or anywhere in this repository (random weights only)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from frameino_amd import ops  # noqa: E402
from frameino_amd.window_attention import WindowAttentionConfig, frame_window_ranges, ranges_density  # noqa: E402


def launch_times(rounds, reps, frames=14, tpf=880, heads=24, dh=128, windows=(1, 2, 3)):
    L, d = frames * tpf, heads * dh
    g = torch.Generator(device="cuda").manual_seed(0)
    qkv = torch.randn(2, L, 3 * d, device="cuda", generator=g).bfloat16()          # the fused projection's layout
    q, k, v = qkv[:, :, :d], qkv[:, :, d:2 * d], qkv[:, :, 2 * d:]
    o = torch.empty(2, L, d, device="cuda", dtype=torch.bfloat16)
    runs, dens = {"dense": lambda: ops.attention(q, k, v, heads, out=o)}, {"dense": 1.0}
    for w in windows:
        tab = frame_window_ranges(frames, tpf, w, (0, -1))
        dens[f"window_frames={w}"] = ranges_density(tab, L)
        runs[f"window_frames={w}"] = (lambda t=tab.cuda(): ops.attention_ranges(q, k, v, heads, t, out=o))
    full = frame_window_ranges(frames, tpf, frames, (0, -1))
    dens["ranges, full table"] = ranges_density(full, L)                           # per-block fixed cost + the lost tail split
    runs["ranges, full table"] = (lambda t=full.cuda(): ops.attention_ranges(q, k, v, heads, t, out=o))
    t = {n: [] for n in runs}
    for f in runs.values():
        f(), f()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for n, f in runs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(reps):
                f()
            e.record()
            torch.cuda.synchronize()
            t[n].append(s.elapsed_time(e) / reps * 1e3)
    return {n: (statistics.median(t[n]), min(t[n]), max(t[n]), dens[n]) for n in runs}


def step_times(workload, rounds, steps, window):
    import bench
    from frameino_amd.pipeline_wan_i2v_motion_frameino import WanImageToVideoPipeline
    from frameino_amd.schedulers import FlowMatchEulerDiscreteScheduler
    from frameino_amd.configs import WAN22_5B_CFG
    cfg, dev = dict(WAN22_5B_CFG), torch.device("cuda")
    fg, lh, lw = bench.WORKLOADS[workload]
    C, nid = cfg["out_channels"], 1
    model = bench.build_model(cfg, dev)
    pipe = WanImageToVideoPipeline(scheduler=FlowMatchEulerDiscreteScheduler(shift=5.0), transformer=model, expand_timesteps=True)
    g = torch.Generator().manual_seed(1234)
    rnd = lambda *s: torch.randn(*s, generator=g)          # noqa: E731
    lat, cond, traj, idl = rnd(1, C, fg, lh, lw), rnd(1, C, 1, lh, lw), rnd(1, C, fg + nid, lh, lw), rnd(1, C, nid, lh, lw)
    traj[:, :, fg:] = 0
    mask = torch.ones(1, 1, fg, lh, lw)
    mask[:, :, 0] = 0
    pe, ne = rnd(1, 512, cfg["text_dim"]), rnd(1, 512, cfg["text_dim"])
    pe[:, 64:], ne[:, 8:] = 0, 0
    pipe.scheduler.set_timesteps(8, device=dev)
    st = pipe.make_state(lat.to(dev), cond.to(dev), traj.to(dev), idl.to(dev), mask.to(dev), pe.to(dev).bfloat16(),
                         ne.to(dev).bfloat16(), 5.0)
    ts, dts, lat0 = pipe.scheduler.timesteps.to(dev).float(), pipe.scheduler.dts.to(dev), st.lat.clone()
    wcfg = WindowAttentionConfig(window_frames=window, sink_frames=(0,))

    def run(windowed, n):
        model.disable_window_attention()
        if windowed:
            model.enable_window_attention(wcfg)
        st.lat.copy_(lat0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            for i in range(n):
                st.t_rows[1:2].copy_(ts[i:i + 1])
                st.dt.copy_(dts[i:i + 1])
                pipe._step(st)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    run(False, 1), run(True, 1)                                           # warm-up: every lazy cache of both paths
    t = {"dense": [], f"window_frames={window}": []}
    for _ in range(rounds):
        t["dense"].append(run(False, steps))
        t[f"window_frames={window}"].append(run(True, steps))
    frames, tpf = fg + nid, (lh // 2) * (lw // 2)
    dens = ranges_density(frame_window_ranges(frames, tpf, window, (0, -1)), frames * tpf)
    del model, pipe, st
    torch.cuda.empty_cache()
    return {n: (statistics.median(v), min(v), max(v)) for n, v in t.items()}, dens, frames, tpf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5, help="launches per timed window")
    ap.add_argument("--steps", type=int, default=3, help="denoise steps per timed window")
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--skip-81f", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("window_attention_bench: needs the GPU (no CPU path, nothing is estimated)")
    lines = [f"# tools/window_attention_bench.py on {torch.cuda.get_device_name(0)}; bf16; sinks = first frame + ID frame",
             "# quality on real checkpoints: NOT measured (random weights only)", ""]
    lt = launch_times(a.rounds, a.reps)
    base = lt["dense"][0]
    lines.append("self-attention launch, [2, 12320, 24 x 128] (14 frames x 880 tokens, 49 q-blocks x 193 key tiles)")
    lines.append(f"{'':28s} {'median us':>10s} {'min':>9s} {'max':>9s} {'ratio':>7s} {'density':>8s} {'(1+density)/2':>14s}")
    for n, (med, lo, hi, dens) in lt.items():
        lines.append(f"{n:28s} {med:10.1f} {lo:9.1f} {hi:9.1f} {med / base:7.3f} {dens:8.3f} {(1 + dens) / 2:14.3f}")
    if not a.skip_steps:
        for wl in ["wan2.2-5b-49f-704x1280"] + ([] if a.skip_81f else ["wan2.2-5b-81f-704x1280"]):
            stt, dens, frames, tpf = step_times(wl, a.step_rounds, a.steps, 2)
            base = stt["dense"][0]
            lines.append("")
            lines.append(f"denoise step, {wl} ({frames} latent frames x {tpf} tokens; eager, CFG batch; window density {dens:.3f})")
            lines.append(f"{'':28s} {'median ms':>10s} {'min':>9s} {'max':>9s} {'ratio':>7s}")
            for n, (med, lo, hi) in stt.items():
                lines.append(f"{n:28s} {med:10.1f} {lo:9.1f} {hi:9.1f} {med / base:7.3f}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
