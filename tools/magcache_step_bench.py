"""MagCache on the full-size Wan2.2-5B DiT (random weights, bf16, 49 frames 704x1280 + one ID frame: L = 12320), one process,
eager loop (the cache's loop), device-synchronised wall time per step after warm-up.  The variants ALTERNATE inside one run and
the whole round is repeated, so that the run's own spread is known:
  off        guidance on, no cache: the uncached step (batch-2 forward + sampler) -- the code path of the forward with the
             cache off, which is the forward as it was before MagCache
  compute    MagCache on, retention_ratio = 1: every step runs the stack, keeps its input and stores the residual
             bar: compute - off <= one residual launch's device time + the spread
  calibrate  MagCache in calibrate mode: every step runs the stack and the calibration launch (reported against `compute`)
  skip       MagCache on, ratios of 1.0, nothing retained, no skip limit within the run: step 0 computes, every later step
             skips the stack in BOTH contexts: embedding, one launch per context, output head, sampler
and: the bare launches at the bench shape [2 x 12320, 3072] bf16 (event-timed) -- fino_magcache_calibrate (three planes read,
one written) next to fino_step_cache_probe (three read, two written) and fino_step_cache_residual, each in bytes per second;
bar: the calibration launch's bytes per second within the run's spread of the probe's --, one 50-step `denoise` at the config
defaults on a SYNTHETIC curve against uncached (reported, no bar), and the box's in-run matrix peak.  RANDOM weights: a curve
calibrated on them says nothing about a real checkpoint, and nothing here says anything about quality, which is not measured.
Writes profiles/magcache_step.txt and prints one JSON line.

    python tools/magcache_step_bench.py [--steps 6] [--warmup 2] [--rounds 3] [--no-denoise] [--out profiles/magcache_step.txt]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from frameino_amd import ops                                               # noqa: E402
from frameino_amd.step_cache import MagCacheConfig                         # noqa: E402

ROWS, DIM = 2 * 12320, 3072


def synthetic_curve(n):
    """a made-up curve of the shape MagCache's paper shows: close to 1 for most of the run, falling towards the end"""
    return [1.0 - 0.03 * (i / max(n - 1, 1)) ** 2 for i in range(n)]


def kernel_times(dev, reps=20, rounds=3):
    """ms and GB/s of the three bare launches, alternated, `rounds` times: {name: [ms, ...]} and the byte counts"""
    g = torch.Generator(device=dev).manual_seed(3)
    mk = lambda: torch.randn(ROWS, DIM, generator=g, device=dev).bfloat16()           # noqa: E731
    x_out, x_in, r_prev = mk(), mk(), mk()
    r_new, copy = torch.empty_like(x_out), torch.empty_like(x_out)
    stats = torch.zeros(2, dtype=torch.float64, device=dev)
    plane = ROWS * DIM * 2

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / reps

    launches = {"calibrate": (lambda: ops.magcache_calibrate(x_out, x_in, r_prev, r_new, stats), 4 * plane),
                "probe": (lambda: ops.step_cache_probe(x_in, x_out, r_prev, r_new, copy), 5 * plane),
                "residual": (lambda: ops.step_cache_residual(x_out, x_in, out=r_new, subtract=True), 3 * plane)}
    ms = {k: [] for k in launches}
    for _ in range(rounds):
        for k, (fn, _) in launches.items():
            ms[k].append(timed(fn))
    return ms, {k: b for k, (_, b) in launches.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-denoise", action="store_true", help="skip the 50-step calls")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "magcache_step.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    from bench import measured_mfma_peak
    from frameino_amd.pipeline_wan_i2v_motion_frameino import WanImageToVideoPipeline
    from frameino_amd.random_init import random_wan_model
    from frameino_amd.schedulers import FlowMatchEulerDiscreteScheduler
    from oracle.wan_dit import WAN22_5B_CFG
    from tests.parity import model_cfg
    cfg = WAN22_5B_CFG
    m = random_wan_model(model_cfg(cfg), dev)
    pipe = WanImageToVideoPipeline(scheduler=FlowMatchEulerDiscreteScheduler(shift=5.0), transformer=m, expand_timesteps=True)
    C, fg, lh, lw = 48, 13, 44, 80
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
    pe, ne = pe.to(dev).bfloat16(), ne.to(dev).bfloat16()
    total = a.warmup + a.steps
    pipe.scheduler.set_timesteps(max(total, 2), device=dev)
    ts, dts = pipe.scheduler.timesteps.to(dev).float(), pipe.scheduler.dts.to(dev)

    configs = {"compute": lambda: MagCacheConfig(mag_ratios=[1.0] * total, num_inference_steps=total + 1, retention_ratio=1.0),
               "calibrate": lambda: MagCacheConfig(calibrate=True, num_inference_steps=total + 1),
               "skip": lambda: MagCacheConfig(mag_ratios=[1.0] * total, num_inference_steps=total + 1, retention_ratio=0.0,
                                              max_skip_steps=10 ** 6)}

    def per_step(variant):
        """ms per step of `steps` eager steps after `warmup` (state fresh at step 0, as in a call)"""
        if m.is_cache_enabled:
            m.disable_cache()
        if variant in configs:
            m.enable_cache(configs[variant]())
        st = pipe.make_state(lat, cond, traj, idl, mask, pe, ne, 5.0)
        with torch.no_grad():
            for i in range(total):
                if i == a.warmup:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                st.t_rows[1:2].copy_(ts[i:i + 1])
                st.dt.copy_(dts[i:i + 1])
                pipe._step(st)
            torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / a.steps
        log = list(m.cache_log) if m.is_cache_enabled else []
        if m.is_cache_enabled:
            m.disable_cache()
        if variant in ("compute", "calibrate"):
            assert all(e[2] for e in log) and len(log) == 2 * total
        if variant == "skip":
            assert [e[2] for e in log] == [True, True] + [False] * (2 * total - 2)
        return ms

    variants = ("off", "compute", "calibrate", "skip")
    times = {v: [] for v in variants}
    for _ in range(a.rounds):
        for v in variants:
            times[v].append(per_step(v))
    res = {"L": 12320, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "ms_per_step": times}
    kms, kbytes = kernel_times(dev, rounds=a.rounds)
    kmed = {k: sorted(t)[len(t) // 2] for k, t in kms.items()}
    gbps = {k: [kbytes[k] / t / 1e6 for t in kms[k]] for k in kms}
    gmed = {k: kbytes[k] / kmed[k] / 1e6 for k in kms}
    gspread = {k: max(v) - min(v) for k, v in gbps.items()}
    med = {v: sorted(t)[len(t) // 2] for v, t in times.items()}
    spread = {v: max(t) - min(t) for v, t in times.items()}
    res.update({"median_ms": med, "spread_ms": spread, "kernel_ms": kms, "kernel_median_ms": kmed, "kernel_GBps": gmed,
                "kernel_GBps_spread": gspread,
                "compute_minus_off_ms": med["compute"] - med["off"],
                "compute_bar_ms": kmed["residual"] + max(spread["compute"], spread["off"]),
                "calibrate_minus_compute_ms": med["calibrate"] - med["compute"],
                "calibrate_vs_probe_GBps": gmed["calibrate"] - gmed["probe"],
                "calibrate_vs_probe_bar_GBps": -max(gspread["calibrate"], gspread["probe"])})
    res["compute_bar_met"] = res["compute_minus_off_ms"] <= res["compute_bar_ms"]
    res["calibrate_bar_met"] = res["calibrate_vs_probe_GBps"] >= res["calibrate_vs_probe_bar_GBps"]
    lines = [f"MagCache, full-size Wan2.2-5B DiT, bf16, L = 12320, eager loop; {a.rounds} rounds of {a.steps} steps after {a.warmup} warm-up steps",
             f"bare launches at [{ROWS}, {DIM}] bf16, {a.rounds} alternated rounds of 20:"]
    for k in kms:
        lines.append(f"  {k:10s} " + " ".join(f"{t:7.4f}" for t in kms[k]) + f" ms   median {kmed[k]:.4f} ms = {gmed[k]:.0f} GB/s "
                     f"over {kbytes[k] / 2 ** 20:.0f} MiB (spread {gspread[k]:.0f} GB/s)")
    lines.append(f"  calibrate - probe   {res['calibrate_vs_probe_GBps']:+.0f} GB/s   bar (within the spread) "
                 f"{res['calibrate_vs_probe_bar_GBps']:.0f} GB/s   {'met' if res['calibrate_bar_met'] else 'MISSED'}")
    for v in variants:
        lines.append(f"{v:10s} " + " ".join(f"{t:8.2f}" for t in times[v]) + f"   median {med[v]:8.2f}  spread {spread[v]:.2f} ms/step")
    lines.append(f"compute - off         {res['compute_minus_off_ms']:+.2f} ms   bar (one residual launch + spread) "
                 f"{res['compute_bar_ms']:.2f} ms   {'met' if res['compute_bar_met'] else 'MISSED'}")
    lines.append(f"calibrate - compute   {res['calibrate_minus_compute_ms']:+.2f} ms   (two calibration launches in place of two "
                 f"residual launches: {2 * (kmed['calibrate'] - kmed['residual']):+.2f} ms of device time)")
    lines.append(f"skip / off            {med['skip'] / med['off']:.4f}   (a step that skips the stack in both contexts)")
    if not a.no_denoise:
        curve = synthetic_curve(50)
        for name, make in (("uncached", None), ("magcache", lambda: MagCacheConfig(mag_ratios=curve, num_inference_steps=50))):
            if make is not None:
                m.enable_cache(make())
            pipe.use_hip_graph = False
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pipe.denoise(lat, cond, traj, idl, mask, pe, ne, 5.0, 50)
            torch.cuda.synchronize()
            res[f"denoise50_{name}_s"] = time.perf_counter() - t0
            extra = ""
            if make is not None:
                log = list(m.cache_log)
                res["denoise50_magcache_skipped_forwards"] = sum(1 for e in log if not e[2])
                res["denoise50_magcache_forwards"] = len(log)
                extra = f"  ({res['denoise50_magcache_skipped_forwards']} of {len(log)} forwards skipped their stack)"
                m.disable_cache()
            lines.append(f"50-step denoise, {name}: {res[f'denoise50_{name}_s']:.2f} s{extra}")
        lines.append("the 50-step MagCache call runs at the config defaults (threshold 0.06, max_skip_steps 3, retention_ratio 0.2) on a "
                     "SYNTHETIC curve, mag_ratios[i] = 1 - 0.03 (i / 49)^2: no real checkpoint's curve is known here")
    lines.append("random weights: a curve calibrated on them says nothing about real checkpoints, and quality on real checkpoints "
                 "is not measured")
    res.update(measured_mfma_peak(dev, 0.0))
    res.pop("frac_of_power_capped_peak", None)
    lines.append(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
