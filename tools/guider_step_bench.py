"""What a guider (frameino_amd/guiders.py) adds to a sampler step, on the bench workload: the full-size Wan2.2-5B DiT (random
weights, bf16, 49 frames 704x1280 + one ID frame: L = 12320, latents [48, 13, 44, 80] = 2.2 M elements), one process, the eager
step, device-synchronised wall time per step after warm-up.  The variants ALTERNATE inside one run and the whole round is
repeated, so that the run's own spread is known:
  off         guidance on, no guider: batch-2 forward + fino_cfg_euler_step.  This stands for the step of the commit before
              guiders: the unguided loop issues the same calls as that commit (tests/test_guiders_cpu.py records the list), and
              fino_cfg_euler_step compiles to the same gfx950 instructions, line for line.  It is measured in THIS run, so that it
              shares the run's clocks with the guided variants; that commit's own recorded figures for the same step are quoted
              next to it (profiles/magcache_step.txt and profiles/ras_step.txt, variant `off`: 263.85 and 263.8 ms)
  zero_star   CFGZeroStarConfig(zero_init_steps=0): forward + fino_guider_coefs (two launches) + fino_guided_euler_step
  apg         AdaptiveProjectedGuidanceConfig(guidance_rescale=0.5)
  rescale     GuidanceRescaleConfig()
and the bare launches at that shape (event-timed, alternated): fino_cfg_euler_step next to fino_guider_coefs +
fino_guided_euler_step, whose difference is the device time a guider adds to a step.  The step's difference is reported next to
the spread it has to be read against.  RANDOM weights: nothing here says anything about quality, which is not measured.
Writes profiles/guider_step.txt and prints one JSON line.

    python tools/guider_step_bench.py [--steps 5] [--warmup 2] [--rounds 3] [--out profiles/guider_step.txt]
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
from frameino_amd.guiders import (AdaptiveProjectedGuidanceConfig, CFGZeroStarConfig, GuidanceRescaleConfig,  # noqa: E402
                                  GuiderPipelineMixin, kernel_args)

C, FG, NID, LH, LW = 48, 13, 1, 44, 80
GUIDERS = {"zero_star": CFGZeroStarConfig(zero_init_steps=0),
           "apg": AdaptiveProjectedGuidanceConfig(guidance_rescale=0.5),
           "rescale": GuidanceRescaleConfig()}


def kernel_times(dev, reps=50, rounds=3):
    """ms of the bare launches, alternated, `rounds` times: {name: [ms, ...]}"""
    g = torch.Generator(device=dev).manual_seed(3)
    pc = torch.randn(C, FG + NID, LH, LW, generator=g, device=dev).bfloat16()
    pu = (0.8 * pc.float() + 0.6 * torch.randn(pc.shape, generator=g, device=dev)).bfloat16()
    lat = torch.randn(C, FG, LH, LW, generator=g, device=dev)
    dt = torch.tensor([-0.02], device=dev)
    gs = {k: GuiderPipelineMixin._guider_state(ops, cfg, lat.numel(), torch.tensor([5.0], device=dev), 4, dev)
          for k, cfg in GUIDERS.items()}

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

    def guided(k):
        s = gs[k]

        def run():
            ops.guider_coefs(pc, pu, FG, s.args, s.g, s.zero, s.workspace, s.ab)
            ops.guided_euler_step_(lat, pc, pu, s.ab, dt)
        return run

    launches = {"cfg_euler": lambda: ops.cfg_euler_step_(lat, pc, pu, 5.0, dt)}
    launches.update({f"coefs+guided_euler[{k}]": guided(k) for k in GUIDERS})
    k0 = next(iter(GUIDERS))
    launches["coefs alone"] = lambda: ops.guider_coefs(pc, pu, FG, kernel_args(GUIDERS[k0]), gs[k0].g, gs[k0].zero,
                                                       gs[k0].workspace, gs[k0].ab)
    ms = {k: [] for k in launches}
    for _ in range(rounds):
        for k, fn in launches.items():
            ms[k].append(timed(fn))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guider_step.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    from frameino_amd.pipeline_wan_i2v_motion_frameino import WanImageToVideoPipeline
    from frameino_amd.random_init import random_wan_model
    from frameino_amd.schedulers import FlowMatchEulerDiscreteScheduler
    from oracle.wan_dit import WAN22_5B_CFG
    from tests.parity import model_cfg
    cfg = WAN22_5B_CFG
    m = random_wan_model(model_cfg(cfg), dev)
    pipe = WanImageToVideoPipeline(scheduler=FlowMatchEulerDiscreteScheduler(shift=5.0), transformer=m, expand_timesteps=True)
    g = torch.Generator().manual_seed(1234)
    lat = torch.randn(1, C, FG, LH, LW, generator=g).to(dev)
    cond = torch.randn(1, C, 1, LH, LW, generator=g).to(dev)
    traj = torch.randn(1, C, FG + NID, LH, LW, generator=g).to(dev)
    traj[:, :, FG:] = 0
    idl = torch.randn(1, C, NID, LH, LW, generator=g).to(dev)
    mask = torch.ones(1, 1, FG, LH, LW, device=dev)
    mask[:, :, 0] = 0
    pe = torch.randn(1, 512, cfg["text_dim"], generator=g)
    pe[:, 64:] = 0
    ne = torch.randn(1, 512, cfg["text_dim"], generator=g)
    ne[:, 8:] = 0
    pe, ne = pe.to(dev).bfloat16(), ne.to(dev).bfloat16()
    total = a.warmup + a.steps
    pipe.scheduler.set_timesteps(max(total, 2), device=dev)
    ts, dts = pipe.scheduler.timesteps.to(dev).float(), pipe.scheduler.dts.to(dev)

    def per_step(variant):
        """ms per step of `steps` eager steps after `warmup`"""
        st = pipe.make_state(lat, cond, traj, idl, mask, pe, ne, 5.0)
        pipe._attach_guider(st, GUIDERS.get(variant), total)        # (as `denoise` does: under a guider the first frame is live)
        with torch.no_grad():
            for i in range(total):
                if i == a.warmup:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                st.t_rows[1:2].copy_(ts[i:i + 1])
                st.dt.copy_(dts[i:i + 1])
                pipe._guider_begin_step(st.guider, i)
                pipe._step(st)
            torch.cuda.synchronize()
        assert bool(torch.isfinite(st.lat).all())
        return (time.perf_counter() - t0) * 1e3 / a.steps

    variants = ("off",) + tuple(GUIDERS)
    times = {v: [] for v in variants}
    for _ in range(a.rounds):
        for v in variants:
            times[v].append(per_step(v))
    kms = kernel_times(dev, rounds=a.rounds)
    med = {v: sorted(t)[len(t) // 2] for v, t in times.items()}
    spread = {v: max(t) - min(t) for v, t in times.items()}
    kmed = {k: sorted(t)[len(t) // 2] for k, t in kms.items()}
    kspread = {k: max(t) - min(t) for k, t in kms.items()}
    res = {"L": 12320, "latent_elements": C * FG * LH * LW, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
           "ms_per_step": times, "median_ms": med, "spread_ms": spread, "kernel_ms": kms, "kernel_median_ms": kmed,
           "added_step_ms": {v: med[v] - med["off"] for v in GUIDERS},
           "added_device_ms": {v: kmed[f"coefs+guided_euler[{v}]"] - kmed["cfg_euler"] for v in GUIDERS}}
    lines = [f"guiders, full-size Wan2.2-5B DiT, bf16, L = 12320, latents [{C}, {FG}, {LH}, {LW}], eager step; {a.rounds} rounds of "
             f"{a.steps} steps after {a.warmup} warm-up steps",
             f"bare launches at that shape, {a.rounds} alternated rounds of 50:"]
    for k in kms:
        lines.append(f"  {k:32s} " + " ".join(f"{t:7.4f}" for t in kms[k]) + f" ms   median {kmed[k]:.4f} ms  spread {kspread[k]:.4f}")
    for v in GUIDERS:
        lines.append(f"  {v:10s} adds {res['added_device_ms'][v] * 1e3:+.1f} us of device time to a step's sampler launches")
    for v in variants:
        lines.append(f"{v:10s} " + " ".join(f"{t:8.2f}" for t in times[v]) + f"   median {med[v]:8.2f}  spread {spread[v]:.2f} ms/step")
    for v in GUIDERS:
        lines.append(f"{v} - off   {res['added_step_ms'][v]:+.2f} ms/step   (the run's spread: {max(spread[v], spread['off']):.2f} ms)")
    lines.append("`off` is this run's unguided step, not a run of the commit before guiders: the unguided loop issues the same calls as "
                 "that commit and fino_cfg_euler_step compiles to the same instructions.  That commit's recorded figures for this "
                 "step: 263.85 ms (profiles/magcache_step.txt, `off`), 263.8 ms (profiles/ras_step.txt, `off`)")
    lines.append("under a guider the first latent frame's prediction is computed in the last block too (the moments cover it): the "
                 "guided variants include that")
    lines.append("random weights: quality is not measured")
    lines.append(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
