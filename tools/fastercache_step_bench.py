"""FasterCache on the full-size Wan2.2-5B DiT (random weights, bf16, 49 frames 704x1280 + one ID frame: L = 12320), one process,
eager loop (the cache's loop), device-synchronised wall time per step after warm-up.  The variants ALTERNATE inside one run and
the whole round is repeated, so that the run's own spread is known:
  off        guidance on, no cache: the uncached step (batch-2 forward + sampler)
  compute    FasterCache on, unconditional_batch_skip_range=1: every step runs both branches and takes the delta
             bar: compute - off <= the delta launch's device time + the spread
  skip       FasterCache on, a skip range beyond the run: step 0 computes, every later step runs the cond branch and the rebuild
  cond_only  guidance off, no cache: one batch-1 forward + the sampler
             bar: skip - cond_only <= the apply launch's device time + the spread; more is a host sync or a copy
and: the two kernels' device times at [720, 44, 80] (event-timed), one 50-step `denoise` at diffusers' defaults with and without
the self-attention part against uncached (reported, no bar; RANDOM weights: nothing about quality), the box's in-run matrix peak.
Writes profiles/fastercache_step.txt and prints one JSON line.

    python tools/fastercache_step_bench.py [--steps 6] [--warmup 2] [--rounds 3] [--no-denoise] [--out profiles/fastercache_step.txt]
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
from frameino_amd.step_cache import FasterCacheConfig                      # noqa: E402

ALL = (-1, 1001)


def kernel_times(dev, reps=20):
    g = torch.Generator(device=dev).manual_seed(3)
    u = torch.randn(720, 44, 80, generator=g, device=dev).bfloat16()
    c = torch.randn(720, 44, 80, generator=g, device=dev).bfloat16()
    dl, dh, out = torch.empty(u.shape, device=dev), torch.empty(u.shape, device=dev), torch.empty_like(u)

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

    t_delta = timed(lambda: ops.fastercache_delta(u, c, dl, dh))
    t_apply = timed(lambda: ops.fastercache_apply(c, dl, dh, 1.1, 1.21, out=out))
    nbytes = u.numel() * (2 + 2 + 4 + 4)
    return {"delta_ms": t_delta, "apply_ms": t_apply, "apply_GBps": nbytes / t_apply / 1e6, "delta_GBps": nbytes / t_delta / 1e6}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-denoise", action="store_true", help="skip the 50-step calls")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fastercache_step.txt"))
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
    ts_host = pipe.scheduler.timesteps.cpu()

    def config(n, attention=None):
        return FasterCacheConfig(unconditional_batch_skip_range=n, unconditional_batch_timestep_skip_range=ALL,
                                 spatial_attention_block_skip_range=attention, attention_weight_callback=lambda mod: 0.5,
                                 current_timestep_callback=lambda: pipe.current_timestep)

    def per_step(variant):
        """ms per step of `steps` eager steps after `warmup` (state fresh at step 0, as in a call)"""
        if m.is_cache_enabled:
            m.disable_cache()
        if variant == "compute":
            m.enable_cache(config(1))
        elif variant == "skip":
            m.enable_cache(config(10 ** 6))
        st = pipe.make_state(lat, cond, traj, idl, mask, pe, ne, 1.0 if variant == "cond_only" else 5.0)
        with torch.no_grad():
            for i in range(total):
                if i == a.warmup:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                pipe._current_timestep = ts_host[i]
                st.t_rows[1:2].copy_(ts[i:i + 1])
                st.dt.copy_(dts[i:i + 1])
                pipe._step(st)
            torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / a.steps
        log = list(m.cache_log) if m.is_cache_enabled else []
        if m.is_cache_enabled:
            m.disable_cache()
        if variant == "compute":
            assert all(e[3] for e in log) and len(log) == 2 * total
        if variant == "skip":
            assert [e[3] for e in log if e[0] == "uncond"] == [True] + [False] * (total - 1)
        return ms

    variants = ("off", "compute", "skip", "cond_only")
    times = {v: [] for v in variants}
    for _ in range(a.rounds):
        for v in variants:
            times[v].append(per_step(v))
    res = {"L": 12320, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "ms_per_step": times}
    res.update(kernel_times(dev))
    med = {v: sorted(t)[len(t) // 2] for v, t in times.items()}
    spread = {v: max(t) - min(t) for v, t in times.items()}
    res.update({"median_ms": med, "spread_ms": spread,
                "compute_minus_off_ms": med["compute"] - med["off"], "compute_bar_ms": res["delta_ms"] + max(spread["compute"], spread["off"]),
                "skip_minus_cond_only_ms": med["skip"] - med["cond_only"],
                "skip_bar_ms": res["apply_ms"] + max(spread["skip"], spread["cond_only"])})
    lines = [f"FasterCache, full-size Wan2.2-5B DiT, bf16, L = 12320, eager loop; {a.rounds} rounds of {a.steps} steps after {a.warmup} warm-up steps",
             f"kernels at [720, 44, 80]: delta {res['delta_ms']:.3f} ms, apply {res['apply_ms']:.3f} ms ({res['apply_GBps']:.0f} GB/s)"]
    for v in variants:
        lines.append(f"{v:10s} " + " ".join(f"{t:8.2f}" for t in times[v]) + f"   median {med[v]:8.2f}  spread {spread[v]:.2f} ms/step")
    lines.append(f"compute - off       {res['compute_minus_off_ms']:+.2f} ms   bar (delta launch + spread) {res['compute_bar_ms']:.2f} ms")
    lines.append(f"skip - cond_only    {res['skip_minus_cond_only_ms']:+.2f} ms   bar (apply launch + spread) {res['skip_bar_ms']:.2f} ms")
    if not a.no_denoise:
        for name, make in (("uncached", None), ("fastercache_uncond", lambda: config(5)), ("fastercache_uncond_attention", lambda: config(5, 2))):
            if make is not None:
                c_ = make()
                c_.unconditional_batch_timestep_skip_range = (-1, 641)              # diffusers' defaults
                m.enable_cache(c_)
            pipe.use_hip_graph = False
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pipe.denoise(lat, cond, traj, idl, mask, pe, ne, 5.0, 50)
            torch.cuda.synchronize()
            res[f"denoise50_{name}_s"] = time.perf_counter() - t0
            log = list(m.cache_log) if make is not None else []
            if make is not None:
                res[f"denoise50_{name}_uncond_skipped"] = sum(1 for e in log if e[0] == "uncond" and not e[3])
                res[f"denoise50_{name}_attention_skipped"] = sum(1 for e in log if e[3] and not e[4])
                m.disable_cache()
            lines.append(f"50-step denoise, {name}: {res[f'denoise50_{name}_s']:.2f} s"
                         + (f"  (uncond stacks skipped {res[f'denoise50_{name}_uncond_skipped']}, attention-skipping forwards "
                            f"{res[f'denoise50_{name}_attention_skipped']})" if make is not None else ""))
        lines.append("random weights: the 50-step times say nothing about quality on real checkpoints (not measured)")
    res.update(measured_mfma_peak(dev, 0.0))
    res.pop("frac_of_power_capped_peak", None)
    lines.append(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
