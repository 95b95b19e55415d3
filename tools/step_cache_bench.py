"""First-block caching on the full-size Wan2.2-5B DiT (random weights, bf16, 49 frames 704x1280 + one ID frame: L = 12320),
one process, eager loop (the cache's loop), device-synchronised wall time per step after warm-up:
  1. cache off                        ms per step (the eager baseline of this run)
  2. threshold 0 (every step computed) ms per step, overhead against 1
  3. threshold inf (step 0 computes, every later step skips in both branches)   ms per skipped step, fraction of 1
  4. the probe kernel alone on two full-size branches, and a device copy of the same bytes (event-timed here; `--probe-only`
     runs just that part, for a `rocprofv3 --kernel-trace --stats` run of its own)
  5. one 50-step `denoise` at threshold 0.1: steps skipped and seconds -- on RANDOM weights, so the skip count says nothing
     about real checkpoints
and the box's in-run matrix peak (fino_diag_mfma_peak).  One JSON line at the end.

    python tools/step_cache_bench.py [--steps 6] [--warmup 2] [--probe-only]
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
from frameino_amd.step_cache import FirstBlockCacheConfig                  # noqa: E402

L, D = 12320, 3072


def probe_vs_copy(dev, reps=20):
    g = torch.Generator(device=dev).manual_seed(3)
    mk = lambda: torch.randn(2 * L, D, generator=g, device=dev).bfloat16()      # noqa: E731
    h0, h1, p, r, c = mk(), mk(), mk(), torch.empty(2 * L, D, dtype=torch.bfloat16, device=dev), \
        torch.empty(2 * L, D, dtype=torch.bfloat16, device=dev)
    segs = [(0, L), (L, 2 * L)]
    args = [[t[a:b] for a, b in segs] for t in (h0, h1, p, r, c)]
    nbytes = 5 * h0.numel() * h0.element_size()               # h0, h1, p read; r, h1 copy written
    src = torch.empty(nbytes // 4, dtype=torch.float16, device=dev)
    dst = torch.empty_like(src)                                # a copy moving the same bytes (half read, half written)

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

    t_probe = timed(lambda: ops.step_cache_probe(*args))
    t_copy = timed(lambda: dst.copy_(src))
    return {"probe_ms": t_probe, "probe_GBps": nbytes / t_probe / 1e6, "copy_ms": t_copy, "copy_GBps": nbytes / t_copy / 1e6,
            "probe_vs_copy": t_copy / t_probe, "probe_gbytes": nbytes / 1e9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--probe-only", action="store_true")
    ap.add_argument("--no-denoise", action="store_true", help="skip measurement 5 (the 50-step call)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.probe_only:
        print(json.dumps(probe_vs_copy(dev)))
        return
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

    def per_step(threshold):
        """ms per step of `steps` eager steps after `warmup` (state fresh at step 0, as in a call)"""
        if m.is_cache_enabled:
            m.disable_cache()
        if threshold is not None:
            m.enable_cache(FirstBlockCacheConfig(threshold=threshold))
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
        log = list(m.cache_log) if threshold is not None else []
        if m.is_cache_enabled:
            m.disable_cache()
        return ms, log

    res = {"L": L, "steps": a.steps, "warmup": a.warmup}
    off_a, _ = per_step(None)
    zero, log0 = per_step(0.0)
    skip, log_inf = per_step(float("inf"))
    off_b, _ = per_step(None)                     # cache off again: the run-to-run spread of this box in this call
    off = min(off_a, off_b)
    res.update({"off_ms_per_step": [off_a, off_b], "thr0_ms_per_step": zero, "thr0_overhead": zero / off - 1,
                "thr0_all_computed": all(e[3] for e in log0),
                "skip_ms_per_step": skip, "skip_vs_computed": skip / off,
                "inf_skipped_after_step0": all(not e[3] for e in log_inf[2:]) and len(log_inf) == 2 * total})
    res.update(probe_vs_copy(dev))
    if not a.no_denoise:
        m.enable_cache(FirstBlockCacheConfig(threshold=0.1))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe.denoise(lat, cond, traj, idl, mask, pe, ne, 5.0, 50)
        torch.cuda.synchronize()
        log = list(m.cache_log)
        res.update({"denoise50_thr0.1_s": time.perf_counter() - t0,
                    "denoise50_thr0.1_steps_skipped": [sum(1 for e in log if e[0] == c and not e[3]) for c in ("cond", "uncond")],
                    "denoise50_note": "random weights: the skip count says nothing about real checkpoints"})
        m.disable_cache()
    res.update(measured_mfma_peak(dev, 0.0))
    res.pop("frac_of_power_capped_peak", None)
    print(f"cache off        {off_a:8.1f} / {off_b:.1f} ms/step (two runs)")
    print(f"threshold 0      {zero:8.1f} ms/step  overhead {100 * res['thr0_overhead']:+.2f} %")
    print(f"threshold inf    {skip:8.1f} ms/skipped step = {100 * res['skip_vs_computed']:.1f} % of a computed step")
    print(f"probe            {res['probe_ms']:8.3f} ms  {res['probe_GBps']:.0f} GB/s = {res['probe_vs_copy']:.2f} of a copy "
          f"({res['copy_GBps']:.0f} GB/s)")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
