"""TaylorSeer caching on the full-size Wan2.2-5B DiT (random weights, bf16, 49 frames 704x1280 + one ID frame: L = 12320), one
process, eager loop (the cache's loop):
  k. the two kernels at [12320, 3072] bf16 (factors bf16), event-timed beside fino_pab_broadcast on the same operands:
     `--rounds` rounds, each timing every launch `--reps` times back to back, the launches taken in turn inside a round
     (alternated), medians over the rounds.  The prediction's bar: its time must not exceed fino_pab_broadcast's scaled by
     the bytes moved (n planes + x read + x written against x + y read + x written) times 1.15.
  a. cache off                                                    ms per step (device-synchronised wall time, twice)
  b. TaylorSeer on, every step computes (cache_interval 1)        ms per step, default and lite mode
  c. every timed step predicts, default mode                      ms per step, beside Pyramid Attention Broadcast's step that
     re-uses both kinds
  d. every timed step predicts, lite mode                         ms per step
  f. one 50-step `denoise` at the config defaults (interval 5, warm-up 3, order 1) in both modes, and one without the cache:
     seconds per clip and the rel-RMS of the final latents -- on RANDOM weights, so the rel-RMS says nothing about real
     checkpoints
One JSON line at the end.

    python tools/taylorseer_bench.py [--steps 4] [--warmup 2] [--rounds 7] [--reps 10] [--no-denoise] [--kernels-only]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from frameino_amd import ops                                                                   # noqa: E402
from frameino_amd.step_cache import PyramidAttentionBroadcastConfig, TaylorSeerCacheConfig    # noqa: E402

L, D = 12320, 3072
MARGIN = 1.15                     # the spread of such launches in profiles/ is up to about 6 %


def kernels(dev, rounds, reps):
    g = torch.Generator(device=dev).manual_seed(3)
    mk = lambda *s: torch.randn(*s, generator=g, device=dev).bfloat16()      # noqa: E731
    # (results go to `out`, not back into x, and updates start from a copy of the same planes: every repetition sees the
    # same finite operands)
    x, y, out = mk(L, D), mk(L, D), torch.empty(L, D, dtype=torch.bfloat16, device=dev)
    fac = mk(4, L, D)
    gate = torch.randn(2, D, generator=g, device=dev)
    sel = (torch.arange(L, device=dev) < 880).to(torch.int32)
    unit = x.numel() * 2                                                      # bytes of one [L, D] bf16 pass
    launches = {"pab_broadcast": (lambda: ops.pab_broadcast(x, y, gate, sel, out=out), 3)}
    for n in (1, 2, 3):
        launches[f"predict_n{n}"] = (lambda n=n: ops.taylor_predict(fac, n, 2, x, gate, sel, out=out), n + 2)
    launches["predict_n2_lite_form"] = (lambda: ops.taylor_predict(fac, 2, 2, out=out), 3)
    for n_old in (0, 1, 2):                                                   # reads y + n_old planes, writes n_old + 1
        launches[f"update_n{n_old}_to_{n_old + 1}"] = (lambda n_old=n_old: ops.taylor_update(y, fac, n_old, 3, n_old + 1),
                                                       2 * n_old + 2)

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / reps

    for fn, _ in launches.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in launches}
    for _ in range(rounds):
        for k, (fn, _) in launches.items():
            ms[k].append(timed(fn))
    res = {}
    pab = statistics.median(ms["pab_broadcast"])
    for k, (_, units) in launches.items():
        med = statistics.median(ms[k])
        res[k] = {"ms": med, "min_ms": min(ms[k]), "max_ms": max(ms[k]), "bytes": units * unit, "GBps": units * unit / med / 1e6}
        if k.startswith("predict_n") and not k.endswith("form"):
            res[k]["bar_ms"] = pab * units / 3 * MARGIN
            res[k]["within_bar"] = med <= res[k]["bar_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-denoise", action="store_true", help="skip measurement f (the three 50-step calls)")
    ap.add_argument("--kernels-only", action="store_true", help="measurement k alone")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"L": L, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "reps": a.reps, "kernels": kernels(dev, a.rounds, a.reps)}
    for k, v in res["kernels"].items():
        bar = f"  bar {v['bar_ms']:.4f} ms: {'within' if v['within_bar'] else 'MISSED'}" if "bar_ms" in v else ""
        print(f"k. {k:22s} {v['ms']:.4f} ms (min {v['min_ms']:.4f}, max {v['max_ms']:.4f})  {v['GBps']:7.0f} GB/s{bar}")
    if a.kernels_only:
        print(json.dumps(res))
        return
    from frameino_amd.pipeline_wan_i2v_motion_frameino import WanImageToVideoPipeline
    from frameino_amd.random_init import random_wan_model
    from frameino_amd.schedulers import FlowMatchEulerDiscreteScheduler
    from oracle.wan_dit import WAN22_5B_CFG
    from tests.parity import model_cfg, rel_rms
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
    big = 10 ** 6                 # an interval no counter reaches: every step after the warm-up predicts / re-uses

    def per_step(config=None):
        """ms per step of `steps` eager steps after `warmup` (state fresh at step 0, as in a call), and the timed steps' log"""
        if m.is_cache_enabled:
            m.disable_cache()
        if config is not None:
            m.enable_cache(config)
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
        log = [e for e in m.cache_log if e[1] >= a.warmup] if config is not None else []
        if m.is_cache_enabled:
            m.disable_cache()
        return ms, log

    taylor = lambda lite, interval: TaylorSeerCacheConfig(cache_interval=interval, disable_cache_before_step=a.warmup,      # noqa: E731
                                                          use_lite_mode=lite)
    pab_both = PyramidAttentionBroadcastConfig(spatial_attention_block_skip_range=big, cross_attention_block_skip_range=big,
                                               spatial_attention_timestep_skip_range=(-1, 1001),
                                               cross_attention_timestep_skip_range=(-1, 1001), current_timestep_callback=lambda: 500.0)
    off_a, _ = per_step()
    b_ms, log_b = per_step(taylor(False, 1))
    b_lite_ms, log_bl = per_step(taylor(True, 1))
    c_ms, log_c = per_step(taylor(False, big))
    pab_ms, log_p = per_step(pab_both)
    d_ms, log_d = per_step(taylor(True, big))
    off_b, _ = per_step()                         # cache off again: the run-to-run spread of this box in this call
    n2 = 2 * a.steps
    res.update({"a_off_ms_per_step": [off_a, off_b], "b_computing_ms_per_step": b_ms, "b_computing_lite_ms_per_step": b_lite_ms,
                "b_all_computed": all(e[2] for e in log_b + log_bl) and len(log_b) == len(log_bl) == n2,
                "c_predicting_ms_per_step": c_ms, "c_predicted": not any(e[2] for e in log_c) and len(log_c) == n2,
                "c_pab_reuse_both_ms_per_step": pab_ms, "c_pab_reused": not any(e[3] or e[4] for e in log_p) and len(log_p) == n2,
                "d_predicting_lite_ms_per_step": d_ms, "d_predicted": not any(e[2] for e in log_d) and len(log_d) == n2})
    print(f"a. cache off                          {off_a:8.1f} / {off_b:.1f} ms/step (two runs)")
    print(f"b. every step computes                {b_ms:8.1f} ms/step (default mode)  {b_lite_ms:.1f} ms/step (lite mode)")
    print(f"c. every step predicts, default mode  {c_ms:8.1f} ms/step   Pyramid Attention Broadcast re-using both kinds {pab_ms:.1f} ms/step")
    print(f"d. every step predicts, lite mode     {d_ms:8.2f} ms/step")
    if not a.no_denoise:
        clips, logs = {}, {}
        for name, config in (("off", None), ("default", TaylorSeerCacheConfig()), ("lite", TaylorSeerCacheConfig(use_lite_mode=True))):
            if config is not None:
                m.enable_cache(config)
            pipe.use_hip_graph = False                # every call on the eager loop
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = pipe.denoise(lat, cond, traj, idl, mask, pe, ne, 5.0, 50)
            torch.cuda.synchronize()
            clips[name] = (time.perf_counter() - t0, out)
            logs[name] = list(m.cache_log) if config is not None else []
            if config is not None:
                m.disable_cache()
        pipe.use_hip_graph = None
        res.update({"denoise50_off_ms_per_clip": clips["off"][0] * 1e3,
                    "denoise50_note": "random weights: the rel-RMS says nothing about real checkpoints"})
        for name in ("default", "lite"):
            res.update({f"denoise50_{name}_ms_per_clip": clips[name][0] * 1e3,
                        f"denoise50_{name}_predicted_steps": sum(1 for e in logs[name] if e[0] == "cond" and not e[2]),
                        f"denoise50_{name}_rel_rms_vs_off": rel_rms(clips[name][1], clips["off"][1])})
        print(f"f. 50 steps at the config defaults: off {res['denoise50_off_ms_per_clip']:.0f} ms/clip, default mode "
              f"{res['denoise50_default_ms_per_clip']:.0f} ms/clip ({res['denoise50_default_predicted_steps']} predicted steps, rel-RMS "
              f"of the latents {res['denoise50_default_rel_rms_vs_off']:.3e}), lite mode {res['denoise50_lite_ms_per_clip']:.0f} ms/clip "
              f"({res['denoise50_lite_predicted_steps']} predicted steps, rel-RMS {res['denoise50_lite_rel_rms_vs_off']:.3e}) -- random weights")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
