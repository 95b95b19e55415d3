"""Region-adaptive sampling on the full-size Wan2.2-5B DiT (random weights, bf16, 49 frames 704x1280 + one ID frame: L = 12320),
one process, eager loop (the policy's loop), device-synchronised wall time per step after warm-up.  The variants ALTERNATE inside
one run and the whole round is repeated, so that the run's own spread is known:
  off        guidance on, no cache: the uncached step (batch-2 forward + sampler)
  off_np     the same with `dedup_shared_prefix = False`: the uncached step without the shared CFG prefix, which the policy
             switches off (one K / V plane set per element and layer) -- what a full step is compared with
  full       the policy on, every step full: the uncached forward without the shared CFG prefix, every layer's K and V also
             written to the planes, the head rows kept
  p25 / p50 / p75   the policy on, step 0 full, every later step partial at sample_ratio 0.25 / 0.5 / 0.75 -- each reported next to
             ratio x the `off` step of the same run (what removing exactly that share of ALL work would give)
and: the bare launches at the bench shape (event-timed) -- the score + select pair over [2 x 12320, 192] head rows, the fused norm /
RoPE / scatter launch on a compact [2 x 6160, 3 x 3072] projection, and the full-forward form of that launch on all 2 x 12320 rows
next to the in-place norm + RoPE launch it replaces (their difference x 30 layers is the K / V-keep cost a full step can account
for) --, and one 50-step `denoise` at the config defaults against uncached.  RANDOM weights: nothing here says anything about
quality, which is not measured.  Writes profiles/ras_step.txt and prints one JSON line.

    python tools/ras_step_bench.py [--steps 4] [--warmup 2] [--rounds 3] [--no-denoise] [--out profiles/ras_step.txt]
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
from frameino_amd.step_cache import RegionAdaptiveSamplingConfig           # noqa: E402

N, DIM, COLS = 12320, 3072, 192
RATIOS = {"p25": 0.25, "p50": 0.5, "p75": 0.75}


def kernel_times(dev, reps=20, rounds=3):
    """ms of the bare launches, alternated, `rounds` times: {name: [ms, ...]}"""
    g = torch.Generator(device=dev).manual_seed(3)
    po = torch.randn(2 * N, COLS, generator=g, device=dev).bfloat16()
    counters = torch.zeros(N, dtype=torch.int32, device=dev)
    score, idx = torch.empty(N, dtype=torch.float32, device=dev), torch.empty(N // 2, dtype=torch.int32, device=dev)
    qkv_all = torch.randn(2 * N, 3 * DIM, generator=g, device=dev).bfloat16()
    qkv_half = qkv_all[:N].clone()                                   # 2 x 6160 compact rows
    planes = torch.empty(2, 2 * N, DIM, dtype=torch.bfloat16, device=dev)
    w = torch.ones(DIM, dtype=torch.bfloat16, device=dev)
    ang = torch.rand(2 * N, 64, generator=g, device=dev) * 6.28
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    rows = torch.randperm(N, generator=g, device=dev)[:N // 2].sort().values.to(torch.int32)
    idx2 = torch.cat([rows, rows + N])

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

    def pair():
        ops.token_score(po, batch=2, counters=counters, starvation_scale=0.1, out=score)
        ops.token_select(score, N // 2, counters=counters, out=idx)

    launches = {
        "score+select": pair,
        "rows_partial": lambda: ops.qkv_rmsnorm_rope_rows_(qkv_half, DIM, w, 1e-6, w, 1e-6, cos[:N], sin[:N], 128, idx2,
                                                           planes[0], planes[1]),
        "rows_full": lambda: ops.qkv_rmsnorm_rope_rows_(qkv_all, DIM, w, 1e-6, w, 1e-6, cos, sin, 128, None, planes[0], planes[1]),
        "in_place_full": lambda: ops.qkv_rmsnorm_rope_(qkv_all, DIM, w, 1e-6, w, 1e-6, cos, sin, 128),
    }
    ms = {k: [] for k in launches}
    for _ in range(rounds):
        for k, fn in launches.items():
            ms[k].append(timed(fn))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-denoise", action="store_true", help="skip the 50-step calls")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ras_step.txt"))
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
    far = 10 ** 6

    def config(variant):
        if variant == "full":
            return RegionAdaptiveSamplingConfig(warmup_steps=far, num_inference_steps=far)
        return RegionAdaptiveSamplingConfig(sample_ratio=RATIOS[variant], warmup_steps=1, full_step_interval=far,
                                            full_steps_at_end=0, num_inference_steps=far)

    def per_step(variant):
        """ms per step of `steps` eager steps after `warmup` (state fresh at step 0, as in a call)"""
        if m.is_cache_enabled:
            m.disable_cache()
        if variant not in ("off", "off_np"):
            m.enable_cache(config(variant))
        m.dedup_shared_prefix = variant != "off_np"
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
        rows = sorted({e[3] for e in log if not e[2]})
        if m.is_cache_enabled:
            m.disable_cache()
        m.dedup_shared_prefix = True
        if variant == "full":
            assert all(e[2] for e in log) and len(log) == 2 * total
        elif variant in RATIOS:
            assert [e[2] for e in log] == [True, True] + [False] * (2 * total - 2) and len(rows) == 1
        return ms, (rows[0] if rows else None)

    variants = ("off", "off_np", "full") + tuple(RATIOS)
    times, active = {v: [] for v in variants}, {}
    for _ in range(a.rounds):
        for v in variants:
            ms, rows = per_step(v)
            times[v].append(ms)
            active[v] = rows
    med = {v: sorted(t)[len(t) // 2] for v, t in times.items()}
    spread = {v: max(t) - min(t) for v, t in times.items()}
    kms = kernel_times(dev, rounds=a.rounds)
    kmed = {k: sorted(t)[len(t) // 2] for k, t in kms.items()}
    layers = cfg["num_layers"]
    keep_ms = layers * (kmed["rows_full"] - kmed["in_place_full"])
    res = {"L": N, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "ms_per_step": times, "median_ms": med,
           "spread_ms": spread, "active_rows": active, "kernel_ms": kms, "kernel_median_ms": kmed,
           "full_minus_off_ms": med["full"] - med["off"], "full_minus_off_np_ms": med["full"] - med["off_np"],
           "kv_keep_accounted_ms": keep_ms, "full_bar_ms": keep_ms + max(spread["full"], spread["off_np"])}
    res["full_within_accounted"] = res["full_minus_off_np_ms"] <= res["full_bar_ms"]
    lines = [f"region-adaptive sampling, full-size Wan2.2-5B DiT, bf16, L = {N}, eager loop; {a.rounds} rounds of {a.steps} steps "
             f"after {a.warmup} warm-up steps",
             f"bare launches, {a.rounds} alternated rounds of 20:"]
    what = {"score+select": f"token_score [2 x {N}, {COLS}] + token_select n = {N}, k = {N // 2}",
            "rows_partial": f"qkv_rmsnorm_rope_rows on [2 x {N // 2}, 3 x {DIM}] by a list into [2 x {N}, {DIM}] planes",
            "rows_full": f"qkv_rmsnorm_rope_rows on all [2 x {N}, 3 x {DIM}] rows (the full forward's form)",
            "in_place_full": "qkv_rmsnorm_rope (in place) on the same rows: the launch it replaces"}
    for k in kms:
        lines.append(f"  {k:14s} " + " ".join(f"{t:7.4f}" for t in kms[k]) + f" ms   median {kmed[k]:.4f} ms   {what[k]}")
    for v in variants:
        lines.append(f"{v:6s} " + " ".join(f"{t:8.2f}" for t in times[v]) + f"   median {med[v]:8.2f}  spread {spread[v]:.2f} ms/step"
                     + (f"   {active[v]} of {N} rows per element" if active.get(v) else ""))
    lines.append(f"full - off      {res['full_minus_off_ms']:+.2f} ms   (of which off_np - off = {med['off_np'] - med['off']:+.2f} ms: the "
                 f"shared CFG prefix, off under the policy)")
    lines.append(f"full - off_np   {res['full_minus_off_np_ms']:+.2f} ms   accounted for: {layers} layers x (rows_full - in_place_full) "
                 f"= {keep_ms:.2f} ms of K / V-keep launches, + the run's spread {max(spread['full'], spread['off_np']):.2f} ms = "
                 f"{res['full_bar_ms']:.2f} ms   {'within' if res['full_within_accounted'] else 'MORE THAN ACCOUNTED FOR'}")
    for v, r in RATIOS.items():
        res[f"{v}_over_ratio_x_off"] = med[v] / (r * med["off"])
        lines.append(f"{v}: {med[v]:8.2f} ms next to {r} x off = {r * med['off']:8.2f} ms   ({res[f'{v}_over_ratio_x_off']:.3f} x; "
                     f"{med[v] / med['off']:.3f} of the uncached step)")
    if not a.no_denoise:
        for name, make in (("uncached", None), ("ras", lambda: RegionAdaptiveSamplingConfig())):
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
                log = [e for e in m.cache_log if e[0] == "cond"]
                res["denoise50_ras_partial_steps"] = sum(1 for e in log if not e[2])
                extra = f"  ({res['denoise50_ras_partial_steps']} of {len(log)} steps partial at sample_ratio 0.5)"
                m.disable_cache()
            lines.append(f"50-step denoise, {name}: {res[f'denoise50_{name}_s']:.2f} s{extra}")
    lines.append(f"peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")
    lines.append("random weights: quality on real checkpoints is not measured")
    lines.append(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
