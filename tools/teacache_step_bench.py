"""TeaCache on the full-size Wan2.2-5B DiT (random weights, bf16, 49 frames 704x1280 + one ID frame: L = 12320), one process,
eager loop (the cache's loop), device-synchronised wall time per step after warm-up.  The variants ALTERNATE inside one run and
the whole round is repeated, so that the run's own spread is known:
  off        guidance on, no cache: the uncached step (batch-2 forward + sampler)
  compute    TeaCache on, identity polynomial, rel_l1_thresh = 0: every step keeps h0, probes both contexts, reads the sums,
             runs the stack and stores the residual
             bar: compute - off <= the launches it adds, each timed on its own (the h0 copy, two probes, two residual stores)
             + the run's spread
  calibrate  TeaCache in calibrate mode: every step runs the stack, the two input probes and the two plain probes of the head's
             rows; nothing is read
  skip       TeaCache on, the zero polynomial, no cap: step 0 computes, every later step skips the stack in BOTH contexts:
             embedding, h0 copy, two probes, one read, two residual adds, output head, sampler
  mag_skip   MagCache's skipping step in the same run (ratios of 1.0, nothing retained, no skip limit)
and: the ops a skipping step calls, by name (a recording proxy in front of frameino_amd.ops for one step: no block's op is
among them); the bare launches at [24640, 3072] bf16 (event-timed) -- fino_teacache_probe (three planes moved: x in, p in,
m out) next to fino_adaln_modulate (two) and fino_magcache_calibrate (four), in bytes per second --; one 50-step `denoise` on
SYNTHETIC coefficients against uncached, with the count of skipped forwards (reported, no bar); and the box's in-run matrix
peak.  RANDOM weights and a made-up polynomial: nothing here says anything about a real checkpoint or about quality, which is
not measured.  Writes profiles/teacache_step.txt and prints one JSON line.

    python tools/teacache_step_bench.py [--steps 6] [--warmup 2] [--rounds 3] [--no-denoise] [--out profiles/teacache_step.txt]
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
from frameino_amd.step_cache import MagCacheConfig, TeaCacheConfig         # noqa: E402

ROWS, DIM = 2 * 12320, 3072
SYNTHETIC = [1.0, 0.0]          # P(d) = d: the accumulated estimate is the accumulated input distance itself


class _Recorder:
    """frameino_amd.ops with every call noted by name"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(ops, name)
        if not callable(fn):
            return fn

        def call(*a, **kw):
            self.calls.append(name)
            return fn(*a, **kw)
        return call


def kernel_times(dev, reps=20, rounds=3):
    """ms of the bare launches, alternated, `rounds` times: {name: [ms, ...]} and the byte counts"""
    g = torch.Generator(device=dev).manual_seed(3)
    mk = lambda rows=ROWS: torch.randn(rows, DIM, generator=g, device=dev).bfloat16()           # noqa: E731
    x, x_in, r_prev, plane = mk(), mk(), mk(), mk()
    out = torch.empty_like(x)
    table = 0.1 * torch.randn(1, 2, DIM, generator=g, device=dev)
    shift, scale = table[:, 0], table[:, 1]
    stats = torch.zeros(2, dtype=torch.float64, device=dev)
    half = ROWS // 2
    full = ROWS * DIM * 2

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

    launches = {"probe": (lambda: ops.teacache_probe(x, plane, stats, shift, scale, None, 1e-6), 3 * full),
                "adaln_modulate": (lambda: ops.adaln_modulate(x, shift, scale, None, 1e-6, out=out), 2 * full),
                "magcache_calibrate": (lambda: ops.magcache_calibrate(x, x_in, r_prev, out, stats), 4 * full),
                # what a computing step adds, at the shapes it launches them with (two contexts of 12320 rows each)
                "h0_copy": (lambda: out.copy_(x), 2 * full),
                "probe_12320": (lambda: ops.teacache_probe(x[:half], plane[:half], stats, shift, scale, None, 1e-6), 3 * full // 2),
                "residual_12320": (lambda: ops.step_cache_residual(x[:half], x_in[:half], out=out[:half], subtract=True),
                                   3 * full // 2)}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "teacache_step.txt"))
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

    n = total + 1               # (the config's step count: the run never reaches the last step, which would always compute)
    configs = {"compute": lambda: TeaCacheConfig(coefficients=SYNTHETIC, rel_l1_thresh=0.0, num_inference_steps=n),
               "calibrate": lambda: TeaCacheConfig(calibrate=True, num_inference_steps=n),
               "skip": lambda: TeaCacheConfig(coefficients=[0.0], num_inference_steps=n),
               "mag_skip": lambda: MagCacheConfig(mag_ratios=[1.0] * total, num_inference_steps=n, retention_ratio=0.0,
                                                  max_skip_steps=10 ** 6)}
    skip_calls = []

    def per_step(variant, record=False):
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
                if record and i == total - 1:           # the last step of a recording run, through the proxy
                    rec = m.ops = _Recorder()
                    try:
                        pipe._step(st)
                    finally:
                        m.ops = ops
                    skip_calls[:] = rec.calls
                else:
                    pipe._step(st)
            torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / a.steps
        log = list(m.cache_log) if m.is_cache_enabled else []
        if m.is_cache_enabled:
            m.disable_cache()
        if variant in ("compute", "calibrate"):
            assert all(e[2] for e in log) and len(log) == 2 * total
        if variant in ("skip", "mag_skip"):
            assert [e[2] for e in log] == [True, True] + [False] * (2 * total - 2)
        return ms

    variants = ("off", "compute", "calibrate", "skip", "mag_skip")
    times = {v: [] for v in variants}
    for _ in range(a.rounds):
        for v in variants:
            times[v].append(per_step(v))
    per_step("skip", record=True)                       # (not timed: one more run whose last step goes through the proxy)
    res = {"L": 12320, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "ms_per_step": times,
           "skipping_step_ops": list(skip_calls)}
    block_ops = {"attention", "attention_fp8", "attention_ranges", "qkv_rmsnorm_rope_", "rmsnorm_rope_", "gated_residual"}
    # (the head runs once per live row segment, a modulated norm and its GEMM each time; the one other GEMM is the embedding)
    res["skipping_step_runs_no_block"] = (not (block_ops & set(skip_calls))
                                          and skip_calls.count("gemm") == 1 + skip_calls.count("adaln_modulate"))
    kms, kbytes = kernel_times(dev, rounds=a.rounds)
    kmed = {k: sorted(t)[len(t) // 2] for k, t in kms.items()}
    gmed = {k: kbytes[k] / kmed[k] / 1e6 for k in kms}
    gspread = {k: max(kbytes[k] / t / 1e6 for t in kms[k]) - min(kbytes[k] / t / 1e6 for t in kms[k]) for k in kms}
    med = {v: sorted(t)[len(t) // 2] for v, t in times.items()}
    spread = {v: max(t) - min(t) for v, t in times.items()}
    added = kmed["h0_copy"] + 2 * kmed["probe_12320"] + 2 * kmed["residual_12320"]
    res.update({"median_ms": med, "spread_ms": spread, "kernel_ms": kms, "kernel_median_ms": kmed, "kernel_GBps": gmed,
                "kernel_GBps_spread": gspread, "compute_minus_off_ms": med["compute"] - med["off"], "added_launches_ms": added,
                "compute_bar_ms": added + max(spread["compute"], spread["off"]),
                "calibrate_minus_compute_ms": med["calibrate"] - med["compute"]})
    res["compute_bar_met"] = res["compute_minus_off_ms"] <= res["compute_bar_ms"]
    lines = [f"TeaCache, full-size Wan2.2-5B DiT, bf16, L = 12320, eager loop; {a.rounds} rounds of {a.steps} steps after {a.warmup} warm-up steps",
             f"bare launches, bf16, {a.rounds} alternated rounds of 20 (the first three at [{ROWS}, {DIM}]):"]
    for k in kms:
        lines.append(f"  {k:18s} " + " ".join(f"{t:7.4f}" for t in kms[k]) + f" ms   median {kmed[k]:.4f} ms = {gmed[k]:.0f} GB/s "
                     f"over {kbytes[k] / 2 ** 20:.0f} MiB (spread {gspread[k]:.0f} GB/s)")
    for v in variants:
        lines.append(f"{v:10s} " + " ".join(f"{t:8.2f}" for t in times[v]) + f"   median {med[v]:8.2f}  spread {spread[v]:.2f} ms/step")
    lines.append(f"compute - off         {res['compute_minus_off_ms']:+.2f} ms   bar (h0 copy + 2 probes + 2 residual stores = "
                 f"{added:.2f} ms, + spread) {res['compute_bar_ms']:.2f} ms   {'met' if res['compute_bar_met'] else 'MISSED'}")
    lines.append(f"calibrate - compute   {res['calibrate_minus_compute_ms']:+.2f} ms   (two plain probes of the head's rows more, "
                 f"no host read)")
    lines.append(f"skip / off            {med['skip'] / med['off']:.4f}   (a step that skips the stack in both contexts); "
                 f"MagCache's skipping step: {med['mag_skip'] / med['off']:.4f}; skip - mag_skip {med['skip'] - med['mag_skip']:+.2f} ms")
    lines.append("ops of one skipping step (both contexts), in call order: " + " ".join(skip_calls))
    lines.append(f"a skipping step runs no block: {res['skipping_step_runs_no_block']} (no attention, q/k norm or gated residual; "
                 f"its GEMMs are the patch embedding and the output head's, one per live row segment)")
    if not a.no_denoise:
        for name, make in (("uncached", None),
                           ("teacache", lambda: TeaCacheConfig(coefficients=SYNTHETIC, num_inference_steps=50))):
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
                res["denoise50_teacache_skipped_forwards"] = sum(1 for e in log if not e[2])
                res["denoise50_teacache_forwards"] = len(log)
                ds = [e[3] for e in log if e[3] is not None]
                res["denoise50_teacache_d_min_max"] = [min(ds), max(ds)] if ds else None
                extra = f"  ({res['denoise50_teacache_skipped_forwards']} of {len(log)} forwards skipped their stack)"
                m.disable_cache()
            lines.append(f"50-step denoise, {name}: {res[f'denoise50_{name}_s']:.2f} s{extra}")
        lines.append("the 50-step TeaCache call runs at the config defaults (rel_l1_thresh 0.2, ret_steps 1, no cap) on SYNTHETIC "
                     "coefficients, P(d) = d: no real checkpoint's polynomial is known here")
    lines.append("random weights: a polynomial fitted on them says nothing about real checkpoints, and quality on real checkpoints "
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
