"""Pyramid Attention Broadcast on the full-size Wan2.2-5B DiT (random weights, bf16, 49 frames 704x1280 + one ID frame: L = 12320),
one process, eager loop (the cache's loop), device-synchronised wall time per step after warm-up:
  a. cache off                                                   ms per step (the eager baseline of this run, twice)
  b. PAB on, a timestep range that excludes every step           ms per step: every step computes and keeps y
  c. spatial range set, every timed step re-uses self-attention  ms per step
  d. spatial + cross set, every timed step re-uses both          ms per step
  (a and b also with the CFG branches as two sequential calls: there b - a is the keep stores plus the last block's dead rows,
  which PAB computes; in the batched form PAB also runs the attention branches element by element and without the shared prefix)
  e. the out-projection at one branch's shape (M = 12320, N = K = 3072), event-timed: the gated-residual GEMM, the same with
     keep=, and the two-launch form (EPI_NONE into the keep buffer + ops.pab_broadcast); the text branch's closing GEMM
     (K = 1728) likewise; and the re-use launch alone
  f. one 50-step `denoise` with spatial=2, cross=3 over (100, 800), and one without the cache: seconds per clip and the rel-RMS
     of the final latents -- on RANDOM weights, so the rel-RMS says nothing about real checkpoints
and the box's in-run matrix peak (fino_diag_mfma_peak).  One JSON line at the end.

    python tools/pab_bench.py [--steps 4] [--warmup 2] [--no-denoise]
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
from frameino_amd.step_cache import PyramidAttentionBroadcastConfig        # noqa: E402

L, D = 12320, 3072
NEVER, ALWAYS = (2000, 3000), (-1, 1001)          # timestep ranges no step / every step lies inside


def keep_forms(dev, reps=10):
    g = torch.Generator(device=dev).manual_seed(3)
    mk = lambda *s: torch.randn(*s, generator=g, device=dev).bfloat16()      # noqa: E731
    # (the result goes to `out`, not back into the residual x: the operands of every repetition are the same finite values)
    x, keep, gate = mk(L, D), torch.empty(L, D, dtype=torch.bfloat16, device=dev), torch.randn(2, D, generator=g, device=dev)
    out_ = torch.empty_like(x)
    sel = (torch.arange(L, device=dev) < 880).to(torch.int32)
    bias = mk(D)

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

    out = {}
    for name, k, epi, gt, sl in (("out_proj", D, ops.EPI_GATED_RESIDUAL, gate, sel), ("text_out", 1728, ops.EPI_RESIDUAL, None, None)):
        a, w = mk(L, k), mk(D, k) * k ** -0.5

        def two_launch():
            ops.gemm(a, w, bias, ops.EPI_NONE, out=keep)
            ops.pab_broadcast(x, keep, gt, sl, out=out_)

        out[name] = {"gemm_ms": timed(lambda: ops.gemm(a, w, bias, epi, residual=x, gate=gt, sel=sl, out=out_)),
                     "gemm_keep_ms": timed(lambda: ops.gemm(a, w, bias, epi, residual=x, gate=gt, sel=sl, out=out_, keep=keep)),
                     "two_launch_ms": timed(two_launch)}
    keep.copy_(mk(L, D))
    t = timed(lambda: ops.pab_broadcast(x, keep, gate, sel, out=out_))
    # (x and y read, out written: the gate rows and the selector, 0.2 % of that, are not counted)
    out["reuse_launch"] = {"ms": t, "GBps": 3 * x.numel() * 2 / t / 1e6}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-denoise", action="store_true", help="skip measurement f (the two 50-step calls)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    from bench import measured_mfma_peak
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
    ts_host = [float(t) for t in pipe.scheduler.timesteps]
    clock = {"t": 0.0}

    def enable(spatial, cross, rng):
        m.enable_cache(PyramidAttentionBroadcastConfig(
            spatial_attention_block_skip_range=spatial, cross_attention_block_skip_range=cross,
            spatial_attention_timestep_skip_range=rng, cross_attention_timestep_skip_range=rng,
            current_timestep_callback=lambda: clock["t"]))

    def per_step(pab=None):
        """ms per step of `steps` eager steps after `warmup` (state fresh at step 0, as in a call); pab = (spatial, cross, range)"""
        if m.is_cache_enabled:
            m.disable_cache()
        if pab is not None:
            enable(*pab)
        st = pipe.make_state(lat, cond, traj, idl, mask, pe, ne, 5.0)
        with torch.no_grad():
            for i in range(total):
                if i == a.warmup:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                clock["t"] = ts_host[i]
                st.t_rows[1:2].copy_(ts[i:i + 1])
                st.dt.copy_(dts[i:i + 1])
                pipe._step(st)
            torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / a.steps
        log = [e for e in m.cache_log if e[1] >= a.warmup] if pab is not None else []
        if m.is_cache_enabled:
            m.disable_cache()
        return ms, log

    big = 10 ** 6             # a block skip range no counter reaches: every in-range step after the first re-uses
    res = {"L": L, "steps": a.steps, "warmup": a.warmup}
    off_a, _ = per_step()
    b_ms, log_b = per_step((2, 2, NEVER))
    c_ms, log_c = per_step((big, None, ALWAYS))
    d_ms, log_d = per_step((big, big, ALWAYS))
    off_b, _ = per_step()                         # cache off again: the run-to-run spread of this box in this call
    off = min(off_a, off_b)
    res.update({"a_off_ms_per_step": [off_a, off_b], "b_all_computed_ms_per_step": b_ms, "b_minus_a_ms": b_ms - off,
                "b_all_computed": all(e[3] and e[4] for e in log_b) and len(log_b) == 2 * a.steps,
                "c_reuse_self_ms_per_step": c_ms, "c_reused": all(not e[3] and e[4] for e in log_c) and len(log_c) == 2 * a.steps,
                "d_reuse_both_ms_per_step": d_ms, "d_reused": all(not e[3] and not e[4] for e in log_d) and len(log_d) == 2 * a.steps})
    pipe.batch_cfg = False
    seq_a, _ = per_step()
    seq_b, _ = per_step((2, 2, NEVER))
    pipe.batch_cfg = True
    res.update({"sequential_cfg_a_off_ms_per_step": seq_a, "sequential_cfg_b_all_computed_ms_per_step": seq_b,
                "sequential_cfg_b_minus_a_ms": seq_b - seq_a})
    res["keep_forms"] = keep_forms(dev)
    if not a.no_denoise:
        clips = {}
        for name in ("off", "pab"):
            if name == "pab":
                m.enable_cache(PyramidAttentionBroadcastConfig(spatial_attention_block_skip_range=2,
                                                               cross_attention_block_skip_range=3,
                                                               current_timestep_callback=lambda: pipe.current_timestep))
            pipe.use_hip_graph = False                # both calls on the eager loop
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = pipe.denoise(lat, cond, traj, idl, mask, pe, ne, 5.0, 50)
            torch.cuda.synchronize()
            clips[name] = (time.perf_counter() - t0, out)
        log = list(m.cache_log)
        m.disable_cache()
        pipe.use_hip_graph = None
        res.update({"denoise50_off_ms_per_clip": clips["off"][0] * 1e3, "denoise50_pab_s2_c3_ms_per_clip": clips["pab"][0] * 1e3,
                    "denoise50_pab_self_reused_steps": sum(1 for e in log if e[0] == "cond" and not e[3]),
                    "denoise50_pab_cross_reused_steps": sum(1 for e in log if e[0] == "cond" and not e[4]),
                    "denoise50_rel_rms_vs_off": rel_rms(clips["pab"][1], clips["off"][1]),
                    "denoise50_note": "random weights: the rel-RMS says nothing about real checkpoints"})
    res.update(measured_mfma_peak(dev, 0.0))
    res.pop("frac_of_power_capped_peak", None)
    print(f"a. cache off                 {off_a:8.1f} / {off_b:.1f} ms/step (two runs)")
    print(f"b. PAB on, all computed      {b_ms:8.1f} ms/step  b - a = {b_ms - off:+.2f} ms")
    print(f"c. self-attention re-used    {c_ms:8.1f} ms/step")
    print(f"d. both re-used              {d_ms:8.1f} ms/step")
    print(f"   sequential CFG calls: a   {seq_a:8.1f}  b {seq_b:.1f} ms/step  b - a = {seq_b - seq_a:+.2f} ms")
    for name, v in res["keep_forms"].items():
        print(f"e. {name:12s} " + "  ".join(f"{k} {x:.3f}" for k, x in v.items()))
    if not a.no_denoise:
        print(f"f. 50 steps: off {res['denoise50_off_ms_per_clip']:.0f} ms/clip, spatial=2 cross=3 over (100, 800) "
              f"{res['denoise50_pab_s2_c3_ms_per_clip']:.0f} ms/clip, rel-RMS of the latents {res['denoise50_rel_rms_vs_off']:.3e} "
              f"(random weights)")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
