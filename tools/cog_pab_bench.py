#!/usr/bin/env python3
"""Pyramid Attention Broadcast on the CogVideoX-5B FrameINO backbone at BASELINE config 5 ([2, 14, 48, 60,
90]: 226 text rows + 14 latent frames x 1350 tokens, L = 19126, random weights), measured on one box in one process with the method
of tools/pab_bench.py and tools/cog_window_attention_bench.py: device events for launches, a host clock around synchronised steps,
the arms alternated round by round, medians with min / max.

  a. the out-projection LAUNCH (M = 2 x 19126, N = K = 3072, FINO_EPI_GATED_RESIDUAL_STAGED), for MXFP8 and MXFP6: the MX GEMM
     without keep, the one-launch `keep=` call (fino_gemm_mxfp8_keep / fino_gemm_mxfp6_keep), and the two launches it replaces
     (the EPI_NONE MX GEMM into the keep buffer + the staged residual pass); the re-use launch alone.  The bar: one launch is not
     slower than the pair beyond the rounds' own spread;
  b. the denoise STEP (CFG batch, eager): cache off, a computing step (cache on, a timestep range that excludes every step) and a
     re-using step (every timed step re-uses), in bf16 and with MXFP8 linears + fp8 attention;
  c. with --denoise: one 50-step `denoise` with spatial 2 over (100, 800) against the uncached eager loop and the uncached graph loop
     (seconds per clip; the rel-RMS of the final latents is on RANDOM weights and says nothing about real checkpoints).

    python tools/cog_pab_bench.py [--rounds 7] [--steps 2] [--denoise] [--out profiles/cog_pab_step.txt]

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
from frameino_amd.step_cache import PyramidAttentionBroadcastConfig  # noqa: E402

FRAMES, TPF, TEXT, D = 14, 1350, 226, 3072
L = TEXT + FRAMES * TPF
NEVER, ALWAYS = (2000, 3000), (-1, 1001)          # timestep ranges no step / every step lies inside
BIG = 10 ** 6                                     # a block skip range no counter reaches: every in-range step after the first re-uses


def _stats(v):
    return statistics.median(v), min(v), max(v)


def _alternate(runs, rounds, reps):
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
    return {n: _stats(v) for n, v in t.items()}


def keep_launches(rounds, reps, m=2 * L):
    """us per call of the out-projection's forms.  The result goes to `out`, not back into the residual x: the operands of every
    repetition are the same finite values."""
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(3)
    mk = lambda *s: torch.randn(*s, generator=g, device=dev).bfloat16()      # noqa: E731
    a, w, bias, x = mk(m, D), mk(D, D) * D ** -0.5, mk(D), mk(m, D)
    keep, out = torch.empty_like(x), torch.empty_like(x)
    gate = torch.randn(4, D, generator=g, device=dev)                        # [2 B, D]: row 2 b = video, 2 b + 1 = text
    sel = torch.zeros(2, L, dtype=torch.int32, device=dev)
    sel[:, :TEXT] = 1
    sel = (sel + 2 * torch.arange(2, device=dev, dtype=torch.int32)[:, None]).reshape(-1).contiguous()
    epi = ops.EPI_GATED_RESIDUAL_STAGED
    res = {}
    for fmt, quantize, gemm in (("MXFP8", ops.quantize_mxfp8, ops.gemm_mxfp8), ("MXFP6", ops.quantize_mxfp6, ops.gemm_mxfp6)):
        (aq, sa), (wq, sw) = quantize(a), quantize(w)

        def two_launches():
            gemm(aq, sa, wq, sw, bias, ops.EPI_NONE, out=keep)
            ops.gated_residual(x, keep, gate, sel, out=out, staged=True)

        res[fmt] = _alternate({
            "GEMM without keep": lambda: gemm(aq, sa, wq, sw, bias, epi, residual=x, gate=gate, sel=sel, out=out),
            "one launch, keep=": lambda: gemm(aq, sa, wq, sw, bias, epi, residual=x, gate=gate, sel=sel, out=out, keep=keep),
            "two launches (EPI_NONE + residual pass)": two_launches}, rounds, reps)
        # same seeded operands, both forms: the bits must agree before the times are compared
        want_keep, want_out = keep.clone(), out.clone()
        gemm(aq, sa, wq, sw, bias, epi, residual=x, gate=gate, sel=sel, out=out, keep=keep)
        torch.cuda.synchronize()
        assert torch.equal(keep, want_keep) and torch.equal(out, want_out), f"{fmt}: one launch and two launches disagree"
    res["re-use"] = _alternate({"re-use launch (gated_residual, staged)":
                                lambda: ops.gated_residual(x, keep, gate, sel, out=out, staged=True)}, rounds, reps)
    return res


def _pipe():
    from frameino_amd.configs import COGVIDEOX_5B_FRAMEINO_CFG as COG5B
    from frameino_amd.pipeline_cogvideox_i2v_motion_frameino import CogVideoXImageToVideoPipeline
    from frameino_amd.random_init import random_cog_model
    from frameino_amd.schedulers import CogVideoXDDIMScheduler
    dev = torch.device("cuda")
    m = random_cog_model(dict(COG5B), dev)
    pipe = CogVideoXImageToVideoPipeline(transformer=m, scheduler=CogVideoXDDIMScheduler())
    g = torch.Generator(device=dev).manual_seed(1)
    F_, C_, h, w = FRAMES - 1, 16, 60, 90
    lat = torch.randn(1, F_, C_, h, w, device=dev, generator=g)
    img = torch.cat([torch.randn(1, 1, C_, h, w, device=dev, generator=g), torch.zeros(1, F_ - 1, C_, h, w, device=dev)], 1)
    trj = torch.randn(1, F_, C_, h, w, device=dev, generator=g)
    idl = torch.randn(1, 1, C_, h, w, device=dev, generator=g)
    pe, ne = torch.randn(1, TEXT, 4096, device=dev, generator=g), torch.randn(1, TEXT, 4096, device=dev, generator=g)
    return pipe, (lat, img, trj, idl, pe, ne)


def _enable(pipe, spatial, rng):
    m = pipe.transformer
    if m.is_cache_enabled:
        m.disable_cache()
    if spatial is not None:
        m.enable_cache(PyramidAttentionBroadcastConfig(spatial_attention_block_skip_range=spatial,
                                                       spatial_attention_timestep_skip_range=rng,
                                                       current_timestep_callback=lambda: pipe.current_timestep))


ARMS = {"cache off": (None, None), "cache on, computing step": (2, NEVER), "cache on, re-using step": (BIG, ALWAYS)}


def step_times(pipe, cond, rounds, steps):
    """ms per step of `steps` eager steps behind step 0 (which always computes: the state is fresh in every `denoise`)"""
    m = pipe.transformer

    def run(arm, n):
        _enable(pipe, *ARMS[arm])
        seen = []

        def cb(p, i, t, kw):                                # (a callback between steps: the loop runs eagerly)
            torch.cuda.synchronize()
            seen.append(time.perf_counter())
            return {}

        res = pipe.denoise(*cond, 6.0, n + 1, callback_on_step_end=cb)
        assert torch.isfinite(res.float()).all()
        if ARMS[arm][0] is not None:                        # the timed steps did what the arm's name says
            assert [e[3] for e in m.cache_log][1:] == [arm.endswith("computing step")] * n, m.cache_log
        return (seen[-1] - seen[0]) / n * 1e3

    for arm in ARMS:
        run(arm, 1)                                         # warm-up: every lazy cache of every arm
    t = {arm: [] for arm in ARMS}
    for _ in range(rounds):
        for arm in ARMS:
            t[arm].append(run(arm, steps))
    _enable(pipe, None, None)
    return {arm: _stats(v) for arm, v in t.items()}


def denoise_times(pipe, cond, rounds, steps=50):
    """seconds per `steps`-step clip: the uncached eager loop, the uncached graph loop, spatial 2 over (100, 800)"""
    from tests.parity import rel_rms
    m = pipe.transformer
    arms = {"cache off, eager loop": (None, None, False), "cache off, graph loop": (None, None, None),
            "spatial 2 over (100, 800), eager loop": (2, (100, 800), None)}
    t, outs, reused = {n: [] for n in arms}, {}, 0
    for _ in range(rounds):
        for name, (spatial, rng, graph) in arms.items():
            _enable(pipe, spatial, rng)
            pipe.use_hip_graph = graph
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs[name] = pipe.denoise(*cond, 6.0, steps)
            torch.cuda.synchronize()
            t[name].append(time.perf_counter() - t0)
            if spatial is not None:
                reused = sum(1 for e in m.cache_log if not e[3])
    _enable(pipe, None, None)
    pipe.use_hip_graph = None
    eager = outs["cache off, eager loop"]
    return ({n: _stats(v) for n, v in t.items()}, reused,
            rel_rms(outs["spatial 2 over (100, 800), eager loop"], eager), torch.equal(outs["cache off, graph loop"], eager))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5, help="launches per timed window")
    ap.add_argument("--steps", type=int, default=2, help="denoise steps per timed window")
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--denoise", action="store_true", help="measurement c: the 50-step clips")
    ap.add_argument("--denoise-rounds", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cog_pab_bench: needs the GPU (no CPU path, nothing is estimated)")
    lines = [f"# tools/cog_pab_bench.py on {torch.cuda.get_device_name(0)}; BASELINE config 5, L = {L}, random weights",
             "# quality on real checkpoints: NOT measured", ""]

    def flush():                                            # after every section: a later failure loses nothing measured so far
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    kl = keep_launches(a.rounds, a.reps)
    lines.append(f"a. out-projection launch, M = 2 x {L}, N = K = {D}, FINO_EPI_GATED_RESIDUAL_STAGED, bf16 output; {a.rounds} rounds of "
                 f"{a.reps} launches, alternated")
    lines.append(f"{'':52s} {'median us':>10s} {'min':>9s} {'max':>9s}")
    for fmt in ("MXFP8", "MXFP6"):
        for n, (med, lo, hi) in kl[fmt].items():
            lines.append(f"{fmt + ' ' + n:52s} {med:10.1f} {lo:9.1f} {hi:9.1f}")
        one, two, plain = (kl[fmt][k] for k in ("one launch, keep=", "two launches (EPI_NONE + residual pass)", "GEMM without keep"))
        # "not slower beyond the rounds' own spread": the one-launch median against the slowest round of the pair
        verdict = "MET" if one[0] <= two[2] else "MISSED"
        lines.append(f"{fmt}: one launch / two launches = {one[0] / two[0]:.3f} (bar: not slower than the pair beyond the rounds' spread: "
                     f"{verdict}); cost of keep over the GEMM without it: {one[0] - plain[0]:+.1f} us ({one[0] / plain[0]:.3f} x)")
    for n, (med, lo, hi) in kl["re-use"].items():
        gbs = 3 * 2 * L * D * 2 / med / 1e3                   # x and y read, out written
        lines.append(f"{n:52s} {med:10.1f} {lo:9.1f} {hi:9.1f}   {gbs:.0f} GB/s")
    lines.append("")
    flush()
    if not a.skip_steps or a.denoise:
        pipe, cond = _pipe()
        m = pipe.transformer
        layers = len(m.transformer_blocks)
        for name, fp8 in (("bf16", False), ("MXFP8 linears + fp8 attention", True)):
            if fp8:
                m.enable_mxfp8_linears()
                m.enable_fp8_attention()
            if not a.skip_steps:
                st = step_times(pipe, cond, a.step_rounds, a.steps)
                base = st["cache off"][0]
                lines.append(f"b. denoise step, {layers} layers, {name} (eager, CFG batch of 2 under one cache context); "
                             f"{a.step_rounds} rounds of {a.steps} steps, alternated")
                lines.append(f"{'':28s} {'median ms':>10s} {'min':>9s} {'max':>9s} {'ratio':>7s}")
                for n, (med, lo, hi) in st.items():
                    lines.append(f"{n:28s} {med:10.1f} {lo:9.1f} {hi:9.1f} {med / base:7.3f}")
                reuse = st["cache on, re-using step"]
                lines.append(f"a re-using step is faster than the uncached step: {'YES' if reuse[2] < st['cache off'][1] else 'NO'} "
                             f"(slowest re-using round {reuse[2]:.1f} ms, fastest uncached round {st['cache off'][1]:.1f} ms)")
                lines.append("")
                flush()
            if a.denoise:
                dn, reused, rr, same = denoise_times(pipe, cond, a.denoise_rounds)
                lines.append(f"c. 50-step denoise, {name}; {a.denoise_rounds} round(s); {reused} of 50 steps re-used the attention branch; "
                             f"graph loop torch.equal to the eager loop: {same}")
                lines.append(f"{'':40s} {'median s':>10s} {'min':>9s} {'max':>9s}")
                for n, (med, lo, hi) in dn.items():
                    lines.append(f"{n:40s} {med:10.2f} {lo:9.2f} {hi:9.2f}")
                lines.append(f"rel-RMS of the final latents, cached against uncached: {rr:.3e} (random weights: says nothing about real "
                             f"checkpoints)")
                lines.append("")
                flush()
        lines.append(f"peak device memory {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB")
    flush()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
