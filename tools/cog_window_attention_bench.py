#!/usr/bin/env python3
"""Sliding-window self-attention over frames on the CogVideoX-5B FrameINO backbone, measured on one box in
one run, with the method of tools/window_attention_bench.py (device events for launches, a host clock around synchronised steps,
dense and windowed alternated, medians):

  1. the joint self-attention LAUNCH at BASELINE config 5 ([2, 19126, 48 x 64]: 226 text rows + 14 latent frames x 1350 tokens,
     sinks = first frame + ID frame): the dense call as the model makes it against the ranges launch at window_frames 1, 2, 3 and
     over the full table -- once for bf16 (ops.attention / ops.attention_ranges), once for fp8 (ops.attention_fp8 /
     ops.attention_fp8_ranges); every ratio against the dense launch of the same operand type;
  2. the config-5 denoise STEP (random weights, CFG batch, eager), dense against window_frames = 2, in bf16 and with MXFP8 linears
     + fp8 attention;
  3. with --parent-lib PATH: the dense fp8 launch of this tree's library against another build's (the parent commit's), both
     loaded into this process, the same call alternated; outputs compared bit for bit.

    python tools/cog_window_attention_bench.py [--rounds 7] [--steps 2] [--parent-lib PATH] [--out profiles/cog_window_attention.txt]

Quality on real checkpoints is NOT measured here or anywhere in this repository (random weights only)."""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from frameino_amd import _lib, ops  # noqa: E402
from frameino_amd.window_attention import WindowAttentionConfig, frame_window_ranges, ranges_density  # noqa: E402

FRAMES, TPF, TEXT, HEADS, DH = 14, 1350, 226, 48, 64
L = TEXT + FRAMES * TPF


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
    return {n: (statistics.median(v), min(v), max(v)) for n, v in t.items()}


def _qkv():
    d = HEADS * DH
    g = torch.Generator(device="cuda").manual_seed(0)
    qkv = torch.randn(2, L, 3 * d, device="cuda", generator=g).bfloat16()          # the fused projection's layout
    return qkv[:, :, :d], qkv[:, :, d:2 * d], qkv[:, :, 2 * d:], torch.empty(2, L, d, device="cuda", dtype=torch.bfloat16)


def launch_times(rounds, reps, fp8, windows=(1, 2, 3)):
    q, k, v, o = _qkv()
    dense = (lambda: ops.attention_fp8(q, k, v, HEADS, out=o)) if fp8 else (lambda: ops.attention(q, k, v, HEADS, out=o))
    walk = ops.attention_fp8_ranges if fp8 else ops.attention_ranges
    runs, dens = {"dense": dense}, {"dense": 1.0}
    for w in windows:
        tab = frame_window_ranges(FRAMES, TPF, w, (0, -1), prefix_rows=TEXT)
        dens[f"window_frames={w}"] = ranges_density(tab, L)
        runs[f"window_frames={w}"] = (lambda t=tab.cuda(): walk(q, k, v, HEADS, t, out=o))
    full = frame_window_ranges(FRAMES, TPF, FRAMES, (0, -1), prefix_rows=TEXT)
    dens["ranges, full table"] = ranges_density(full, L)                           # what the kernel change itself costs
    runs["ranges, full table"] = (lambda t=full.cuda(): walk(q, k, v, HEADS, t, out=o))
    return {n: r + (dens[n],) for n, r in _alternate(runs, rounds, reps).items()}


def step_times(rounds, steps, window):
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
    wcfg = WindowAttentionConfig(window_frames=window, sink_frames=(0,))

    def run(windowed, n):
        m.disable_window_attention()
        if windowed:
            m.enable_window_attention(wcfg)
        seen = []

        def cb(p, i, t, kw):                                # (a callback between steps: the loop runs eagerly)
            torch.cuda.synchronize()
            seen.append(time.perf_counter())
            return {}

        res = pipe.denoise(lat, img, trj, idl, pe, ne, 6.0, n + 1, callback_on_step_end=cb)
        assert torch.isfinite(res.float()).all()
        return (seen[-1] - seen[0]) / n * 1e3

    out = {}
    for name, fp8 in (("bf16", False), ("MXFP8 linears + fp8 attention", True)):
        if fp8:
            m.enable_mxfp8_linears()
            m.enable_fp8_attention()
        run(False, 1), run(True, 1)                         # warm-up: every lazy cache of both paths
        t = {"dense": [], f"window_frames={window}": []}
        for _ in range(rounds):
            t["dense"].append(run(False, steps))
            t[f"window_frames={window}"].append(run(True, steps))
        out[name] = {n: (statistics.median(v), min(v), max(v)) for n, v in t.items()}
    layers = len(m.transformer_blocks)
    del m, pipe
    torch.cuda.empty_cache()
    return out, layers


def parent_ab(path, rounds, reps):
    """the dense fp8 launch (default kernel, default p_mode) through this tree's library and through the one at `path`"""
    q, k, v, o = _qkv()
    o2 = torch.empty_like(o)
    other = ctypes.CDLL(path)                               # (an older build lacks newer symbols: bind the two used here only)
    for name in ("fino_attn_fp8_kv_bytes", "fino_attn_fwd_fp8", "fino_last_error"):
        getattr(other, name).argtypes = _lib.SIGNATURES.get(name)
        getattr(other, name).restype = getattr(_lib.lib(), name).restype
    libs = {"this tree": _lib.lib(), "parent": other}
    need = libs["this tree"].fino_attn_fp8_kv_bytes(2, HEADS, L, DH)
    assert need == libs["parent"].fino_attn_fp8_kv_bytes(2, HEADS, L, DH)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(lib, out):
        rc = lib.fino_attn_fwd_fp8(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), 2, HEADS, L, L, DH, q.stride(0),
                                   q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1), out.stride(0), out.stride(1),
                                   ctypes.c_float(DH ** -0.5), 0, ops.FP8_P_DEFAULT, ws.data_ptr(), need, st)
        assert rc == 0, lib.fino_last_error()

    res = _alternate({"this tree": lambda: call(libs["this tree"], o), "parent": lambda: call(libs["parent"], o2)}, rounds, reps)
    torch.cuda.synchronize()
    return res, torch.equal(o, o2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5, help="launches per timed window")
    ap.add_argument("--steps", type=int, default=2, help="denoise steps per timed window")
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--parent-lib", default=None, help="another build of libframeino_hip.so to alternate the dense fp8 launch with")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cog_window_attention_bench: needs the GPU (no CPU path, nothing is estimated)")
    lines = [f"# tools/cog_window_attention_bench.py on {torch.cuda.get_device_name(0)}; sinks = first frame + ID frame",
             "# quality on real checkpoints: NOT measured (random weights only)", ""]

    def flush():                                            # after every section: a later failure loses nothing measured so far
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    launch = {}
    for name, fp8 in (("bf16 (dense: ops.attention, the default kernel; ranges: attn_ppd_kernel<T, 64, 2>)", False),
                      ("fp8 (dense: ops.attention_fp8, free-running kernel; ranges: its range walk)", True)):
        lt = launch[fp8] = launch_times(a.rounds, a.reps, fp8)
        base = lt["dense"][0]
        lines.append(f"self-attention launch, [2, {L}, {HEADS} x {DH}] ({TEXT} text rows + {FRAMES} frames x {TPF} tokens, 75 q-blocks x "
                     f"299 key tiles), {name}")
        lines.append(f"{'':28s} {'median us':>10s} {'min':>9s} {'max':>9s} {'ratio':>7s} {'density':>8s} {'(1+density)/2':>14s}")
        for n, (med, lo, hi, dens) in lt.items():
            lines.append(f"{n:28s} {med:10.1f} {lo:9.1f} {hi:9.1f} {med / base:7.3f} {dens:8.3f} {(1 + dens) / 2:14.3f}")
        lines.append("")
        flush()
    med, _, _, dens = launch[True]["window_frames=2"]
    ratio = med / launch[True]["dense"][0]
    lines.append(f"bar for the fp8 range walk at window_frames = 2: ratio {ratio:.3f} <= (1 + density) / 2 = {(1 + dens) / 2:.3f}: "
                 f"{'MET' if ratio <= (1 + dens) / 2 else 'MISSED'}")
    if not a.skip_steps:
        stt, layers = step_times(a.step_rounds, a.steps, 2)
        for (name, res), fp8 in zip(stt.items(), (False, True)):
            base = res["dense"][0]
            lines.append("")
            lines.append(f"denoise step, BASELINE config 5 [2, 14, 48, 60, 90], {layers} layers, {name} (eager, CFG batch)")
            lines.append(f"{'':28s} {'median ms':>10s} {'min':>9s} {'max':>9s} {'ratio':>7s}")
            for n, (med, lo, hi) in res.items():
                lines.append(f"{n:28s} {med:10.1f} {lo:9.1f} {hi:9.1f} {med / base:7.3f}")
            lt = launch[fp8]
            lines.append(f"step loss {base - res['window_frames=2'][0]:.1f} ms; {layers} x the launch difference = "
                         f"{layers * (lt['dense'][0] - lt['window_frames=2'][0]) / 1e3:.1f} ms")
    flush()
    if a.parent_lib:
        res, same = parent_ab(a.parent_lib, a.rounds, a.reps)
        lines.append("")
        lines.append(f"dense fp8 launch, this tree's library against {os.path.basename(a.parent_lib)} (one process, alternated): outputs "
                     f"torch.equal: {same}")
        lines.append(f"{'':28s} {'median us':>10s} {'min':>9s} {'max':>9s}")
        for n, (med, lo, hi) in res.items():
            lines.append(f"{n:28s} {med:10.1f} {lo:9.1f} {hi:9.1f}")
    flush()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
