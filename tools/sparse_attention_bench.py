#!/usr/bin/env python3
"""Dynamic block-sparse self-attention, measured on one box in one run:

  1. the self-attention LAUNCH at the bench shape ([2, 12320, 24 x 128], 14 latent frames x 880 tokens, sinks = first frame +
     ID frame): ops.attention_tiles under per-head masks -- (a) the window_frames = 0 forced set alone, (b) the forced set plus
     random extra tiles, drawn per (batch element, head, q-block), up to densities 0.25 / 0.5 / 0.75 -- against the dense call as
     the model makes it (tail split included) and against ops.attention_ranges at window_frames = 2; time ratio next to tile
     density, the bar of section 6f: ratio <= (1 + density) / 2.  Alternated, median of the rounds, device events;
  2. the PLAN (pool + select, ops.attention_tile_plan) per call at that shape, on the same events;
  3. the whole denoise STEP of the bench workload and of the 81-frame workload (random Wan2.2-5B weights, CFG batch, eager),
     dense against cdf_threshold = 0.9, alternated, with the density the masks reached.  Random weights give a near-uniform
     pooled softmax: that density says nothing about real checkpoints.

  4. with --parent-lib PATH: the dense launch of this tree's library against another build's (the parent commit's), both loaded
     into this process, alternated.

    python tools/sparse_attention_bench.py [--rounds 7] [--steps 3] [--skip-81f] [--parent-lib PATH]
                                           [--out profiles/sparse_attention.txt]

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
from frameino_amd.window_attention import (SparseAttentionConfig, block_mask, frame_window_ranges, pack_tile_mask,  # noqa: E402
                                           ranges_density)


def _forced_keep(frames, tpf, L):
    """bool [nqb, ntall]: the window_frames = 0 forced tiles"""
    return block_mask(frame_window_ranges(frames, tpf, 0, (0, -1)), L, L)[::256, ::64]


def launch_times(rounds, reps, frames=14, tpf=880, heads=24, dh=128, densities=(0.25, 0.5, 0.75)):
    L, d, b = frames * tpf, heads * dh, 2
    g = torch.Generator(device="cuda").manual_seed(0)
    qkv = torch.randn(b, L, 3 * d, device="cuda", generator=g).bfloat16()          # the fused projection's layout
    q, k, v = qkv[:, :, :d], qkv[:, :, d:2 * d], qkv[:, :, 2 * d:]
    o = torch.empty(b, L, d, device="cuda", dtype=torch.bfloat16)
    runs, dens = {"dense": lambda: ops.attention(q, k, v, heads, out=o)}, {"dense": 1.0}
    tab = frame_window_ranges(frames, tpf, 2, (0, -1))
    dens["ranges, window_frames=2"] = ranges_density(tab, L)
    runs["ranges, window_frames=2"] = (lambda t=tab.cuda(): ops.attention_ranges(q, k, v, heads, t, out=o))
    forced = _forced_keep(frames, tpf, L)
    cg = torch.Generator().manual_seed(1)
    masks = {"tiles, forced set (window_frames=0)": forced.expand(b, heads, -1, -1)}
    for want in densities:
        f0 = float(forced.float().mean())
        extra = torch.rand(b, heads, *forced.shape, generator=cg) < (want - f0) / (1.0 - f0)
        masks[f"tiles, forced + random to {want}"] = forced | extra
    masks["tiles, full mask"] = torch.ones(b, heads, *forced.shape, dtype=torch.bool)
    for n, keep in masks.items():
        dens[n] = float(keep.float().mean())
        runs[n] = (lambda m=pack_tile_mask(keep).cuda(): ops.attention_tiles(q, k, v, heads, m, out=o))
    keep_tab = frame_window_ranges(frames, tpf, 0, (0, -1)).cuda()
    mask_out = torch.zeros(b, heads, forced.shape[0], (forced.shape[1] + 31) // 32, dtype=torch.int32, device="cuda")
    for cdf in (0.5, 0.9):
        runs[f"plan (pool + select), cdf={cdf}"] = (lambda c=cdf: ops.attention_tile_plan(q, k, heads, c, keep_ranges=keep_tab,
                                                                                         out=mask_out))
        dens[f"plan (pool + select), cdf={cdf}"] = float("nan")
    t = {n: [] for n in runs}
    for f in runs.values():
        f(), f()
    torch.cuda.synchronize()
    for n in dens:
        if n.startswith("plan"):
            runs[n]()
            dens[n] = ops.tile_mask_density(mask_out, L)                           # what the plan kept on these N(0, 1) inputs
    for _ in range(rounds):
        for n, f in runs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(reps):
                f()
            e.record()
            torch.cuda.synchronize()
            t[n].append(s.elapsed_time(e) / reps * 1e3)
    return {n: (statistics.median(t[n]), min(t[n]), max(t[n]), dens[n]) for n in runs}


def parent_ab(path, rounds, reps, frames=14, tpf=880, heads=24, dh=128):
    """the dense self-attention launch (ops.attention's call, tail split included) through this tree's library and through the
    one at `path` (the parent commit's build), both loaded into this process, alternated"""
    import ctypes
    from frameino_amd import _lib
    L, d, b = frames * tpf, heads * dh, 2
    g = torch.Generator(device="cuda").manual_seed(0)
    qkv = torch.randn(b, L, 3 * d, device="cuda", generator=g).bfloat16()
    q, k, v = qkv[:, :, :d], qkv[:, :, d:2 * d], qkv[:, :, 2 * d:]
    outs = {"this tree": torch.empty(b, L, d, device="cuda", dtype=torch.bfloat16)}
    outs["parent"] = torch.empty_like(outs["this tree"])
    other = ctypes.CDLL(path)                               # (an older build lacks newer symbols: bind the three used here only)
    for name in ("fino_attn_workspace_bytes", "fino_attn_fwd_ws", "fino_last_error"):
        getattr(other, name).argtypes = _lib.SIGNATURES.get(name)
        getattr(other, name).restype = getattr(_lib.lib(), name).restype
    libs = {"this tree": _lib.lib(), "parent": other}
    need = libs["this tree"].fino_attn_workspace_bytes(b, heads, L, L, dh)
    assert need == libs["parent"].fino_attn_workspace_bytes(b, heads, L, L, dh)
    ws = torch.empty(max(need, 16) // 4, dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(n):
        o = outs[n]
        rc = libs[n].fino_attn_fwd_ws(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), b, heads, L, L, dh, q.stride(0),
                                      q.stride(1), dh, k.stride(0), k.stride(1), dh, v.stride(0), v.stride(1), dh, o.stride(0),
                                      o.stride(1), dh, ctypes.c_float(dh ** -0.5), 0, ws.data_ptr(), need, st)
        assert rc == 0, libs[n].fino_last_error()

    t = {n: [] for n in libs}
    for n in libs:
        call(n), call(n)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for n in libs:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(reps):
                call(n)
            e.record()
            torch.cuda.synchronize()
            t[n].append(s.elapsed_time(e) / reps * 1e3)
    return {n: (statistics.median(v), min(v), max(v)) for n, v in t.items()}, torch.equal(outs["this tree"], outs["parent"])


def step_times(workload, rounds, steps, cdf):
    import bench
    from frameino_amd.pipeline_wan_i2v_motion_frameino import WanImageToVideoPipeline
    from frameino_amd.schedulers import FlowMatchEulerDiscreteScheduler
    from frameino_amd.configs import WAN22_5B_CFG
    cfg, dev = dict(WAN22_5B_CFG), torch.device("cuda")
    fg, lh, lw = bench.WORKLOADS[workload]
    C, nid = cfg["out_channels"], 1
    model = bench.build_model(cfg, dev)
    pipe = WanImageToVideoPipeline(scheduler=FlowMatchEulerDiscreteScheduler(shift=5.0), transformer=model, expand_timesteps=True)
    g = torch.Generator().manual_seed(1234)
    rnd = lambda *s: torch.randn(*s, generator=g)          # noqa: E731
    lat, cond, traj, idl = rnd(1, C, fg, lh, lw), rnd(1, C, 1, lh, lw), rnd(1, C, fg + nid, lh, lw), rnd(1, C, nid, lh, lw)
    traj[:, :, fg:] = 0
    mask = torch.ones(1, 1, fg, lh, lw)
    mask[:, :, 0] = 0
    pe, ne = rnd(1, 512, cfg["text_dim"]), rnd(1, 512, cfg["text_dim"])
    pe[:, 64:], ne[:, 8:] = 0, 0
    pipe.scheduler.set_timesteps(8, device=dev)
    st = pipe.make_state(lat.to(dev), cond.to(dev), traj.to(dev), idl.to(dev), mask.to(dev), pe.to(dev).bfloat16(),
                         ne.to(dev).bfloat16(), 5.0)
    ts, dts, lat0 = pipe.scheduler.timesteps.to(dev).float(), pipe.scheduler.dts.to(dev), st.lat.clone()

    def run(sparse, n, keep_masks=False):
        model.disable_sparse_attention()
        if sparse:
            model.enable_sparse_attention(SparseAttentionConfig(cdf_threshold=cdf, window_frames=0, sink_frames=(0,),
                                                                keep_masks=keep_masks))
        st.lat.copy_(lat0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            for i in range(n):
                st.t_rows[1:2].copy_(ts[i:i + 1])
                st.dt.copy_(dts[i:i + 1])
                pipe._step(st)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    run(False, 1), run(True, 1, keep_masks=True)                          # warm-up: every lazy cache of both paths ...
    per_layer = model.sparse_attention_density()                          # ... and the density of the first step's masks
    dens = sum(per_layer.values()) / len(per_layer)
    t = {"dense": [], f"cdf_threshold={cdf}": []}
    for _ in range(rounds):
        t["dense"].append(run(False, steps))
        t[f"cdf_threshold={cdf}"].append(run(True, steps))
    frames, tpf = fg + nid, (lh // 2) * (lw // 2)
    forced = ranges_density(frame_window_ranges(frames, tpf, 0, (0, -1)), frames * tpf)
    del model, pipe, st
    torch.cuda.empty_cache()
    return ({n: (statistics.median(v), min(v), max(v)) for n, v in t.items()}, dens, min(per_layer.values()),
            max(per_layer.values()), forced, frames, tpf)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5, help="launches per timed window")
    ap.add_argument("--steps", type=int, default=3, help="denoise steps per timed window")
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--cdf", type=float, default=0.9)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--skip-81f", action="store_true")
    ap.add_argument("--parent-lib", default=None, help="another build of libframeino_hip.so to alternate the dense launch with")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sparse_attention_bench: needs the GPU (no CPU path, nothing is estimated)")
    lines = [f"# tools/sparse_attention_bench.py on {torch.cuda.get_device_name(0)}; bf16; one box, one run",
             "# forced tiles: own frame(s), first frame, ID frame (window_frames = 0); extra tiles: random per (b, head, q-block)",
             "# quality on real checkpoints: NOT measured (random weights only)", ""]
    lt = launch_times(a.rounds, a.reps)
    base = lt["dense"][0]
    lines.append("self-attention launch, [2, 12320, 24 x 128] (14 frames x 880 tokens, 49 q-blocks x 193 key tiles)")
    lines.append(f"{'':40s} {'median us':>10s} {'min':>9s} {'max':>9s} {'ratio':>7s} {'density':>8s} {'(1+density)/2':>14s}")
    for n, (med, lo, hi, dens) in lt.items():
        lines.append(f"{n:40s} {med:10.1f} {lo:9.1f} {hi:9.1f} {med / base:7.3f} {dens:8.3f} {(1 + dens) / 2:14.3f}")
    lines.append("(plan rows: the density column is what the plan kept on these N(0, 1) inputs; no bar applies to them)")
    if a.parent_lib:
        ab, same = parent_ab(a.parent_lib, 9, a.reps)
        lines.append("")
        lines.append(f"dense launch, this tree's library against the parent commit's (one process, alternated, 9 rounds x {a.reps} "
                     f"launches); outputs torch.equal: {same}")
        lines.append(f"{'':28s} {'median us':>10s} {'min':>9s} {'max':>9s}")
        for n, (med, lo, hi) in ab.items():
            lines.append(f"{n:28s} {med:10.1f} {lo:9.1f} {hi:9.1f}")
    if not a.skip_steps:
        for wl in ["wan2.2-5b-49f-704x1280"] + ([] if a.skip_81f else ["wan2.2-5b-81f-704x1280"]):
            stt, dens, dlo, dhi, forced, frames, tpf = step_times(wl, a.step_rounds, a.steps, a.cdf)
            base = stt["dense"][0]
            lines.append("")
            lines.append(f"denoise step, {wl} ({frames} latent frames x {tpf} tokens; eager, CFG batch; mask density of the first "
                         f"step: mean {dens:.3f}, layers {dlo:.3f} .. {dhi:.3f}; forced tiles alone {forced:.3f})")
            lines.append("(random weights: a near-uniform pooled softmax -- this density says nothing about real checkpoints)")
            lines.append(f"{'':28s} {'median ms':>10s} {'min':>9s} {'max':>9s} {'ratio':>7s}")
            for n, (med, lo, hi) in stt.items():
                lines.append(f"{n:28s} {med:10.1f} {lo:9.1f} {hi:9.1f} {med / base:7.3f}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
