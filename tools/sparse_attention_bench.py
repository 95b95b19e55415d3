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

  5. with --gate (nothing of 1 - 4 is run): the PLAN per call at the bench shape through the old entry,
     with the similarity gate (a theta nothing falls under, so that every q-block runs the whole select, and one everything
     falls under), with a per-head table, and with both -- alternated in one run; with --parent-lib the old entry of this
     tree's library against the parent commit's, masks compared; and the bench STEP dense / cdf_threshold 0.9 / cdf_threshold
     0.9 + similarity_threshold, with the share of q-blocks and key tiles the gate fired on.

  6. with --fp8 (nothing of 1 - 5 is run): the LAUNCH table of 1 on the fp8 operands -- ops.attention_fp8 dense
     (tail split included) against ops.attention_fp8_tiles over the same scattered masks and the full mask, the same bar; with
     --parent-lib the dense fp8 launch (fino_attn_fwd_fp8) of this tree's library against the parent commit's, outputs compared;
     and the bench STEP with MXFP8 linears + fp8 attention, dense against cdf_threshold = 0.9 (random weights: no bar).

    python tools/sparse_attention_bench.py [--rounds 7] [--steps 3] [--skip-81f] [--parent-lib PATH]
                                           [--out profiles/sparse_attention.txt]
    python tools/sparse_attention_bench.py --gate [--theta 0.3] [--parent-lib PATH] [--out profiles/sparse_attention_gate.txt]
    python tools/sparse_attention_bench.py --fp8 [--parent-lib PATH] [--out profiles/sparse_attention_fp8.txt]

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


def _scattered_masks(forced, b, heads, densities):
    """the masks of the launch tables: the forced set alone, the forced set + random extra tiles per (batch element, head, q-block)
    up to each density, the full mask"""
    cg = torch.Generator().manual_seed(1)
    masks = {"tiles, forced set (window_frames=0)": forced.expand(b, heads, -1, -1)}
    for want in densities:
        f0 = float(forced.float().mean())
        extra = torch.rand(b, heads, *forced.shape, generator=cg) < (want - f0) / (1.0 - f0)
        masks[f"tiles, forced + random to {want}"] = forced | extra
    masks["tiles, full mask"] = torch.ones(b, heads, *forced.shape, dtype=torch.bool)
    return masks


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
    masks = _scattered_masks(forced, b, heads, densities)
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


def fp8_launch_times(rounds, reps, frames=14, tpf=880, heads=24, dh=128, densities=(0.25, 0.5, 0.75)):
    """the launch table on the fp8 operands: ops.attention_fp8 dense (as the model calls it: pre-pass, tail split and combine
    included) and ops.attention_fp8_tiles (the same pre-pass, whole blocks) over the scattered masks of launch_times"""
    L, d, b = frames * tpf, heads * dh, 2
    g = torch.Generator(device="cuda").manual_seed(0)
    qkv = torch.randn(b, L, 3 * d, device="cuda", generator=g).bfloat16()
    q, k, v = qkv[:, :, :d], qkv[:, :, d:2 * d], qkv[:, :, 2 * d:]
    o = torch.empty(b, L, d, device="cuda", dtype=torch.bfloat16)
    runs, dens = {"dense fp8": lambda: ops.attention_fp8(q, k, v, heads, out=o)}, {"dense fp8": 1.0}
    for n, keep in _scattered_masks(_forced_keep(frames, tpf, L), b, heads, densities).items():
        dens[n] = float(keep.float().mean())
        runs[n] = (lambda m=pack_tile_mask(keep).cuda(): ops.attention_fp8_tiles(q, k, v, heads, m, out=o))
    t = _median_us(runs, rounds, reps)
    return {n: t[n] + (dens[n],) for n in runs}


def fp8_parent_ab(path, rounds, reps, frames=14, tpf=880, heads=24, dh=128):
    """the dense fp8 self-attention launch (fino_attn_fwd_fp8 with the default p_mode) through this tree's library and through the
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
    for name in ("fino_attn_fp8_kv_bytes", "fino_attn_fwd_fp8", "fino_last_error"):
        getattr(other, name).argtypes = _lib.SIGNATURES.get(name)
        getattr(other, name).restype = getattr(_lib.lib(), name).restype
    libs = {"this tree": _lib.lib(), "parent": other}
    need = libs["this tree"].fino_attn_fp8_kv_bytes(b, heads, L, dh)
    assert need == libs["parent"].fino_attn_fp8_kv_bytes(b, heads, L, dh)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(n):
        o = outs[n]
        rc = libs[n].fino_attn_fwd_fp8(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), b, heads, L, L, dh, q.stride(0),
                                       q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1), o.stride(0), o.stride(1),
                                       ctypes.c_float(dh ** -0.5), 0, ops.FP8_P_DEFAULT, ws.data_ptr(), need, st)
        assert rc == 0, libs[n].fino_last_error()

    t = _median_us({n: (lambda n=n: call(n)) for n in libs}, rounds, reps)
    return t, torch.equal(outs["this tree"], outs["parent"])


def _median_us(runs, rounds, reps):
    """{name: callable} -> {name: (median, min, max)} in us per call; alternated, device events"""
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


def gate_plan_times(rounds, reps, theta, parent_lib=None, frames=14, tpf=880, heads=24, dh=128, cdf=0.9):
    """the plan per call: old entry / gated / per-head table / both, and (parent_lib) the old entry of the parent's library"""
    import ctypes
    from frameino_amd import _lib
    L, d, b = frames * tpf, heads * dh, 2
    g = torch.Generator(device="cuda").manual_seed(0)
    qkv = torch.randn(b, L, 3 * d, device="cuda", generator=g).bfloat16()
    q, k = qkv[:, :, :d], qkv[:, :, d:2 * d]
    keep_tab = frame_window_ranges(frames, tpf, 0, (0, -1)).cuda()
    nqb, nt = -(-L // 256), -(-L // 64)
    new_mask = lambda: torch.zeros(b, heads, nqb, (nt + 31) // 32, dtype=torch.int32, device="cuda")          # noqa: E731
    ws = torch.empty(ops.attention_tile_plan_gated_bytes(b, heads, L, L, dh) // 4, dtype=torch.float32, device="cuda")
    table = torch.full((heads,), cdf, dtype=torch.float32, device="cuda")
    table[::2] = 0.5
    never = 1e-6                # N(0, 1) rows: similarity ~ 1 / n = 0.004 (q-blocks), 0.016 (key tiles) -- nothing falls under this
    names = {"ungated (old entry)": {}, f"gated, theta={never} (fires nowhere)": dict(similarity_threshold=never),
             f"gated, theta={theta} (fires everywhere)": dict(similarity_threshold=theta),
             "per-head table, no gate": dict(cdf_heads=table),
             f"gated, theta={never} + per-head table": dict(similarity_threshold=never, cdf_heads=table)}
    masks = {n: new_mask() for n in names}
    runs = {n: (lambda kw=kw, m=masks[n]: ops.attention_tile_plan(q, k, heads, cdf, keep_ranges=keep_tab, out=m, workspace=ws, **kw))
            for n, kw in names.items()}
    same = None
    if parent_lib:
        other = ctypes.CDLL(parent_lib)
        for name in ("fino_attn_tile_plan", "fino_last_error"):
            getattr(other, name).argtypes = _lib.SIGNATURES.get(name)
            getattr(other, name).restype = getattr(_lib.lib(), name).restype
        st = torch.cuda.current_stream().cuda_stream

        def raw(lib, m):                    # the C entry itself, for both libraries: no front-end work between the launches
            rc = lib.fino_attn_tile_plan(q.data_ptr(), k.data_ptr(), b, heads, L, L, dh, q.stride(0), q.stride(1), dh, k.stride(0),
                                         k.stride(1), dh, dh ** -0.5, 0, cdf, keep_tab.data_ptr(), m.data_ptr(), m.shape[3],
                                         ws.data_ptr(), ws.numel() * 4, st)
            assert rc == 0, lib.fino_last_error()

        for n, lib in (("ungated, C entry, this tree's library", _lib.lib()), ("ungated, C entry, parent commit's library", other)):
            masks[n] = new_mask()
            runs[n] = (lambda lib=lib, m=masks[n]: raw(lib, m))
    t = _median_us(runs, rounds, reps)
    if parent_lib:
        same = torch.equal(masks["ungated, C entry, this tree's library"], masks["ungated, C entry, parent commit's library"]) and \
            torch.equal(masks["ungated (old entry)"], masks["ungated, C entry, parent commit's library"])
    gate_off_same = torch.equal(masks["ungated (old entry)"], masks[f"gated, theta={never} (fires nowhere)"])
    dens = {n: ops.tile_mask_density(m, L) for n, m in masks.items()}
    return t, dens, same, gate_off_same


def step_times(workload, rounds, steps, cdf, theta=None, fp8=False):
    import bench
    from frameino_amd.pipeline_wan_i2v_motion_frameino import WanImageToVideoPipeline
    from frameino_amd.schedulers import FlowMatchEulerDiscreteScheduler
    from frameino_amd.configs import WAN22_5B_CFG
    cfg, dev = dict(WAN22_5B_CFG), torch.device("cuda")
    fg, lh, lw = bench.WORKLOADS[workload]
    C, nid = cfg["out_channels"], 1
    model = bench.build_model(cfg, dev)
    if fp8:                                                               # the precision path: MXFP8 linears + fp8 attention operands
        model.enable_mxfp8_linears()
        model.enable_fp8_attention()
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

    def run(sparse, n, keep_masks=False, similarity=None):
        model.disable_sparse_attention()
        if sparse:
            model.enable_sparse_attention(SparseAttentionConfig(cdf_threshold=cdf, window_frames=0, sink_frames=(0,),
                                                                keep_masks=keep_masks, similarity_threshold=similarity))
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
    gate = None
    if theta is not None:                                                 # the gate's first step: what it fired on, what was kept
        run(True, 1, keep_masks=True, similarity=theta)
        sims, gd = model.sparse_attention_similarity(), model.sparse_attention_density()
        gate = {"density": sum(gd.values()) / len(gd), "sim_q": sum(v[0] for v in sims.values()) / len(sims),
                "sim_k": sum(v[1] for v in sims.values()) / len(sims), "q_fired": sum(v[2] for v in sims.values()) / len(sims),
                "k_fired": sum(v[3] for v in sims.values()) / len(sims)}
        t[f"cdf_threshold={cdf}, similarity_threshold={theta}"] = []
    for _ in range(rounds):
        t["dense"].append(run(False, steps))
        t[f"cdf_threshold={cdf}"].append(run(True, steps))
        if theta is not None:
            t[f"cdf_threshold={cdf}, similarity_threshold={theta}"].append(run(True, steps, similarity=theta))
    frames, tpf = fg + nid, (lh // 2) * (lw // 2)
    forced = ranges_density(frame_window_ranges(frames, tpf, 0, (0, -1)), frames * tpf)
    del model, pipe, st
    torch.cuda.empty_cache()
    out = ({n: (statistics.median(v), min(v), max(v)) for n, v in t.items()}, dens, min(per_layer.values()),
           max(per_layer.values()), forced, frames, tpf)
    return out if theta is None else out + (gate,)


def gate_report(a):
    lines = [f"# tools/sparse_attention_bench.py --gate on {torch.cuda.get_device_name(0)}; bf16; one box, one run",
             "# the similarity gate and the per-head thresholds of the sparse attention (DESIGN.md section 6k)",
             "# quality on real checkpoints: NOT measured (random weights and N(0, 1) inputs only: what the gate fires on here says",
             "# nothing about a real checkpoint)", ""]
    t, dens, same, gate_off_same = gate_plan_times(a.rounds, a.reps, a.theta, a.parent_lib, cdf=a.cdf)
    base = t["ungated (old entry)"]
    lines.append(f"plan (pool + select) per call, [2, 12320, 24 x 128], cdf = {a.cdf}; alternated, {a.rounds} rounds x {a.reps} calls")
    lines.append(f"{'':46s} {'median us':>10s} {'min':>9s} {'max':>9s} {'vs ungated':>11s} {'density':>8s}")
    for n, (med, lo, hi) in t.items():
        lines.append(f"{n:46s} {med:10.1f} {lo:9.1f} {hi:9.1f} {med / base[0]:11.3f} {dens[n]:8.3f}")
    lines.append(f"run-to-run spread of the ungated plan in this run: {base[2] - base[1]:.1f} us ({(base[2] - base[1]) / base[0] * 100:.1f} % "
                 f"of its median)")
    lines.append(f"mask of the gated entry with a theta nothing falls under == mask of the old entry: {gate_off_same}")
    if same is not None:
        own, par = t["ungated, C entry, this tree's library"], t["ungated, C entry, parent commit's library"]
        lines.append(f"ungated plan through the C entry, this tree against the parent commit's library: {own[0]:.1f} vs {par[0]:.1f} us "
                     f"(difference {own[0] - par[0]:+.1f} us; spread of the two {own[2] - own[1]:.1f} / {par[2] - par[1]:.1f} us); masks "
                     f"torch.equal: {same}")
        lines.append("(the rows above it go through ops.attention_tile_plan, whose argument checks sit between the launches)")
    worst = max(v[0] for n, v in t.items() if n.startswith("gated"))
    lines.append(f"the tile walk saves 320 us per launch at density 0.9 (profiles/sparse_attention.txt: 3222.9 dense, density x "
                 f"1.067 x dense walked); the costliest gated plan takes {worst:.1f} us of that, the ungated plan {base[0]:.1f} us")
    if not a.skip_steps:
        wl = "wan2.2-5b-49f-704x1280"
        stt, d0, dlo, dhi, forced, frames, tpf, gate = step_times(wl, a.step_rounds, a.steps, a.cdf, a.theta)
        b0 = stt["dense"][0]
        lines.append("")
        lines.append(f"denoise step, {wl} ({frames} latent frames x {tpf} tokens; eager, CFG batch); first step's mask density "
                     f"{d0:.3f} without the gate, {gate['density']:.3f} with similarity_threshold = {a.theta}")
        lines.append(f"the gate on that step: mean sim_q {gate['sim_q']:.3f}, mean sim_k {gate['sim_k']:.3f}; it fired on "
                     f"{gate['q_fired'] * 100:.1f} % of the q-blocks and {gate['k_fired'] * 100:.1f} % of the key tiles (means over the layers)")
        lines.append("(random weights: these shares and densities say nothing about real checkpoints)")
        lines.append(f"{'':48s} {'median ms':>10s} {'min':>9s} {'max':>9s} {'ratio':>7s}")
        for n, (med, lo, hi) in stt.items():
            lines.append(f"{n:48s} {med:10.1f} {lo:9.1f} {hi:9.1f} {med / b0:7.3f}")
    return lines


def fp8_report(a):
    lines = [f"# tools/sparse_attention_bench.py --fp8 on {torch.cuda.get_device_name(0)}; bf16 storage, fp8 (e4m3) attention "
             f"operands; one box, one run",
             "# block-sparse fp8 self-attention (DESIGN.md section 6m): ops.attention_fp8_tiles against ops.attention_fp8",
             "# forced tiles: own frame(s), first frame, ID frame (window_frames = 0); extra tiles: random per (b, head, q-block)",
             "# quality on real checkpoints: NOT measured (random weights and N(0, 1) inputs only)", ""]
    lt = fp8_launch_times(a.rounds, a.reps)
    base = lt["dense fp8"][0]
    lines.append("fp8 self-attention launch (K / V pre-pass included in every row), [2, 12320, 24 x 128] (14 frames x 880 tokens, 49 "
                 "q-blocks x 193 key tiles)")
    lines.append(f"{'':40s} {'median us':>10s} {'min':>9s} {'max':>9s} {'ratio':>7s} {'density':>8s} {'(1+density)/2':>14s} {'bar':>5s}")
    for n, (med, lo, hi, dens) in lt.items():
        bar = "" if n == "dense fp8" else ("met" if med / base <= (1 + dens) / 2 else "MISS")
        lines.append(f"{n:40s} {med:10.1f} {lo:9.1f} {hi:9.1f} {med / base:7.3f} {dens:8.3f} {(1 + dens) / 2:14.3f} {bar:>5s}")
    if a.parent_lib:
        ab, same = fp8_parent_ab(a.parent_lib, 9, a.reps)
        lines.append("")
        lines.append(f"dense fp8 launch (fino_attn_fwd_fp8), this tree's library against the parent commit's (one process, alternated, "
                     f"9 rounds x {a.reps} launches); outputs torch.equal: {same}")
        lines.append(f"{'':28s} {'median us':>10s} {'min':>9s} {'max':>9s}")
        for n, (med, lo, hi) in ab.items():
            lines.append(f"{n:28s} {med:10.1f} {lo:9.1f} {hi:9.1f}")
    if not a.skip_steps:
        wl = "wan2.2-5b-49f-704x1280"
        stt, dens, dlo, dhi, forced, frames, tpf = step_times(wl, a.step_rounds, a.steps, a.cdf, fp8=True)
        base = stt["dense"][0]
        lines.append("")
        lines.append(f"denoise step, {wl}, MXFP8 linears + fp8 attention ({frames} latent frames x {tpf} tokens; eager, CFG batch; mask "
                     f"density of the first step: mean {dens:.3f}, layers {dlo:.3f} .. {dhi:.3f}; forced tiles alone {forced:.3f})")
        lines.append("(random weights: a near-uniform pooled softmax -- this density says nothing about real checkpoints; no bar applies)")
        lines.append(f"{'':28s} {'median ms':>10s} {'min':>9s} {'max':>9s} {'ratio':>7s}")
        for n, (med, lo, hi) in stt.items():
            lines.append(f"{n:28s} {med:10.1f} {lo:9.1f} {hi:9.1f} {med / base:7.3f}")
    return lines


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
    ap.add_argument("--gate", action="store_true", help="measure the similarity gate and the per-head table only (section 6k)")
    ap.add_argument("--theta", type=float, default=0.3, help="with --gate: the similarity threshold")
    ap.add_argument("--fp8", action="store_true", help="measure the block-sparse fp8 self-attention only (section 6m)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sparse_attention_bench: needs the GPU (no CPU path, nothing is estimated)")
    if a.gate or a.fp8:
        text = "\n".join(gate_report(a) if a.gate else fp8_report(a)) + "\n"
        print(text)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text)
        return
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
