#!/usr/bin/env python3
"""The full-size Wan2.2-5B denoise step (bench.py's workload: 49 frames 704 x 1280, batch-2 CFG, eager) in bf16, with MXFP8
linears, with MXFP6 linears and with MXFP6 linears on rotated blocks (`enable_mxfp6_linears(rotate=True)`), in one process on
one box: the precisions alternated, the sequence run `--reps` times, device events around `steps` steps after `warmup`, plus the
in-run matrix peak (fino_diag_mfma_peak) so boxes can be compared.  With --parent-lib PATH the unrotated MXFP6 step also runs on
another build of the library (the parent commit's), alternated with the rest: the rotation must not have moved it.
Usage: mxfp6_step_bench.py [--steps 6] [--warmup 2] [--layers N] [--parent-lib PATH] > profiles/mxfp6_step.txt"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--layers", type=int, default=None, help="fewer layers (a quick look; not the step)")
    ap.add_argument("--only", default=None, choices=["bf16", "mxfp8", "mxfp6", "mxfp6-rot"], help="one precision (for a kernel trace)")
    ap.add_argument("--parent-lib", default=None, help="another build of libframeino_hip.so: the unrotated MXFP6 step runs on it too")
    a = ap.parse_args()
    from frameino_amd import _lib
    from frameino_amd.configs import WAN22_5B_CFG
    from frameino_amd.pipeline_wan_i2v_motion_frameino import WanImageToVideoPipeline
    from frameino_amd.schedulers import FlowMatchEulerDiscreteScheduler
    dev = torch.device("cuda", 0)
    cfg = dict(WAN22_5B_CFG)
    if a.layers:
        cfg["num_layers"] = a.layers
    fg, lh, lw = bench.WORKLOADS["wan2.2-5b-49f-704x1280"]
    C = cfg["out_channels"]
    model = bench.build_model(cfg, dev)
    pipe = WanImageToVideoPipeline(scheduler=FlowMatchEulerDiscreteScheduler(shift=5.0), transformer=model, expand_timesteps=True)
    pipe.use_hip_graph = False
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
    total = a.warmup + a.steps
    pipe.scheduler.set_timesteps(max(total, 2), device=dev)
    st = pipe.make_state(lat, cond, traj, idl, mask, pe.to(dev).bfloat16(), ne.to(dev).bfloat16(), 5.0)
    ts, dts = pipe.scheduler.timesteps.to(dev).float(), pipe.scheduler.dts.to(dev)
    lat0 = st.lat.clone()

    def run():
        st.lat.copy_(lat0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.no_grad():
            for i in range(total):
                if i == a.warmup:
                    e0.record()
                j = min(i, ts.numel() - 1)
                st.t_rows[1:2].copy_(ts[j:j + 1])
                st.dt.copy_(dts[j:j + 1])
                pipe._step(st)
            e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps

    own, parent = _lib.lib(), None
    if a.parent_lib:                               # the same ABI version; entries it lacks (newer ones) are simply not bound
        parent = ctypes.CDLL(a.parent_lib)
        assert parent.fino_version() == _lib.ABI_VERSION
        for name, argtypes in _lib.SIGNATURES.items():
            fn = getattr(parent, name, None)
            if fn is not None:
                fn.argtypes, fn.restype = argtypes, _lib._RESTYPES.get(name, ctypes.c_int)

    def switch(name):
        model.enable_mxfp8_linears(False)
        model.enable_mxfp6_linears(False)
        _lib._lib = parent if name == "mxfp6-parent" else own       # what every ops call of the step goes through
        if name == "mxfp8":
            model.enable_mxfp8_linears()
        elif name in ("mxfp6", "mxfp6-parent"):
            model.enable_mxfp6_linears()
        elif name == "mxfp6-rot":
            model.enable_mxfp6_linears(rotate=True)

    names = [a.only] if a.only else ["bf16", "mxfp8", "mxfp6", "mxfp6-rot"] + (["mxfp6-parent"] if parent else [])
    print(f"# {torch.cuda.get_device_name(0)}  layers {cfg['num_layers']}  L = {(fg + 1) * (lh // 2) * (lw // 2)} x 2 (CFG)  "
          f"{a.steps} steps after {a.warmup}, eager")
    res = {n: [] for n in names}
    for r in range(1 if a.only else a.reps):
        for n in names:
            switch(n)
            res[n].append(run())
            print(f"rep {r}: {n:12s} linears  {res[n][-1]:8.2f} ms per step")
    switch("bf16")
    if not a.only:
        for n in names:
            print(f"{n:12s}: min {min(res[n]):8.2f}  median {statistics.median(res[n]):8.2f}  max {max(res[n]):8.2f} ms per step")
        peak = bench.measured_mfma_peak(dev, 0.0)
        print(f"matrix peak in this run (fino_diag_mfma_peak, bf16 32x32x16): {peak['power_capped_peak']} TFLOP/s")
    return 0


if __name__ == "__main__":
    sys.exit(main())
