#!/usr/bin/env python3
"""The full-size Wan2.2-5B denoise step (bench.py's workload: 49 frames 704 x 1280, batch-2 CFG, eager) in bf16, with MXFP8
linears and with MXFP6 linears, in one process on one box: the three precisions alternated, the sequence run twice, device
events around `steps` steps after `warmup`, plus the in-run matrix peak (fino_diag_mfma_peak) so boxes can be compared.
Usage: mxfp6_step_bench.py [--steps 6] [--warmup 2] [--layers N] > profiles/mxfp6_step.txt"""
import argparse
import os
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
    ap.add_argument("--only", default=None, choices=["bf16", "mxfp8", "mxfp6"], help="one precision (for a kernel trace)")
    a = ap.parse_args()
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

    def switch(name):
        model.enable_mxfp8_linears(False)
        model.enable_mxfp6_linears(False)
        if name == "mxfp8":
            model.enable_mxfp8_linears()
        elif name == "mxfp6":
            model.enable_mxfp6_linears()

    names = [a.only] if a.only else ["bf16", "mxfp8", "mxfp6"]
    print(f"# {torch.cuda.get_device_name(0)}  layers {cfg['num_layers']}  L = {(fg + 1) * (lh // 2) * (lw // 2)} x 2 (CFG)  "
          f"{a.steps} steps after {a.warmup}, eager")
    res = {n: [] for n in names}
    for r in range(1 if a.only else a.reps):
        for n in names:
            switch(n)
            res[n].append(run())
            print(f"rep {r}: {n:6s} linears  {res[n][-1]:8.2f} ms per step")
    if not a.only:
        for n in names:
            print(f"{n:6s}: min {min(res[n]):8.2f}  max {max(res[n]):8.2f} ms per step")
        peak = bench.measured_mfma_peak(dev, 0.0)
        print(f"matrix peak in this run (fino_diag_mfma_peak, bf16 32x32x16): {peak['power_capped_peak']} TFLOP/s")
    return 0


if __name__ == "__main__":
    sys.exit(main())
