"""LoRA merge roofline on the full-size Wan2.2-5B DiT (random weights): a rank-64 adapter on all ten linears of the 30 blocks
(4.9e9 parameters), timed with device events after warm-up --
  * fino_lora_merge over every target weight (base copy -> parameter), the merge alone;
  * a device-to-device copy of the same bytes (the same weights, base copy -> parameter) in the same run;
  * the whole `set_adapters` re-merge as a caller sees it: bookkeeping, the merges, reset_caches and the re-pack of the fused
    QKV / KV weights.
Prints GB/s and the fraction of copy bandwidth; one JSON line at the end.

    python tools/lora_merge_bench.py [--rank 64] [--reps 5]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from frameino_amd import ops                                         # noqa: E402
from frameino_amd.random_init import random_wan_model                # noqa: E402
from oracle.wan_dit import WAN22_5B_CFG                              # noqa: E402
from tests.parity import model_cfg                                   # noqa: E402

LINEARS = ("attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "attn2.to_q", "attn2.to_k", "attn2.to_v",
           "attn2.to_out.0", "ffn.net.0.proj", "ffn.net.2")


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    m = random_wan_model(model_cfg(WAN22_5B_CFG), dev)
    g = torch.Generator(device=dev).manual_seed(1)
    sd = {}
    for i in range(WAN22_5B_CFG["num_layers"]):
        for lin in LINEARS:
            w = m.get_parameter(f"blocks.{i}.{lin}.weight")
            sd[f"transformer.blocks.{i}.{lin}.lora_A.weight"] = (torch.randn(args.rank, w.shape[1], generator=g, device=dev)
                                                               / args.rank ** 0.5).to(w.dtype)
            sd[f"transformer.blocks.{i}.{lin}.lora_B.weight"] = (0.01 * torch.randn(w.shape[0], args.rank, generator=g,
                                                                                     device=dev)).to(w.dtype)
    m.load_lora_adapter(sd, adapter_name="a")
    m.fuse_lora(1.0)                      # first merge: the base copies are made here
    st = m._lora_state()
    params = dict(m.named_parameters())
    jobs = []
    for name in st["bases"]:
        mod, attr = m._lora_owner(name)
        fac = [f for f in st["adapters"]["a"]["factors"] if f[0] == name][0]
        jobs.append((getattr(mod, attr), params[name].data, fac[1].to(dev), fac[2].to(dev)))
    n_params = sum(w.numel() for _, w, _, _ in jobs)
    nbytes = 2 * sum(w.numel() * w.element_size() for _, w, _, _ in jobs)        # read base + write parameter

    def merge():
        for base, w, a, b in jobs:
            ops.lora_merge_(base, [(a, b, 0.7)], out=w)

    def copy():
        for base, w, _, _ in jobs:
            w.copy_(base)

    weight = [0.5]

    def remerge():
        weight[0] = 1.5 - weight[0]       # a new adapter weight every time: a real re-merge
        m.unfuse_lora()
        m.set_adapters(["a"], [weight[0]])
        m._lora_sync()
        m._pack()

    t_merge, t_copy = timed(merge, args.reps), timed(copy, args.reps)
    t_remerge = timed(remerge, args.reps)
    res = {"params": n_params, "gbytes": nbytes / 1e9, "rank": args.rank,
           "merge_ms": t_merge, "merge_GBps": nbytes / t_merge / 1e6,
           "copy_ms": t_copy, "copy_GBps": nbytes / t_copy / 1e6, "merge_vs_copy": t_copy / t_merge,
           "set_adapters_remerge_ms": t_remerge}
    print(f"{n_params / 1e9:.2f}e9 parameters, {nbytes / 1e9:.1f} GB read+write, rank {args.rank}")
    print(f"fino_lora_merge   {t_merge:8.2f} ms  {res['merge_GBps']:8.0f} GB/s")
    print(f"d2d copy          {t_copy:8.2f} ms  {res['copy_GBps']:8.0f} GB/s")
    print(f"merge / copy bandwidth {res['merge_vs_copy']:.3f}")
    print(f"set_adapters re-merge + re-pack {t_remerge:.2f} ms")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
