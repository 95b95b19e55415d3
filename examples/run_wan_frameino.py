#!/usr/bin/env python3
"""End-to-end FrameINO clip on one MI355X, the way app.py:inference drives the reference pipeline (app.py:560-760):
canvas image + point tracks + identity reference + prompt -> 49 frames.

With `--ckpt <folder>` (a diffusers-format Wan2.2-TI2V-5B FrameINO checkpoint: transformer/, vae/, and -- for text
prompts -- text_encoder/ + tokenizer/ loadable by transformers) it runs the released weights.  Without it the script
runs the same code on random-init weights of the same architecture and synthetic conditions (there is no network
here), which is what `--smoke` (tiny shapes, seconds) checks in the test suite.

    python examples/run_wan_frameino.py --steps 50 --out clip.npy
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synthetic_conditions(frames, height, width, device, seed=0):
    """Stand-ins for the app's inputs (SURVEY 8c harness rows), built the way app.py builds the real ones (:270-350,
    :582-620, :634-695) with the device-side builders of frameino_amd.conditions: a first frame area-resampled into the
    black unbounded canvas, clicked trajectories (one object entering the frame late = 'frame in') resampled by arc
    length into per-frame tracks, an identity reference scaled and zero-padded to the canvas."""
    import PIL.Image
    from frameino_amd.conditions import build_inference_canvas, prepare_id_tensor, tracks_from_trajectories
    rng = np.random.default_rng(seed)
    pad_h, pad_w = (height // 8) // 16 * 16, (width // 6) // 16 * 16
    first = rng.integers(0, 255, (360, 640, 3), dtype=np.uint8)                  # the user's photo, any size
    canvas = build_inference_canvas(first, height - 2 * pad_h, width - 2 * pad_w, pad_h, pad_w, pad_h, pad_w, device)
    uh, uw = 480, 720                                                            # the UI board the user clicks on
    clicks = [[[(uw * 0.25, uh * 0.5), (uw * 0.75, uh * 0.5)], [(uw * 0.27, uh * 0.52), (uw * 0.77, uh * 0.52)]],
              [[(-20.0, uh * 0.3), (uw * 0.55, uh * 0.3)]]]                      # second object starts outside
    tracks = tracks_from_trajectories(clicks, frames, height, width, uh, uw)
    ident = rng.integers(0, 255, (300, 200, 3), dtype=np.uint8)                  # already-masked reference, portrait
    id_tensor = prepare_id_tensor(ident, height, width, "Wan", device)           # [1, 3, 1, H, W] in [-1, 1]
    return PIL.Image.fromarray(canvas.cpu().numpy()), tracks, id_tensor, (pad_h, pad_w, pad_h, pad_w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--frames", type=int, default=49)
    ap.add_argument("--height", type=int, default=704)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--guidance", type=float, default=5.0)
    ap.add_argument("--prompt", default="A corgi runs into the frame from the left.")
    ap.add_argument("--scheduler", choices=["euler", "unipc"], default="unipc")
    ap.add_argument("--smoke", action="store_true", help="tiny random model + tiny VAE, 64x96, 5 frames")
    ap.add_argument("--repeat", type=int, default=1, help="generate the clip this many times (the first call is cold)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--lora", default=None, metavar="PATH",
                    help="a LoRA adapter (local folder or .safetensors file), merged into the transformer's weights")
    ap.add_argument("--lora-scale", type=float, default=1.0, help="the adapter's scale (attention_kwargs['scale'])")
    ap.add_argument("--first-block-cache", type=float, default=None, metavar="THRESHOLD",
                    help="diffusers' first-block caching (approximate; eager loop): skip blocks 1..N-1 of a step whose first-block "
                         "residual changed by at most THRESHOLD (relative L1), e.g. 0.1")
    ap.add_argument("--pab", default=None, metavar="N[,M]",
                    help="diffusers' Pyramid Attention Broadcast (approximate; eager loop): while the timestep is inside (100, 800) "
                         "the self-attention branch is recomputed every N-th step and re-used in between, and with M the text "
                         "cross-attention branch every M-th, e.g. 2 or 2,3.  Not together with --first-block-cache")
    ap.add_argument("--taylorseer", type=int, default=None, metavar="N",
                    help="diffusers' TaylorSeer caching (approximate; eager loop; quality on real checkpoints unmeasured): after "
                         "the warm-up steps every N-th step computes and the steps between extrapolate every attention branch's "
                         "output from finite differences of the computed ones, e.g. 5.  Not together with --first-block-cache, "
                         "--pab, --window-frames or --sparse-attention")
    ap.add_argument("--taylorseer-order", type=int, default=1, metavar="K", help="order of the extrapolation, 0 to 3")
    ap.add_argument("--taylorseer-warmup", type=int, default=3, metavar="W", help="the first W steps always compute")
    ap.add_argument("--taylorseer-lite", action="store_true",
                    help="lite mode: extrapolate the model's output itself; a predicted step runs no block at all")
    ap.add_argument("--fastercache", type=int, nargs="?", const=5, default=None, metavar="N",
                    help="diffusers' FasterCache (approximate; eager loop; quality on real checkpoints unmeasured): while the "
                         "timestep is inside (-1, 641) the unconditional CFG branch runs on every N-th step (default 5) and is "
                         "rebuilt in between from the conditional prediction plus the frequency-split difference of the last "
                         "step that ran both.  Not together with --first-block-cache, --pab or --taylorseer")
    ap.add_argument("--fastercache-attention", type=int, default=None, metavar="M",
                    help="with --fastercache: also recompute every block's self-attention on every M-th step only while the "
                         "timestep is inside (-1, 681), e.g. 2, and extrapolate it from its last two outputs in between (weight "
                         "0.5).  Not together with --window-frames or --sparse-attention")
    ap.add_argument("--magcache", default=None, metavar="FILE",
                    help="diffusers' MagCache (approximate; eager loop; quality on real checkpoints unmeasured) with the per-context "
                         "curves of FILE (written by --magcache-calibrate at the same --steps): a step whose accumulated magnitude "
                         "error stays within the threshold runs no block at all and adds the block stack's residual of the last "
                         "computing step.  Not together with the other cache flags")
    ap.add_argument("--magcache-threshold", type=float, default=0.06, metavar="X", help="with --magcache: the error bound")
    ap.add_argument("--magcache-max-skip", type=int, default=3, metavar="K",
                    help="with --magcache: at most K consecutive skipped steps")
    ap.add_argument("--magcache-retention", type=float, default=0.2, metavar="R",
                    help="with --magcache: the first R * steps steps always compute")
    ap.add_argument("--magcache-calibrate", default=None, metavar="OUT.json",
                    help="run the clip with MagCache in calibrate mode (every step computes; one extra pass over the residual per "
                         "step and context) and write the measured curves, per cache context, to OUT.json.  Curves depend on "
                         "the weights, the step count and the scheduler.  Not together with the other cache flags")
    ap.add_argument("--teacache", default=None, metavar="FILE",
                    help="TeaCache (approximate; eager loop; quality on real checkpoints unmeasured) with the per-context "
                         "polynomials of FILE (written by --teacache-calibrate): before block 0 a step measures how far its "
                         "timestep-modulated input has moved since the previous step, and while the accumulated polynomial of that "
                         "distance stays below the threshold it re-uses the block stack's residual.  Not together with the other "
                         "cache flags")
    ap.add_argument("--teacache-threshold", type=float, default=0.2, metavar="X", help="with --teacache: the accumulated bound")
    ap.add_argument("--teacache-max-skip", type=int, default=None, metavar="K",
                    help="with --teacache: at most K consecutive skipped steps (default: no cap)")
    ap.add_argument("--teacache-calibrate", default=None, metavar="OUT.json",
                    help="run the clip with TeaCache in calibrate mode (every step computes; one probe of block 0's input and one "
                         "of the output rows per step and context), fit a quartic per cache context and write it, with the "
                         "measurements, to OUT.json.  The polynomial depends on the weights.  Not together with the other cache "
                         "flags")
    ap.add_argument("--ras", type=float, default=None, metavar="RATIO",
                    help="region-adaptive sampling (approximate; eager loop; quality on real checkpoints unmeasured): on most steps "
                         "only the fraction RATIO of the tokens whose prediction is moving most, e.g. 0.5, runs through the DiT; "
                         "the others keep their last prediction and serve the self-attention from per-layer K / V planes (two "
                         "planes per CFG branch and layer: 9.1 GB at 704x1280x81).  Not together with the other cache flags, "
                         "--window-frames, --sparse-attention or --fp8-attention")
    ap.add_argument("--ras-interval", type=int, default=5, metavar="N", help="with --ras: every N-th step runs every token")
    ap.add_argument("--ras-warmup", type=int, default=4, metavar="W", help="with --ras: the first W steps run every token")
    ap.add_argument("--ras-trajectory-mask", action="store_true",
                    help="with --ras: the tokens under the painted trajectories are active on every step")
    ap.add_argument("--window-frames", type=int, default=None, metavar="N",
                    help="sliding-window self-attention over latent frames (approximate; quality on real checkpoints unmeasured): "
                         "every query attends its own frame +- N neighbours plus the first frame and the ID frame, e.g. 2.  Not "
                         "together with --pab")
    ap.add_argument("--sparse-attention", type=float, default=None, metavar="TAU",
                    help="dynamic block-sparse self-attention (approximate; quality on real checkpoints unmeasured): per head and "
                         "q-block only the key tiles that a pooled predictor credits with a share TAU of the softmax mass, e.g. "
                         "0.9, plus the own frame, the first frame and the ID frame.  Combines with --fp8-attention (the fp8 tile "
                         "walk, head_dim 128).  Not together with --window-frames or --pab")
    ap.add_argument("--sparse-window-frames", type=int, default=0, metavar="N",
                    help="with --sparse-attention: the own frame +- N neighbours are always kept (default 0)")
    ap.add_argument("--sparse-similarity", type=float, default=None, metavar="THETA",
                    help="with --sparse-attention: never predict from a block whose tokens do not resemble each other (mean "
                         "pairwise cosine below THETA, e.g. 0.3): such a q-block attends everything, such a key tile is always kept")
    ap.add_argument("--sparse-calibrate", default=None, metavar="OUT.json",
                    help="with --sparse-attention: before the clip, run a short dense clip that measures, per layer and head, the "
                         "smallest threshold of a grid whose sparse output stays within --sparse-l1 of the dense one; write the "
                         "thresholds to OUT.json and use them (measured in the DiT's dtype: --fp8-attention is switched on "
                         "after the calibration)")
    ap.add_argument("--sparse-l1", type=float, default=0.05, metavar="X",
                    help="with --sparse-calibrate: the relative L1 error bound per layer and head (default 0.05)")
    ap.add_argument("--sparse-thresholds", default=None, metavar="FILE",
                    help="sparse attention with the configuration and per-head thresholds of FILE (written by --sparse-calibrate); "
                         "instead of --sparse-attention")
    ap.add_argument("--fp8-attention", action="store_true",
                    help="fp8 (e4m3) operands in the 3-D self-attention (reduced precision, opt-in).  Combines with --sparse-attention; not "
                         "together with --window-frames")
    ap.add_argument("--smooth-k", action="store_true",
                    help="with --fp8-attention: subtract the key mean before K is quantised (exact for the softmax)")
    ap.add_argument("--smooth-v", action="store_true",
                    help="with --fp8-attention: subtract the value mean before V is quantised and add it back to the output (exact: "
                         "the softmax weights sum to one)")
    ap.add_argument("--smooth-q", action="store_true",
                    help="with --fp8-attention: subtract each 256-row q-block's mean before Q is quantised and add its share of the "
                         "logits back in fp32 (exact; the dense attention only: not with window or sparse attention)")
    ap.add_argument("--mxfp6", action="store_true", help="MXFP6 (e2m3) linears in the DiT (reduced precision, opt-in)")
    ap.add_argument("--mxfp6-rotate", action="store_true",
                    help="with --mxfp6: rotate every 32-element block of weights and activations by the Walsh-Hadamard matrix "
                         "before it is quantised (exact algebra; spreads outliers over their block)")
    ap.add_argument("--dtype", choices=["fp16", "bf16"], default="fp16",
                    help="the DiT's dtype.  Default fp16 = what the reference app loads it in (app.py:156: "
                         "`WanTransformer3DModel.from_pretrained(..., torch_dtype=torch.float16)`, fp32 islands kept); bf16 is what "
                         "bench.py's headline times (the two run within 1 %% of each other)")
    ap.add_argument("--vae-fp32", type=int, nargs="?", const=3, default=0, metavar="PLANES",
                    help="run the VAE like the reference app does (app.py:157 loads it in fp32): fp32-compute mode on split-bf16 "
                         "products, 3 (default) or 2 bf16 planes per fp32 operand -- `vae.set_compute_dtype(torch.float32)`")
    from frameino_amd.guiders import add_guider_arguments, guider_from_arguments
    add_guider_arguments(ap)
    a = ap.parse_args()
    guider = guider_from_arguments(ap, a)
    if a.mxfp6_rotate and not a.mxfp6:
        ap.error("--mxfp6-rotate needs --mxfp6")
    if a.fastercache_attention is not None and a.fastercache is None:
        ap.error("--fastercache-attention needs --fastercache")
    if a.magcache is not None or a.magcache_calibrate is not None:
        if a.magcache is not None and a.magcache_calibrate is not None:
            ap.error("--magcache FILE applies curves, --magcache-calibrate OUT.json measures them: one at a time")
        if any(v is not None for v in (a.first_block_cache, a.pab, a.taylorseer, a.fastercache)):
            ap.error("--magcache / --magcache-calibrate: not together with --first-block-cache, --pab, --taylorseer or --fastercache")
    if a.teacache is not None or a.teacache_calibrate is not None:
        if a.teacache is not None and a.teacache_calibrate is not None:
            ap.error("--teacache FILE applies polynomials, --teacache-calibrate OUT.json measures them: one at a time")
        if any(v is not None for v in (a.first_block_cache, a.pab, a.taylorseer, a.fastercache, a.magcache, a.magcache_calibrate,
                                       a.ras)):
            ap.error("--teacache / --teacache-calibrate: not together with --first-block-cache, --pab, --taylorseer, --fastercache, "
                     "--magcache or --ras")
    elif a.teacache_threshold != 0.2 or a.teacache_max_skip is not None:
        ap.error("--teacache-threshold / --teacache-max-skip need --teacache FILE")

    if a.ras is None and (a.ras_trajectory_mask or a.ras_interval != 5 or a.ras_warmup != 4):
        ap.error("--ras-interval / --ras-warmup / --ras-trajectory-mask need --ras RATIO")
    if a.ras is not None and any(v is not None for v in (a.first_block_cache, a.pab, a.taylorseer, a.fastercache, a.magcache,
                                                         a.magcache_calibrate)):
        ap.error("--ras: not together with --first-block-cache, --pab, --taylorseer, --fastercache or --magcache")

    from frameino_amd import _lib
    from frameino_amd.autoencoder_kl_wan import AutoencoderKLWan
    from frameino_amd.conditions import prepare_traj_tensor
    from frameino_amd.pipeline_wan_i2v_motion_frameino import WanImageToVideoPipeline
    from frameino_amd.schedulers import FlowMatchEulerDiscreteScheduler, UniPCMultistepScheduler
    _lib.load()
    dev = torch.device("cuda")
    dit_dtype = torch.float16 if a.dtype == "fp16" else torch.bfloat16
    sched = UniPCMultistepScheduler(flow_shift=5.0) if a.scheduler == "unipc" else FlowMatchEulerDiscreteScheduler(shift=5.0)

    tokenizer = text_encoder = None
    if a.ckpt:
        from frameino_amd.autoencoder_kl_wan import AutoencoderKLWan as _V
        from frameino_amd.configs import WAN22_5B_CFG, WAN22_VAE_CFG
        from frameino_amd.loading import config_report, load_scheduler, load_wan_transformer, load_wan_vae, read_config
        from frameino_amd.transformer_wan import WanTransformer3DModel as _T
        # the hyper-parameters this package assumes offline were written from memory: say, key by
        # key, where the checkpoint disagrees -- the checkpoint wins, a surprise here is worth knowing before the clip
        for sub, assumed, cls in (("transformer", WAN22_5B_CFG, _T), ("vae", WAN22_VAE_CFG, _V)):
            for line in config_report(read_config(os.path.join(a.ckpt, sub)), assumed, cls, f"{sub}/config.json"):
                print("[config]", line)
        transformer = load_wan_transformer(os.path.join(a.ckpt, "transformer"), dit_dtype, dev)
        # (app.py:157 loads the VAE in fp32: with --vae-fp32 the interface dtype is fp32 too, not only the arithmetic)
        vae = load_wan_vae(os.path.join(a.ckpt, "vae"), torch.float32 if a.vae_fp32 else torch.bfloat16, dev)
        if os.path.isfile(os.path.join(a.ckpt, "scheduler", "scheduler_config.json")):
            sched = load_scheduler(os.path.join(a.ckpt, "scheduler"))
            print("[config] scheduler from the checkpoint:", type(sched).__name__, dict(sched.config))
        if os.path.isdir(os.path.join(a.ckpt, "text_encoder")):
            from transformers import AutoTokenizer, UMT5EncoderModel
            tokenizer = AutoTokenizer.from_pretrained(os.path.join(a.ckpt, "tokenizer"))
            text_encoder = UMT5EncoderModel.from_pretrained(os.path.join(a.ckpt, "text_encoder"),
                                                            torch_dtype=torch.bfloat16).to(dev)
        text_dim = transformer.config.text_dim
    else:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from bench import build_model
        if a.smoke:
            a.height, a.width, a.frames, a.steps = 64, 96, 5, min(a.steps, 3)
            cfg = dict(patch_size=(1, 2, 2), num_attention_heads=2, attention_head_dim=128, in_channels=32,
                       out_channels=16, text_dim=64, freq_dim=256, ffn_dim=512, num_layers=2, cross_attn_norm=True,
                       qk_norm="rms_norm_across_heads", eps=1e-6, rope_max_seq_len=1024)
            vae = AutoencoderKLWan(base_dim=32, decoder_base_dim=32, z_dim=16, dim_mult=[1, 2, 4, 4], num_res_blocks=1,
                                   temperal_downsample=[False, True, True], is_residual=True, in_channels=12,
                                   out_channels=12, patch_size=2, scale_factor_temporal=4, scale_factor_spatial=16,
                                   latents_mean=[0.0] * 16, latents_std=[1.0] * 16).random_init_(seed=2, device=dev)
        else:
            from frameino_amd.configs import WAN22_5B_CFG, WAN22_VAE_CFG
            cfg = dict(WAN22_5B_CFG)
            vae = AutoencoderKLWan(**WAN22_VAE_CFG).random_init_(seed=2, device=dev)
        transformer = build_model(cfg, dev, dtype=dit_dtype)
        text_dim = cfg["text_dim"]

    if a.vae_fp32:
        vae.set_compute_dtype(torch.float32, planes=a.vae_fp32)
    pipe = WanImageToVideoPipeline(tokenizer=tokenizer, text_encoder=text_encoder, vae=vae, scheduler=sched,
                                   transformer=transformer, expand_timesteps=True)
    if guider is not None:                         # how the two CFG predictions are combined (frameino_amd/guiders.py)
        pipe.set_guider(guider)
    if a.lora:                                     # merged before the first step: the denoise step itself is unchanged
        pipe.load_lora_weights(a.lora, adapter_name="lora")
    if a.first_block_cache is not None:
        from frameino_amd.step_cache import FirstBlockCacheConfig
        transformer.enable_cache(FirstBlockCacheConfig(threshold=a.first_block_cache))
    if a.pab is not None:
        from frameino_amd.step_cache import PyramidAttentionBroadcastConfig
        n_m = [int(v) for v in a.pab.split(",")]
        transformer.enable_cache(PyramidAttentionBroadcastConfig(
            spatial_attention_block_skip_range=n_m[0], cross_attention_block_skip_range=n_m[1] if len(n_m) > 1 else None,
            current_timestep_callback=lambda: pipe.current_timestep))
    if a.taylorseer is not None:
        from frameino_amd.step_cache import TaylorSeerCacheConfig
        transformer.enable_cache(TaylorSeerCacheConfig(cache_interval=a.taylorseer, max_order=a.taylorseer_order,
                                                       disable_cache_before_step=a.taylorseer_warmup,
                                                       use_lite_mode=a.taylorseer_lite))
    if a.fastercache is not None:
        from frameino_amd.step_cache import FasterCacheConfig
        transformer.enable_cache(FasterCacheConfig(unconditional_batch_skip_range=a.fastercache,
                                                   spatial_attention_block_skip_range=a.fastercache_attention,
                                                   attention_weight_callback=lambda _module: 0.5,
                                                   current_timestep_callback=lambda: pipe.current_timestep))
    if a.magcache is not None or a.magcache_calibrate is not None:
        from frameino_amd.step_cache import MagCacheConfig, load_mag_ratios
        transformer.enable_cache(MagCacheConfig(
            threshold=a.magcache_threshold, max_skip_steps=a.magcache_max_skip, retention_ratio=a.magcache_retention,
            num_inference_steps=a.steps, calibrate=a.magcache is None,
            mag_ratios=None if a.magcache is None else load_mag_ratios(a.magcache)))
    if a.teacache is not None or a.teacache_calibrate is not None:
        from frameino_amd.step_cache import TeaCacheConfig, load_teacache
        transformer.enable_cache(TeaCacheConfig(
            rel_l1_thresh=a.teacache_threshold, max_skip_steps=a.teacache_max_skip, num_inference_steps=a.steps,
            calibrate=a.teacache is None, coefficients=None if a.teacache is None else load_teacache(a.teacache)))
    if a.mxfp6:                                    # after the LoRA merge: the merged weights are what is quantised
        transformer.enable_mxfp6_linears(rotate=a.mxfp6_rotate)
    if a.fp8_attention:
        transformer.enable_fp8_attention(smooth_k=a.smooth_k, smooth_v=a.smooth_v, smooth_q=a.smooth_q)
    if a.window_frames is not None:                # sinks: the first frame (config) and the ID frame (the loop's id_frames)
        from frameino_amd.window_attention import WindowAttentionConfig
        transformer.enable_window_attention(WindowAttentionConfig(window_frames=a.window_frames, sink_frames=(0,)))
    sparse_cfg = None
    if a.sparse_thresholds is not None:
        if a.sparse_attention is not None or a.sparse_calibrate is not None:
            ap.error("--sparse-thresholds FILE carries its own configuration: not together with --sparse-attention / --sparse-calibrate")
        from frameino_amd.sparse_calibration import load_sparse_thresholds
        sparse_cfg = load_sparse_thresholds(a.sparse_thresholds)
    elif a.sparse_attention is not None:           # forced tiles: own frame +- N, the first frame, the ID frame (id_frames)
        from frameino_amd.window_attention import SparseAttentionConfig
        sparse_cfg = SparseAttentionConfig(cdf_threshold=a.sparse_attention, window_frames=a.sparse_window_frames,
                                           sink_frames=(0,), similarity_threshold=a.sparse_similarity)
    elif a.sparse_similarity is not None or a.sparse_calibrate is not None:
        ap.error("--sparse-similarity / --sparse-calibrate need --sparse-attention TAU")
    if sparse_cfg is not None and a.sparse_calibrate is None:
        transformer.enable_sparse_attention(sparse_cfg)
    t0 = time.perf_counter()
    canvas, tracks, id_tensor, pads = synthetic_conditions(a.frames, a.height, a.width, dev)
    traj = prepare_traj_tensor(tracks, a.height, a.width, 6, a.width, a.height, device=dev)        # [F, 3, H, W]
    if a.ras is not None:
        from frameino_amd.conditions import trajectory_token_mask
        from frameino_amd.step_cache import RegionAdaptiveSamplingConfig
        pinned = None
        if a.ras_trajectory_mask:                  # a token = patch x the VAE's spatial stride pixels; the ID frame comes last
            px = vae.config.scale_factor_spatial * transformer.config.patch_size[1]
            pinned = trajectory_token_mask(traj, a.height // px, a.width // px, vae.config.scale_factor_temporal,
                                           extra_frames=0 if id_tensor is None else 1)
            print(f"ras: {int(pinned.sum())} of {pinned.numel()} tokens lie under the trajectories")
        transformer.enable_cache(RegionAdaptiveSamplingConfig(sample_ratio=a.ras, full_step_interval=a.ras_interval,
                                                              warmup_steps=a.ras_warmup, num_inference_steps=a.steps,
                                                              always_active=pinned))
    kw = {}
    if text_encoder is None:                                   # no text encoder offline: synthetic prompt embeddings
        g = torch.Generator().manual_seed(0)
        pe = torch.randn(1, 512, text_dim, generator=g)
        pe[:, 32:] = 0
        kw = dict(prompt_embeds=pe.to(dev), negative_prompt_embeds=torch.zeros(1, 512, text_dim, device=dev))
    else:
        kw = dict(prompt=a.prompt, negative_prompt="")
    if a.lora:
        kw["attention_kwargs"] = {"scale": a.lora_scale}
    if a.sparse_calibrate is not None:             # a short dense clip that measures the thresholds on this model's own weights
        from frameino_amd.sparse_calibration import calibrate_sparse_attention, save_sparse_thresholds
        if a.fp8_attention:                        # thresholds are calibrated in bf16 / fp16 and loaded
            transformer.enable_fp8_attention(False)
        sparse_cfg, report = calibrate_sparse_attention(
            transformer, lambda: pipe(image=canvas, traj_tensor=traj, ID_tensor=id_tensor, height=a.height, width=a.width,
                                      num_frames=a.frames, num_inference_steps=min(a.steps, 4), guidance_scale=a.guidance,
                                      generator=torch.Generator().manual_seed(1234), **kw),
            l1_bound=a.sparse_l1, base=sparse_cfg)
        save_sparse_thresholds(a.sparse_calibrate, sparse_cfg)
        flat = [t for row in sparse_cfg.head_thresholds.values() for t in row]
        print(f"sparse calibration: {len(flat)} (layer, head) thresholds within L1 {a.sparse_l1} -> {a.sparse_calibrate}; "
              f"{sum(t >= 1.0 for t in flat)} stay dense, mean threshold of the others "
              f"{sum(t for t in flat if t < 1.0) / max(1, sum(t < 1.0 for t in flat)):.3f}")
        transformer.enable_sparse_attention(sparse_cfg)
        if a.fp8_attention:
            transformer.enable_fp8_attention(smooth_k=a.smooth_k, smooth_v=a.smooth_v, smooth_q=a.smooth_q)
    torch.cuda.synchronize()
    tc = time.perf_counter()
    for rep in range(a.repeat):
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        frames = pipe(image=canvas, traj_tensor=traj, ID_tensor=id_tensor, height=a.height, width=a.width,
                      num_frames=a.frames, num_inference_steps=a.steps, guidance_scale=a.guidance,
                      generator=torch.Generator().manual_seed(1234), **kw).frames[0]
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        assert frames.shape == (a.frames, a.height, a.width, 3) and np.isfinite(frames).all()
        cond_s = f"conditions {tc - t0:.2f} s, " if rep == 0 else ""
        print(f"{cond_s}clip ({a.frames} frames {a.height}x{a.width}, {a.steps} steps, "
              f"{a.scheduler}) {t2 - t1:.2f} s{' (cold)' if rep == 0 and a.repeat > 1 else ''}, "
              f"frames in [{frames.min():.3f}, {frames.max():.3f}], peak device memory "
              f"{torch.cuda.max_memory_allocated() / 2**30:.1f} GiB")
    if a.magcache_calibrate is not None:           # filed when each context finished its steps: one host read per context
        from frameino_amd.step_cache import save_mag_ratios
        cal = transformer.magcache_calibration
        save_mag_ratios(a.magcache_calibrate, cal)
        for ctx, entry in cal.items():
            print(f"magcache calibration [{ctx}]: {len(entry['mag_ratios'])} steps, ratios in [{min(entry['mag_ratios']):.4f}, "
                  f"{max(entry['mag_ratios']):.4f}], largest cosine distance {max(entry['cos_dist']):.2e} -> {a.magcache_calibrate}")
    elif a.magcache is not None:
        log = transformer.cache_log
        print(f"magcache: {sum(not e[2] for e in log)} of {len(log)} forwards re-used the stack's residual")
    if a.teacache_calibrate is not None:           # filed when each context finished its steps: one host read per context
        from frameino_amd.step_cache import fit_teacache_coefficients, save_teacache
        cal = transformer.teacache_calibration
        coef = fit_teacache_coefficients(cal, degree=4)
        save_teacache(a.teacache_calibrate, coef, cal)
        for ctx, entry in cal.items():
            ds = [v for v in entry["rel_l1_in"] if v is not None]
            print(f"teacache calibration [{ctx}]: {len(entry['rel_l1_in'])} steps, input distances in [{min(ds):.4f}, {max(ds):.4f}], "
                  f"coefficients {[round(c, 6) for c in coef[ctx]]} -> {a.teacache_calibrate}")
    elif a.teacache is not None:
        log = transformer.cache_log
        print(f"teacache: {sum(not e[2] for e in log)} of {len(log)} forwards re-used the stack's residual")
    if a.ras is not None:
        log = [e for e in transformer.cache_log if e[0] == "cond"]
        print(f"ras: {sum(not e[2] for e in log)} of {len(log)} steps ran {min(e[3] for e in log)} of {max(e[3] for e in log)} tokens")
    from frameino_amd.conditions import crop_unpadded
    region = crop_unpadded(frames, *pads)                     # app.py:741-748: the original (un-extended) region
    print(f"cropped region {tuple(region.shape)} uint8")
    if a.out:
        np.save(a.out, frames)


if __name__ == "__main__":
    main()
