"""MI355X-native WanTransformer3DModel (Wan2.2-TI2V-5B DiT as used by FrameINO).

Host-side mirror of /root/reference/architecture/transformer_wan.py: same class / parameter names (HF checkpoints
load by key), same `forward(hidden_states, timestep, encoder_hidden_states, encoder_hidden_states_image=None,
return_dict=True, attention_kwargs=None)` signature, same `blocks[i].attn1/attn2` + processor plugin surface,
`cache_context(name)`, `.config`, `.dtype`.  All arithmetic runs in the HIP kernels of libframeino_hip.so.

What is different by design (results identical):
  * the per-token timestep embedding is de-duplicated: R distinct timestep values -> R rows through the time MLP
    and an [R, layers, 6, D] fp32 modulation table + an int32 per-token selector, instead of the reference's
    [1, L, 6, D] fp32 tensors (908 MB per block at L=12320);
  * RoPE tables are built once per (frames, height, width) and kept compact ([L, 64] cos/sin);
  * text K/V of the cross-attention (step-invariant) are cached per `cache_context` name;
  * Q/K/V are one fused GEMM; norm+RoPE run in place on the fused buffer; attention reads it in place;
    bias / GELU / gated-residual are GEMM epilogues.
`enable_cache(FirstBlockCacheConfig(...))` (diffusers' CacheMixin, reference :28, :353) skips blocks 1 .. N-1 of a step whose
first-block residual barely changed; `enable_cache(PyramidAttentionBroadcastConfig(...))` re-uses the self- and / or
cross-attention branch outputs of the previous step on a schedule of the step counter and the timestep
(frameino_amd/step_cache.py); `TaylorSeerCacheConfig` extrapolates the attention branches (or the output) along the step axis;
`FasterCacheConfig` skips the unconditional CFG branch on a schedule and rebuilds its prediction from the conditional one, and
extrapolates the self-attention branches; `MagCacheConfig` skips the whole block stack of a step and adds the stack's residual
of the last computing step, on a schedule of the step counter and a per-model curve (`calibrate=True` measures it);
`RegionAdaptiveSamplingConfig` (this project's) runs only the active token rows of most steps, the others serving the self-attention
from per-layer K / V planes.  One at a time, all off by default.
"""
import contextlib
import math
import os
from types import SimpleNamespace

import torch
from torch import nn

from . import ops
from .attention_processor import Attention, MI355WanAttnProcessor
from .loading import FromPretrainedMixin
from .lora import LoraModelMixin
from .mx_linears import MXLinearsMixin
from .step_cache import StepCacheMixin
from .window_attention import SelfAttentionOptionsMixin


class _Config(dict):
    __getattr__ = dict.__getitem__


class _FP32LayerNormParams(nn.Module):
    """Parameter holder for diffusers' FP32LayerNorm (weight/bias stay fp32: reference :393)."""

    def __init__(self, dim, eps, elementwise_affine):
        super().__init__()
        self.eps = eps
        if elementwise_affine:
            self.weight = nn.Parameter(torch.ones(dim))
            self.bias = nn.Parameter(torch.zeros(dim))
        else:
            self.register_parameter("weight", None)
            self.register_parameter("bias", None)


class _GELUProj(nn.Module):
    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.proj = nn.Linear(dim_in, dim_out)


class FeedForward(nn.Module):
    """Parameter layout of diffusers FeedForward("gelu-approximate"): net.0.proj, net.2."""

    def __init__(self, dim, inner_dim):
        super().__init__()
        self.net = nn.ModuleList([_GELUProj(dim, inner_dim), nn.Dropout(0.0), nn.Linear(inner_dim, dim)])


class _MLP2(nn.Module):
    def __init__(self, d_in, d_hidden, d_out=None):
        super().__init__()
        self.linear_1 = nn.Linear(d_in, d_hidden)
        self.linear_2 = nn.Linear(d_hidden, d_out or d_hidden)


class WanTimeTextImageEmbedding(nn.Module):
    """Parameters of reference :146-166 (image_embedder absent: image_dim=None for TI2V-5B)."""

    def __init__(self, dim, time_freq_dim, time_proj_dim, text_embed_dim):
        super().__init__()
        self.time_embedder = _MLP2(time_freq_dim, dim)
        self.time_proj = nn.Linear(dim, time_proj_dim)
        self.text_embedder = _MLP2(text_embed_dim, dim)


def wan_rope_tables(head_dim, max_seq_len, ppf, pph, ppw, theta=10000.0):
    """Compact RoPE tables [L, head_dim/2] (cos, sin) equal to WanRotaryPosEmbed (reference :192-253) sampled at
    the slots the processor reads (:82-83).  fp64 angle tables, stored fp32, as the reference."""
    h_dim = w_dim = 2 * (head_dim // 6)
    t_dim = head_dim - h_dim - w_dim

    def axis(dim):
        freqs = 1.0 / (theta ** (torch.arange(0, dim, 2, dtype=torch.float64)[: dim // 2] / dim))
        ang = torch.outer(torch.arange(max_seq_len, dtype=torch.float64), freqs)
        return ang.cos().float(), ang.sin().float()          # [S, dim/2] (pairwise-repeated values deduplicated)

    (ct, st), (ch, sh), (cw, sw) = axis(t_dim), axis(h_dim), axis(w_dim)

    def build(t, h, w):
        a = t[:ppf].view(ppf, 1, 1, -1).expand(ppf, pph, ppw, -1)
        b = h[:pph].view(1, pph, 1, -1).expand(ppf, pph, ppw, -1)
        c = w[:ppw].view(1, 1, ppw, -1).expand(ppf, pph, ppw, -1)
        return torch.cat([a, b, c], dim=-1).reshape(ppf * pph * ppw, -1).contiguous()

    return build(ct, ch, cw), build(st, sh, sw)


class WanTransformerBlock(nn.Module):
    def __init__(self, dim, ffn_dim, num_heads, qk_norm="rms_norm_across_heads", cross_attn_norm=False, eps=1e-6):
        super().__init__()
        self.attn1 = Attention(dim, heads=num_heads, dim_head=dim // num_heads, qk_norm=qk_norm, eps=eps, bias=True,
                               out_bias=True, processor=MI355WanAttnProcessor())
        self.attn2 = Attention(dim, heads=num_heads, dim_head=dim // num_heads, qk_norm=qk_norm, eps=eps, bias=True,
                               out_bias=True, processor=MI355WanAttnProcessor())
        self.norm2 = _FP32LayerNormParams(dim, eps, True) if cross_attn_norm else None
        self.ffn = FeedForward(dim, ffn_dim)
        self.scale_shift_table = nn.Parameter(torch.randn(1, 6, dim) / dim ** 0.5)


class WanTransformer3DModel(nn.Module, FromPretrainedMixin, LoraModelMixin, StepCacheMixin, MXLinearsMixin,
                            SelfAttentionOptionsMixin):
    """MX linears (enable_mxfp8_linears / enable_mxfp6_linears): the six large linears of every block -- QKV, attention out,
    cross-attention q / out, FFN up / down.

    fp8 attention (enable_fp8_attention): the 3-D self-attention (transformer_wan.py:108) -- fino_attn_fwd_fp8, head_dim 128 as
    two 64-channel sub-heads.  Single-GPU forward only; rel-RMS ~5e-2 per attention output on N(0, 1) inputs
    (tests/test_attention_fp8_gpu.py).  The text cross-attention stays bf16.

    Window attention (enable_window_attention; frameino_amd/window_attention.py): first-block caching, MX
    linears and LoRA work with it; fp8 attention (the range walk exists in the bf16 / fp16 kernel only), Pyramid Attention
    Broadcast, a token-sharded plan and user-installed attention processors are refused.

    Sparse attention (enable_sparse_attention): per head and q-block only the key tiles a device-side
    predictor picks, plus the own frame, the sink frames and the ID frame.  First-block caching, MX linears, LoRA and the
    hipGraph loop work with it, and so does fp8 attention at head_dim 128 (the fp8 tile walk, fino_attn_fwd_fp8_tiles, over the
    mask predicted from the bf16 / fp16 q and k; DESIGN.md section 6m -- any other head_dim is refused); window attention,
    Pyramid Attention Broadcast, TaylorSeer caching, a token-sharded plan and user-installed attention processors are refused.
    Its similarity gate, per-head thresholds and their calibration (frameino_amd/sparse_calibration.py; bf16 / fp16 only):
    DESIGN.md section 6k.

    FasterCache (enable_cache(FasterCacheConfig(...))): the unconditional CFG branch runs on a schedule and
    is rebuilt from the conditional prediction in between (`_faster_forward`); that part works with MX linears, fp8 / window /
    sparse attention and LoRA.  Its self-attention extrapolation takes TaylorSeer's route through the attention branches and
    refuses what TaylorSeer's default mode refuses.

    Region-adaptive sampling (enable_cache(RegionAdaptiveSamplingConfig(...))): a partial forward runs the
    listed token rows alone (`_ras_partial`), q at lq = La against per-layer K / V planes of all rows; LoRA and MX linears work with
    it; window, sparse and fp8 attention, a token-sharded plan and user-installed attention processors are refused."""
    _window_table_cache = "_rope_cache"
    _loader_name = "load_wan_transformer"
    _keep_in_fp32_modules = ["time_embedder", "scale_shift_table", "norm1", "norm2", "norm3"]   # reference :393
    _lora_wan_layout = True   # LoRA files in the original Wan-repo / kohya key layout map onto these names (frameino_amd/lora.py)

    def __init__(self, patch_size=(1, 2, 2), num_attention_heads=40, attention_head_dim=128, in_channels=16,
                 out_channels=16, text_dim=4096, freq_dim=256, ffn_dim=13824, num_layers=40, cross_attn_norm=True,
                 qk_norm="rms_norm_across_heads", eps=1e-6, image_dim=None, added_kv_proj_dim=None,
                 rope_max_seq_len=1024, pos_embed_seq_len=None):
        super().__init__()
        if image_dim is not None or added_kv_proj_dim is not None:
            raise NotImplementedError("Wan2.1 image-embedding branch is outside FrameINO's TI2V-5B path")
        self.config = _Config(patch_size=tuple(patch_size), num_attention_heads=num_attention_heads,
                              attention_head_dim=attention_head_dim, in_channels=in_channels,
                              out_channels=out_channels or in_channels, text_dim=text_dim, freq_dim=freq_dim,
                              ffn_dim=ffn_dim, num_layers=num_layers, cross_attn_norm=cross_attn_norm, qk_norm=qk_norm,
                              eps=eps, image_dim=image_dim, added_kv_proj_dim=added_kv_proj_dim,
                              rope_max_seq_len=rope_max_seq_len, pos_embed_seq_len=pos_embed_seq_len)
        inner = num_attention_heads * attention_head_dim
        self.inner_dim = inner
        self.patch_embedding = nn.Conv3d(in_channels, inner, kernel_size=patch_size, stride=patch_size)
        self.condition_embedder = WanTimeTextImageEmbedding(inner, freq_dim, inner * 6, text_dim)
        self.blocks = nn.ModuleList([WanTransformerBlock(inner, ffn_dim, num_attention_heads, qk_norm, cross_attn_norm,
                                                         eps) for _ in range(num_layers)])
        self.proj_out = nn.Linear(inner, self.config.out_channels * math.prod(patch_size))
        self.scale_shift_table = nn.Parameter(torch.randn(1, 2, inner) / inner ** 0.5)
        self._packed = None
        self._rope_cache = {}
        self._text_cache = {}
        self._ws = {}
        self._ws_rows_floor = 0           # FasterCache: a batch-1 step of a batch-2 loop binds the batch-2 workspace
        self._faster_text = None          # ... and the "cond" row of the loop's stacked prompt, sliced once per prompt
        self._faster_defer_delta = False  # the loop's two-stream CFG path takes the delta itself, after the streams join
        self._ctx_name = None
        self.ops = ops            # kernel front end (tests of the sharding logic inject a CPU stand-in)
        self.parallel = None      # frameino_amd.parallel.TokenShard or None
        self.dedup_shared_prefix = True   # A/B knob: CFG-batched call computes the branch-invariant prefix once
        # True: q of the self-attention leaves its norm + RoPE kernel already multiplied by head_dim**-0.5 * log2(e) (fp32,
        # one rounding) and the attention kernels take q.k as the exp2 argument (FINO_ATTN_SCALE_FOLDED), which lets the
        # 4-wave kernel fold the running maximum into its MFMAs.  False (default): q rounded where the reference rounds it,
        # scale applied to the logits -- inside the power-capped step the fold buys nothing.
        self.fold_softmax_scale = False
        self._init_self_attention_options()
        # The text cross-attention over a ZERO-PADDED prompt (pipeline_wan...FrameINO.py:235-238 pads every prompt to 512 tokens
        # with zero rows): all padding tokens yield the same K and V row, so the real tokens + ONE key that stands for the run
        # give the same softmax (ops.attention_tail: softmax(q.[K; k x M]) [V; v x M] = softmax(q.[K; k] + [0; ln M]) [V; v]).
        # Found per prompt from the embeddings themselves (trailing all-zero rows), default processors only; False = attend to
        # all 512 rows as the reference does.
        self.dedup_text_padding = os.environ.get("FINO_TEXT_FOLD", "1") != "0"      # (the environment switch: A/B timing)
        # ... and then the text cross-attention's out-projection re-associated as P.(V W_o^T) (see _text_out_weights)
        self.reassociate_text_out = os.environ.get("FINO_TEXT_REASSOC", "1") != "0"
        # honour `forward(live_rows=...)`: in the last block, rows the caller discards contribute K | V only (round 6)
        self.skip_dead_rows = os.environ.get("FINO_SKIP_DEAD_ROWS", "1") != "0"

    # ------------------------------------------------------------------ diffusers-style surface
    @property
    def dtype(self):
        return self.proj_out.weight.dtype

    @property
    def device(self):
        return self.proj_out.weight.device

    @contextlib.contextmanager
    def cache_context(self, name):
        prev, self._ctx_name = self._ctx_name, name
        try:
            yield
        finally:
            self._ctx_name = prev

    @property
    def attn_processors(self):
        out = {}
        for i, blk in enumerate(self.blocks):
            out[f"blocks.{i}.attn1.processor"] = blk.attn1.processor
            out[f"blocks.{i}.attn2.processor"] = blk.attn2.processor
        return out

    def load_reference_state_dict(self, sd, dtype=None):
        """Load weights keyed by the reference's parameter names; non-fp32-island tensors are cast to `dtype`."""
        own = self.state_dict()
        missing = [k for k in own if k not in sd]
        extra = [k for k in sd if k not in own]
        if missing or extra:
            raise KeyError(f"state-dict mismatch: missing {missing[:5]} unexpected {extra[:5]}")
        with torch.no_grad():
            for k, p in self.named_parameters():
                keep32 = any(s in k for s in self._keep_in_fp32_modules)
                t = sd[k].to(torch.float32 if keep32 else (dtype or sd[k].dtype))
                p.data = t.to(p.device).contiguous()
        self.reset_caches()
        return self

    # ------------------------------------------------------------------ derived state
    def reset_caches(self):
        """Drop everything derived from the parameters or the prompt: packed/fused weight copies, MX weights, text
        K/V, RoPE tables, workspaces, first-block-cache residuals.  Called whenever the parameters may have changed or moved.
        Returns whether MX linears were on (they are re-quantised by the next forward)."""
        had_fp8 = self._mx_invalidate()
        self._reset_stateful_cache()
        self._packed = None
        self._text_cache.clear()
        self._faster_text = None
        self._rope_cache.clear()          # (the window-attention range tables live here too: `_window_table_cache`)
        self._ws.clear()
        return had_fp8

    def _apply(self, fn, *args, **kwargs):          # .to() / .cuda() / .half() / .float(): parameters move or change
        out = super()._apply(fn, *args, **kwargs)
        if hasattr(self, "_text_cache"):
            self.reset_caches()
        return out

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self.reset_caches()
        return out

    def _default_processors(self):
        # exactly our processor (not a subclass): the fused strategies behind `_self_attention` and the default arm of
        # `_cross_attention` ARE that processor's body; anything else the user installed (set_processor, at any time) is called
        # through the plugin protocol instead (`_sa_processors`, the other arm of `_cross_attention`).
        return all(type(b.attn1.processor) is MI355WanAttnProcessor and type(b.attn2.processor) is MI355WanAttnProcessor
                   for b in self.blocks)

    def _pack(self):
        """One-time repack for the fused kernels: fused QKV / KV weights, flat patch-embed weight, the 30 per-block
        scale_shift_tables stacked (fp32)."""
        d = self.inner_dim
        pk = SimpleNamespace(layers=[])
        for blk in self.blocks:
            a1, a2 = blk.attn1, blk.attn2
            e = SimpleNamespace()
            e.wqkv = torch.cat([a1.to_q.weight, a1.to_k.weight, a1.to_v.weight]).detach().contiguous()
            e.bqkv = torch.cat([a1.to_q.bias, a1.to_k.bias, a1.to_v.bias]).detach().contiguous()
            e.wkv2 = torch.cat([a2.to_k.weight, a2.to_v.weight]).detach().contiguous()
            e.bkv2 = torch.cat([a2.to_k.bias, a2.to_v.bias]).detach().contiguous()
            pk.layers.append(e)
        pk.sst = torch.stack([b.scale_shift_table.detach().float()[0] for b in self.blocks])        # [layers, 6, D]
        pk.w_patch = self.patch_embedding.weight.detach().reshape(d, -1).contiguous()
        self._packed = pk
        return pk

    def _mx_linear_weights(self, pk):
        for li, (blk, e) in enumerate(zip(self.blocks, pk.layers)):
            for key, w in (("qkv", e.wqkv), ("out", blk.attn1.to_out[0].weight), ("q2", blk.attn2.to_q.weight),
                           ("out2", blk.attn2.to_out[0].weight), ("ff1", blk.ffn.net[0].proj.weight),
                           ("ff2", blk.ffn.net[2].weight)):
                yield li, key, w

    def _window_refusals(self, fp8, default_procs, shard=None):
        what = "window attention (enable_window_attention)"
        if fp8:
            raise NotImplementedError(f"{what} with fp8 attention: the range walk exists in the bf16 / fp16 kernel only; switch "
                                      f"one of them off first (disable_window_attention() / enable_fp8_attention(False))")
        self._cache_refusals(window=True)
        if shard is not None and getattr(shard, "active", True):
            raise NotImplementedError(f"{what} with a token-sharded plan: it runs on one GPU")
        if not default_procs:
            raise NotImplementedError(f"{what} with a user-installed attention processor: the windows are applied by the "
                                      f"built-in MI355WanAttnProcessor path only")

    def _cache_refusals(self, policy=None, config=None, enabling=False, window=False, sparse=False, shard=None, default_procs=True,
                        fp8=False):
        """What a step cache does not combine with on this model, in both orders.  `enabling`: `enable_cache` asks about `policy`
        and `config`, against what the model has on; else the enabled cache is asked about the feature that is being switched
        on (`window` / `sparse`: `_window_refusals`, `_sparse_refusals`) and about the forward that is about to run (`shard`,
        `default_procs`: `_bind`, before its first launch).  No cache runs token-sharded.  One that takes over the attention
        branches (`policy.hooks_attention`) does not run beside window or sparse attention and needs the built-in processors;
        the policies state the two exceptions (`takes_windows`, `takes_any_processor`).  `fp8`: fp8 self-attention, for a policy that
        keeps K / V in the model dtype (`takes_fp8_attention`)."""
        policy = policy or self._step_cache_policy
        if policy is None:
            return
        config = config if enabling else self._step_cache_config
        if enabling:
            window, sparse, shard, fp8 = self._window is not None, self._sparse is not None, self.parallel, self.fp8_attention
            default_procs = policy.takes_any_processor(config) or self._default_processors()
        if shard is not None and getattr(shard, "active", True):
            raise NotImplementedError(f"{policy.label} with a token-sharded plan: the step caches run on one GPU")
        what = policy.attention_label or policy.label
        if fp8 and not policy.takes_fp8_attention(config):
            first, second = (what, "fp8 attention (enable_fp8_attention)") if enabling else ("fp8 attention (enable_fp8_attention)", what)
            raise NotImplementedError(f"{first} with {second}: the K / V planes are kept in the model dtype and read by the "
                                      f"bf16 / fp16 kernel; switch one of them off first")
        for on, other in ((window, "window attention (enable_window_attention)"), (sparse, "sparse attention (enable_sparse_attention)")):
            if on and not policy.takes_windows(config):
                first, second = (what, other) if enabling else (other, what)
                raise NotImplementedError(f"{first} with {second}: not implemented in this version ({policy.instead})")
        if not default_procs and not policy.takes_any_processor(config):
            raise NotImplementedError(f"{what} with a user-installed attention processor: the attention branches are predicted on "
                                      f"the built-in MI355WanAttnProcessor path only")

    def disable_cache(self):
        super().disable_cache()
        for ws in self._ws.values():          # TaylorSeer's [n, D] scratch for a computed branch's y
            ws.taylor_y = None

    def _workspace(self, L, dtype, device):
        # one workspace per (shape, cache_context name): the two CFG branches may run concurrently on two streams
        key = (L, dtype, str(device), self._ctx_name)
        if L < self._ws_rows_floor:     # FasterCache's batch-1 step of a batch-2 loop: the views of the larger workspace
            big = self._ws.get((self._ws_rows_floor,) + key[1:])
            if big is not None:
                return big
        ws = self._ws.get(key)
        if ws is None:
            d, f = self.inner_dim, self.config.ffn_dim
            mk = lambda *s: torch.empty(*s, dtype=dtype, device=device)          # noqa: E731
            ws = SimpleNamespace(x=mk(L, d), n=mk(L, d), qkv=mk(L, 3 * d), att=mk(L, d), q2=mk(L, d), ff=mk(L, f),
                                 a=mk(L, self.config.in_channels * math.prod(self.config.patch_size)),
                                 po=mk(L, self.config.out_channels * math.prod(self.config.patch_size)))
            self._ws = {k: v for k, v in self._ws.items() if k[:3] == key[:3]}      # drop other shapes, keep branches
            self._ws[key] = ws
        return ws

    def _rope(self, ppf, pph, ppw, device):
        key = (ppf, pph, ppw, str(device))
        if key not in self._rope_cache:
            cos, sin = wan_rope_tables(self.config.attention_head_dim, self.config.rope_max_seq_len, ppf, pph, ppw)
            self._rope_cache[key] = (cos.to(device), sin.to(device))
        return self._rope_cache[key]

    # ------------------------------------------------------------------ conditioning
    def _time_rows(self, t_rows, act_dtype):
        """Reference :175-183 on R distinct timestep values.  Returns temb [R, D] (act dtype) and
        timestep_proj [R, 6, D] (act dtype)."""
        ce = self.condition_embedder
        half = self.config.freq_dim // 2
        expo = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32, device=t_rows.device) / half)
        ang = t_rows.float()[:, None] * expo[None, :]
        sinus = torch.cat([torch.cos(ang), torch.sin(ang)], dim=-1)               # flip_sin_to_cos=True
        te = ce.time_embedder
        wd = te.linear_1.weight.dtype                     # fp32 when the reference's fp32 islands are kept (:393)
        silu = torch.nn.functional.silu
        outs = []
        for i in range(0, sinus.shape[0], 16):                                    # skinny kernel: <= 16 rows/call
            s = sinus[i:i + 16].to(wd).float().contiguous()                       # :179-181
            h = self.ops.skinny_linear(s, te.linear_1.weight, te.linear_1.bias).to(wd)
            h = silu(h).float().contiguous()
            e = self.ops.skinny_linear(h, te.linear_2.weight, te.linear_2.bias).to(wd)
            temb = e.to(act_dtype)                                                # .type_as(encoder_hidden_states) :182
            a = silu(temb).float().contiguous()                                   # act_fn(temb) in the act dtype :183
            tp = self.ops.skinny_linear(a, ce.time_proj.weight, ce.time_proj.bias).to(ce.time_proj.weight.dtype)
            outs.append((temb, tp))
        temb = torch.cat([o[0] for o in outs])
        tproj = torch.cat([o[1] for o in outs]).unflatten(1, (6, -1))
        return temb, tproj

    def _qk_norm_rope(self, blk, qkv, d, cos, sin, dh, qfold, **scatter):
        """norm_q / norm_k ("rms_norm_across_heads", :64-67) + RoPE (:73-90) on the q and k columns of the fused projection in
        ONE launch (the arithmetic of two rmsnorm_rope_ calls, bit for bit): in place, or -- `scatter`: out / head_off / head_ld
        of the heads exchange -- q, k and v written by head into the send buffers"""
        a = blk.attn1
        self.ops.qkv_rmsnorm_rope_(qkv, d, a.norm_q.weight, a.norm_q.eps, a.norm_k.weight, a.norm_k.eps, cos, sin, dh,
                                   q_out_scale=qfold.get("out_scale", 1.0), **scatter)

    def _text_tail(self, ehs, lq):
        """(rows to keep, per-sample key counts, per-sample multiplicities) when every sample of the prompt batch ends in a run of
        all-zero rows worth folding into one key, else None.  One host read per prompt (the result is cached with the K / V)."""
        o = self.ops
        b, lt, _ = ehs.shape
        if not (self.dedup_text_padding and hasattr(o, "attention_tail")):
            return None
        live = (ehs != 0).any(dim=-1)                                                  # [b, lt]
        last = torch.where(live.any(dim=1), lt - 1 - live.flip(1).int().argmax(dim=1), torch.full((b,), -1, device=ehs.device))
        n_real = [int(x) + 1 for x in last.tolist()]                                   # tokens before the zero run
        if max(n_real) >= lt:                                                          # a prompt without padding
            return None
        keep = max(128, -(-(max(n_real) + 1) // 64) * 64)                              # >= 2 key tiles for the walking kernel
        heads = self.config.num_attention_heads
        if keep > lt - 64 or not o.attention_tail_supported(b, heads, lq, keep, self.inner_dim // heads):
            return None
        return keep, [n + 1 for n in n_real], [float(lt - n) for n in n_real]

    def _text_out_weights(self, val, b, lq, pk):
        """(P.V) W_o^T = P.(V W_o^T): with the padding run folded a sample's text is lk <= ~130 keys, so per layer and sample
        W2 = [W_o,h V_h^T]_h  ([D, heads x kp], kp = lk rounded up to 8) is a per-prompt constant and the out-projection of the
        text cross-attention (:117 after :108) a GEMM over K = heads x kp (1728 / 384 at 64 / 8 prompt tokens) instead of 3072,
        fed by the attention PROBABILITIES (ops.attention_probs).  One GEMM per layer and sample builds it: W_o against the
        block-diagonal arrangement of V (row h kp + j = V[j] restricted to head h's channels)."""
        o, d = self.ops, self.inner_dim
        heads = self.config.num_attention_heads
        dh = d // heads
        lk_b = val.tail[0]
        kps = [-(-lk // 8) * 8 for lk in lk_b]
        dev, dt = val.txt.device, val.txt.dtype
        hidx = torch.arange(heads, device=dev)
        val.kp = kps
        val.pbuf = [torch.empty((lq, heads * kp), dtype=dt, device=dev) for kp in kps]
        val.rrms = torch.empty(b * lq, dtype=torch.float32, device=dev)
        val.w2 = []
        for li, blk in enumerate(self.blocks):
            kv = val.kv[li].view(b, val.lt, 2 * d)
            per_sample = []
            for i, kp in enumerate(kps):
                vblk = torch.zeros((heads, kp, heads, dh), dtype=dt, device=dev)
                vblk[hidx, :, hidx, :] = kv[i, :kp, d:].reshape(kp, heads, dh).permute(1, 0, 2)
                per_sample.append(o.gemm(blk.attn2.to_out[0].weight, vblk.view(heads * kp, d)))       # [D, heads*kp]
            val.w2.append(per_sample)
        if dt == torch.float16:
            # fp16 only (round 6): V W_o^T is STORED in the model dtype.  A text key with a large value vector and a vanishing
            # probability is harmless in the reference's order -- (P.V) stays finite -- but an element of V W_o^T beyond 65504
            # is inf here and P.inf = nan for every query.  One host read per prompt (this runs when the per-prompt cache is
            # built, never inside a captured step): if anything left the range, this prompt keeps the ordinary out-projection.
            finite = torch.stack([torch.isfinite(w).all() for layer in val.w2 for w in layer]).all()
            if not bool(finite):
                val.w2, val.pbuf, val.rrms = None, None, None

    def _text_kv(self, encoder_hidden_states, pk, lq=0, may_fold=False, slot=None):
        """text_embedder (:185) + the 30 layers' attn2 K (after norm_k) and V: step-invariant, cached per
        cache_context name for as long as the caller passes the SAME prompt tensor object, unmodified.  `may_fold`: the
        zero-padded tail of the prompt may be folded into one key (`dedup_text_padding`): then only the kept rows are embedded
        and projected (row-wise operations: the kept rows come out bit-identical) and `.tail` carries (key counts, multiplicities)."""
        name = self._ctx_name if slot is None else (self._ctx_name, slot)     # (`slot`: a second entry under one context)
        hit = self._text_cache.get(name)
        key = (bool(may_fold), int(lq) if may_fold else 0, self._mx_on, self.reassociate_text_out, self.dedup_text_padding)
        if hit is not None and hit[0] is encoder_hidden_states and hit[1] == encoder_hidden_states._version and hit[3] == key:
            return hit[2]
        ce = self.condition_embedder
        d = self.inner_dim
        tail = self._text_tail(encoder_hidden_states, lq) if may_fold else None
        kept = encoder_hidden_states if tail is None else encoder_hidden_states[:, :tail[0]].contiguous()
        ctx = kept.reshape(-1, kept.shape[-1])
        h = self.ops.gemm(ctx, ce.text_embedder.linear_1.weight, ce.text_embedder.linear_1.bias, self.ops.EPI_GELU_TANH)
        txt = self.ops.gemm(h, ce.text_embedder.linear_2.weight, ce.text_embedder.linear_2.bias)
        kvs = []
        for blk, e in zip(self.blocks, pk.layers):
            kv = self.ops.gemm(txt, e.wkv2, e.bkv2)                                     # [Lt, 2D]
            self.ops.rmsnorm_rope_(kv[:, :d], blk.attn2.norm_k.weight, blk.attn2.norm_k.eps)
            kvs.append(kv)
        # (a field added to this namespace, here or in `_text_out_weights`, needs its one-sample view in `_text_element` below:
        # Pyramid Attention Broadcast runs a batch's attention branches on it)
        val = SimpleNamespace(txt=txt, kv=kvs, lt=kept.shape[1], tail=None if tail is None else (tail[1], tail[2]), w2=None)
        # P.(V W_o^T) pays only while its K = heads x keys stays well under D (K = 1728 / 384 at 64 / 8 prompt tokens against
        # 3072): from ~77 kept keys on (24 heads) it costs the FLOPs it saves, plus the rrms / probabilities passes, a GEMM per
        # sample and 30 cached [D, heads x kp] matrices per sample (0.32 GB for a 64-token prompt, per cache context).  Longer prompts take the
        # folded attention + the ordinary out-projection.
        worth = tail is not None and self.config.num_attention_heads * (-(-max(tail[1]) // 8) * 8) <= 0.6 * d
        if worth and self.reassociate_text_out and not self._mx_on \
                and hasattr(self.ops, "attention_probs") \
                and self.ops.attention_probs_supported(1, self.config.num_attention_heads, lq, kept.shape[1],
                                                       d // self.config.num_attention_heads):
            self._text_out_weights(val, kept.shape[0], lq, pk)
        # the entry holds the prompt tensor itself: identity (`is`) + in-place version, never its address -- a freed
        # prompt's address is handed to the next same-shape prompt by the caching allocator
        self._text_cache[name] = (encoder_hidden_states, encoder_hidden_states._version, val, key)
        return val

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward(self, hidden_states, timestep, encoder_hidden_states, encoder_hidden_states_image=None,
                return_dict=True, attention_kwargs=None, timestep_rows=None, live_rows=None, _cache_contexts=None,
                id_frames=0, _active_rows=None):
        """`timestep_rows=(values [R], selector int32 [L])` is the de-duplicated form of a per-token timestep; when a
        2-D `timestep` is given instead it is de-duplicated here (torch.unique: host sync, eager only).
        `live_rows=(lo, hi)` (round 6): the caller will only read the output of token rows [lo, hi) -- the FrameINO loop drops the
        ID frame's prediction (pipeline_wan_i2v_motion_FrameINO.py:884-885) and re-imposes the first latent frame from the
        condition before every forward and at the end (:829, :913).  In the LAST block the other rows then only feed the
        self-attention as keys and values: their q projection's use, attention queries, out-projection, text branch, FFN and
        output head are skipped, and their part of the returned tensor is ZERO.  Every kept row is computed exactly as without it.
        A bare `transformer(...)` call (None) keeps the full output.
        `_cache_contexts` (private; a step cache enabled -- first-block caching, Pyramid Attention Broadcast, TaylorSeer, MagCache): one
        cache-context name per batch element, each element then decided on its own as if called alone under that context -- the
        pipeline's CFG-batched call passes ("cond", "uncond").  Without it a batch-B call under one `cache_context` makes one
        joint decision, as diffusers does (first-block caching: over the means of all its rows; Pyramid Attention Broadcast:
        one counter and one [B * L, D] buffer per layer and kind for the whole batch; TaylorSeer likewise, with its factor planes).
        `id_frames` (window and sparse attention only, `enable_window_attention` / `enable_sparse_attention`): the trailing latent frames that are identity-reference
        frames -- every query sees them, like the configured sink frames.
        `_active_rows` (private, a TEST HOOK of region-adaptive sampling): an integer tensor of token rows that replaces the list
        the model would derive, for this one forward, which is then partial whatever the schedule says (the sit-out counters
        stay as they are)."""
        gen = self.forward_steps(hidden_states, timestep, encoder_hidden_states, encoder_hidden_states_image,
                                 return_dict, attention_kwargs, timestep_rows, live_rows=live_rows,
                                 _cache_contexts=_cache_contexts, id_frames=id_frames, _active_rows=_active_rows)
        while True:
            try:
                next(gen)
            except StopIteration as done:
                return done.value

    def forward_steps(self, hidden_states, timestep, encoder_hidden_states, encoder_hidden_states_image=None,
                      return_dict=True, attention_kwargs=None, timestep_rows=None, shard=None, live_rows=None,
                      _cache_contexts=None, id_frames=0, _active_rows=None):
        """The forward as a generator that yields after the embedding stage and after every block, so that a caller
        can interleave two independent forwards (the CFG branches) kernel-stream by kernel-stream
        (frameino_amd/parallel.py: one branch's K|V all-gather then flies under the other branch's compute).  Every
        piece of per-call state (workspace, text K/V, shard) is bound at the first `next()` (`_bind` -> `_Call`); `shard`
        overrides `self.parallel` for this call.  Returns (StopIteration.value) what `forward` returns.
        The stages are plain methods on that state; which self-attention strategy a call takes is `_self_attention`'s dispatch."""
        if encoder_hidden_states_image is not None:
            raise NotImplementedError("encoder_hidden_states_image: Wan2.1 branch, outside the TI2V-5B path")
        if attention_kwargs is not None:
            attention_kwargs = dict(attention_kwargs)
        # LoRA scale (:463-476): adapters are merged into the weights, a changed scale re-merges them here (frameino_amd/lora.py)
        self._lora_apply(attention_kwargs.pop("scale", None) if attention_kwargs is not None else None)
        self._mx_requantise_if_pending()
        args = (attention_kwargs, timestep_rows, shard, live_rows, id_frames)
        if _active_rows is not None and not self._ras_on:
            raise ValueError("forward(_active_rows=...) is a hook of region-adaptive sampling "
                             "(enable_cache(RegionAdaptiveSamplingConfig(...)) first)")
        if self._faster_on:
            out = yield from self._faster_forward(hidden_states, timestep, encoder_hidden_states, _cache_contexts, args)
        else:
            out = yield from self._forward_stack(hidden_states, timestep, encoder_hidden_states, _cache_contexts, *args,
                                                 active_rows=_active_rows)
        return (out,) if not return_dict else SimpleNamespace(sample=out)

    def _faster_forward(self, hidden_states, timestep, encoder_hidden_states, contexts, args):
        """The forward under FasterCache (frameino_amd/step_cache.py): the unconditional-branch rule around the stack.  A
        computing step runs the stack as without the cache and then takes the delta of the two predictions; a skipping step of
        the batched call runs the stack for the "cond" element alone -- in the batch-2 workspace, its text K / V under a slot of
        their own, its prediction written into row 0 of the result -- and rebuilds row 1; the "uncond" call of a skipping step
        runs nothing but the rebuild.  -> the prediction [b, C, F, H, W]"""
        b = hidden_states.shape[0]
        self._cache_refusals(shard=args[2] if args[2] is not None else self.parallel)      # (before the forward counts)
        fc = self._faster_begin(b, hidden_states.shape[1:], hidden_states.dtype, hidden_states.device, contexts)
        entry = {e.name: e for e in fc.entries}
        if fc.mode == "batched" and fc.skip:
            cond_kv = getattr(self, "_faster_text", None)
            if cond_kv is None or cond_kv[0] is not encoder_hidden_states or cond_kv[1] != encoder_hidden_states._version:
                cond_kv = self._faster_text = (encoder_hidden_states, encoder_hidden_states._version,
                                               encoder_hidden_states[:1].contiguous())
            ts = timestep[:1] if (timestep is not None and timestep.ndim >= 1 and timestep.shape[0] == b) else timestep
            cfg = self.config
            both = torch.empty((2, cfg.out_channels) + tuple(hidden_states.shape[2:]), dtype=hidden_states.dtype,
                               device=hidden_states.device)
            pt, ph, pw = cfg.patch_size
            self._ws_rows_floor = 2 * (hidden_states.shape[2] // pt) * (hidden_states.shape[3] // ph) * (hidden_states.shape[4] // pw)
            try:
                yield from self._forward_stack(hidden_states[:1], ts, cond_kv[2], ("cond",), *args, faster=fc, out_buf=both[0],
                                               text_slot="fastercache-cond")
            finally:
                self._ws_rows_floor = 0
            entry["cond"].state.out, entry["cond"].state.out_i = both[0], entry["cond"].i
            self._faster_rebuild(fc, both[0], out=both[1])
            return both
        if fc.mode == "uncond" and fc.skip:
            cond = (self._step_cache_states or {}).get("cond")
            if cond is None or cond.out is None or cond.out_i != entry["uncond"].i:
                raise RuntimeError(f"FasterCache: forward {entry['uncond'].i} of the \"uncond\" context skips its stack and is rebuilt "
                                   f"from the conditional prediction of the same step, but the \"cond\" context has not run "
                                   f"forward {entry['uncond'].i} (call it first, under cache_context(\"cond\"))")
            return self._faster_rebuild(fc, cond.out)[None]
        out = yield from self._forward_stack(hidden_states, timestep, encoder_hidden_states, contexts, *args, faster=fc)
        if fc.mode == "batched":
            self._faster_pair(entry["cond"], out[0])
            self._faster_pair(entry["uncond"], out[1])
        elif fc.mode is not None:
            self._faster_pair(entry[fc.mode], out[0])
        return out

    def _forward_stack(self, hidden_states, timestep, encoder_hidden_states, _cache_contexts, attention_kwargs, timestep_rows,
                       shard, live_rows, id_frames, faster=None, out_buf=None, text_slot=None, active_rows=None):
        """embedding, blocks and output head of one call (the body of `forward_steps`) -> the prediction [b, C, F, H, W]"""
        c = self._bind(hidden_states, timestep, encoder_hidden_states, attention_kwargs, timestep_rows, shard, live_rows,
                       _cache_contexts, id_frames, faster, out_buf, text_slot, active_rows)
        if c.ras is not None and not c.ras.full:
            return (yield from self._ras_partial(c, hidden_states))        # region-adaptive sampling: the active rows alone
        if c.lite is not None and not any(seg.compute["self"] for seg in c.lite.segs):
            return self._taylor_lite_rows(c, c.ws.po[:c.nr])                      # TaylorSeer, lite mode: the output rows predicted
        self._embed(c, hidden_states)
        if c.tea is not None:
            # TeaCache: block 0's norm1 modulation of h0 against the previous forward's, one host read, the decisions
            self._teacache_probe(c.tea, c.h0, c.mod[:, 0, 0], c.mod[:, 0, 1], c.sel, c.eps)
        yield

        last = len(self.blocks) - 1
        # MagCache / TeaCache: when every segment re-uses its residual the block stack does not run; when some do, it runs on
        # all rows (as under first-block caching) and the skipping segments' rows are overwritten afterwards
        whole = c.mag if c.mag is not None else c.tea
        stack = whole is None or any(seg.compute for seg in whole.segs)
        for li, (blk, e) in enumerate(zip(self.blocks, c.pk.layers) if stack else ()):
            m = c.mod[:, li]                                                      # [R, 6, D] view, row stride = layers*6*D
            if c.live is not None and li == last:
                c.rows, c.segs = c.live, c.live_segs                              # dead rows: keys and values only
            if c.branches is not None:
                self._pab_attention(c, li, blk, e, m)                             # 1. + 2., each computed or re-used
            else:
                if not self._self_attention(c, li, blk, e, m):                    # 1. self-attention (:334-336)
                    self._self_attention_out(c, li, blk, m)
                self._cross_attention(c, li, blk)                                 # 2. cross-attention (:339-341)
            self._ffn(c, li, blk, m)                                              # 3. feed-forward (:344-348)
            if c.fbc is not None and li == 0:
                computes = self._step_cache_probe(c.fbc, c.h0, c.x, c.h1c)        # one host read: the rule's decision
            yield
            if c.fbc is not None and not any(computes):
                break                                                             # every segment skips blocks 1 .. N-1

        if c.fbc is not None:
            # tail residuals of the computed segments; T(tail + h1) for the skipped ones.  With `live_rows` the last block left
            # the dead rows at block N-2's output, so a tail residual is meaningful on the live rows only -- the rows the caller
            # reads; the head below runs on those rows alone whether or not the blocks ran.
            self._step_cache_finish(c.fbc, computes, c.x, c.h1c)
            if c.live is not None:
                c.segs = c.live_segs
        if c.mag is not None:
            # the stack's residual T(x - h0) of the computing segments, T(h0 + r) for the skipping ones; `live_rows` as under
            # first-block caching: the residual is meaningful on the live rows, which are the rows the head runs on
            self._magcache_finish(c.mag, c.x, c.h0)
            if c.live is not None:
                c.segs = c.live_segs
        if c.tea is not None:               # (likewise)
            self._teacache_finish(c.tea, c.x, c.h0)
            if c.live is not None:
                c.segs = c.live_segs
        return self._output_head(c)

    # ------------------------------------------------------------------ forward: per-call state
    def _timestep_selector(self, timestep, timestep_rows, b, n, lo, sharded, dev):
        """The three timestep forms -> (t_rows [R], selector int32 [b * n] or None, same_rows) (F7), cut to the shard's rows and
        repeated over the batch.  `same_rows`: every batch element sees the same modulation rows BY CONSTRUCTION (the selector of
        one element repeated, or one scalar timestep) -- the precondition of the shared prefix."""
        if timestep_rows is not None:
            t_rows, sel = timestep_rows
            if sel is not None and sharded:
                sel = sel[lo:lo + n].contiguous()
            if sel is not None and b > 1:
                sel = sel.repeat(b)
            return t_rows, sel, True
        if timestep.ndim == 2:
            t_rows, inv = torch.unique(timestep.reshape(-1), return_inverse=True)
            sel = inv.to(torch.int32).contiguous()
            if sharded:
                return t_rows, sel[lo:lo + n].contiguous(), False
            if timestep.shape[0] == 1 and b > 1:                                   # one row of per-token values: broadcast
                return t_rows, sel.repeat(b), True
            return t_rows, sel, False
        t_rows = timestep.reshape(-1)
        if b == 1 or t_rows.numel() == 1:
            return t_rows, None, b > 1
        return t_rows, torch.arange(b, device=dev, dtype=torch.int32).repeat_interleave(n), False

    def _bind(self, hidden_states, timestep, encoder_hidden_states, attention_kwargs, timestep_rows, shard, live_rows,
              cache_contexts, id_frames=0, faster=None, out_buf=None, text_slot=None, active_rows=None):
        """Everything the stages of one call share, as a `_Call`: geometry, this rank's token shard, workspace views, RoPE
        tables, modulation tables + selector, text K/V and the switches that pick a path."""
        o, cfg = self.ops, self.config
        pk = self._packed or self._pack()
        default_procs = self._default_processors()
        b, _, nf, hh, ww = hidden_states.shape
        pt, ph, pw = cfg.patch_size
        ppf, pph, ppw = nf // pt, hh // ph, ww // pw
        L = ppf * pph * ppw
        d, heads, dh = self.inner_dim, cfg.num_attention_heads, cfg.attention_head_dim
        dev, dt = hidden_states.device, hidden_states.dtype
        cos1, sin1 = self._rope(ppf, pph, ppw, dev)

        # ---- token shard of this rank (frameino_amd/parallel.py); single GPU: the whole sequence ----
        sh = shard if shard is not None else self.parallel
        sh = sh if (sh is not None and sh.active) else None
        if self._window is not None:             # what window attention refuses, before anything is launched
            self._window_refusals(self.fp8_attention, default_procs, sh)
        if self._sparse is not None:             # ... and what sparse attention refuses
            self._sparse_refusals(self.fp8_attention, default_procs, sh)
        self._cache_refusals(shard=sh, default_procs=default_procs, fp8=self.fp8_attention)      # ... and what the enabled step cache refuses
        lo, n, lpad = 0, L, L
        tk = {}         # the shard's tile height for its GEMM calls (a per-call argument of the C ABI; {} = the library's planner)
        if sh is not None:
            if b != 1:
                raise NotImplementedError("token-sharded execution runs one sample per call")
            lo, n, lpad = sh.rows(L)              # first row, valid rows, padded shard length (equal on all ranks)
            cos1, sin1 = cos1[lo:lo + n].contiguous(), sin1[lo:lo + n].contiguous()
            if sh.gemm_tile_m:
                tk = {"tile_m": sh.tile_m_for(n)}
        # the step cache's places in this forward, each None when it does not sit there: `fbc` around block 0 (first-block
        # caching), `lite` around the whole stack (TaylorSeer's lite mode), `branches` in every block's attention branches,
        # `mag` around the block stack between the embedding and the output head (MagCache), `ras` along the token axis of the
        # whole forward (region-adaptive sampling).
        # Their decisions are taken here, before any launch (a timestep callback is read once)
        policy = self._step_cache_policy
        fbc = lite = branches = mag = tea = ras = None
        if policy is not None:
            ras = policy.ras(self, b, n, d, cfg.out_channels * math.prod(cfg.patch_size), dt, dev, cache_contexts,
                             _live_range(live_rows, n), active_rows)
            fbc = policy.segments(self, b, n, cache_contexts)
            mag = policy.magcache(self, b, n, d, dt, dev, cache_contexts)        # MagCache: around the whole block stack
            tea = policy.teacache(self, b, n, d, dt, dev, cache_contexts)        # TeaCache: likewise, decided after the embedding
            lite = policy.lite(self, b, n, cfg.out_channels * math.prod(cfg.patch_size), dt, dev, cache_contexts)
            if lite is not None and not any(seg.compute["self"] for seg in lite.segs):
                # every segment predicts: no embedding, no block, no head -- the call needs its geometry and the output rows
                return _Call(b=b, n=n, nr=b * n, L=L, nf=nf, hh=hh, ww=ww, d=d, dev=dev, dt=dt, sh=None,
                             ws=self._workspace(b * lpad, dt, dev), lite=lite, live=None, segs=[(0, b * n)], out_buf=None)
            branches = policy.branches(self, b, n, d, dt, dev, cache_contexts, faster)
        # Batch elements are extra ROWS of the token-major buffers ([B*n, D]): every GEMM / norm is one launch over
        # both CFG branches (twice the tiles per launch, weights read once); attention and RoPE index rows per batch.
        nr = b * n
        ws = self._workspace(b * lpad, dt, dev)
        cos, sin = cos1, sin1
        if b > 1:
            key = ("rope_b", ppf, pph, ppw, b, str(dev))
            if key not in self._rope_cache:
                self._rope_cache[key] = (cos1.repeat(b, 1).contiguous(), sin1.repeat(b, 1).contiguous())
            cos, sin = self._rope_cache[key]

        t_rows, sel, same_rows = self._timestep_selector(timestep, timestep_rows, b, n, lo, sh is not None, dev)
        temb, tproj = self._time_rows(t_rows.to(dev), encoder_hidden_states.dtype)       # [R,D], [R,6,D]
        # per-layer modulation tables: scale_shift_table + temb.float()  (:317-319)  -> [R, layers, 6, D] fp32
        mod = (pk.sst[None] + tproj.float()[:, None]).contiguous()
        head = (self.scale_shift_table.float() + temb.float()[:, None]).contiguous()     # [R, 2, D]  (:522/:527)
        text = self._text_kv(encoder_hidden_states, pk, lq=n, may_fold=default_procs, slot=text_slot)   # (token shards too: n = the shard's rows)

        # `shared`: the batch elements are the SAME latent (the pipeline's CFG-batched call passes x.expand(2, ...)) under
        # the same timestep rows: everything up to the first text cross-attention is identical for them, so the patch
        # embedding and layer 0's self-attention branch run once and their result is copied (exactly what each element
        # would have computed).  A per-sample timestep ([b] or [b, L] values) takes the general path.
        # (Pyramid Attention Broadcast keeps one cache per context and layer: every element runs block 0's branch itself)
        shared = (self.dedup_shared_prefix and b > 1 and sh is None and hidden_states.stride(0) == 0 and default_procs
                  and same_rows and branches is None and ras is None)
        fold = self.fold_softmax_scale
        fp8 = self.fp8_attention and sh is None and hasattr(o, "attention_fp8")     # this call's self-attention takes fp8 operands
        # sliding-window self-attention over frames: this forward's decision (the timestep callback is read here, once)
        win = self._window_begin(ppf, pph * ppw, 0, id_frames, dev)
        # dynamic block-sparse self-attention: the always-kept tiles, the mask buffer and the plan workspace of this forward
        sp = self._sparse_begin(ppf, pph * ppw, id_frames, dev, ws, b, heads, dh)
        # rows whose output the caller reads (`live_rows`): honoured in the last block on the single-GPU default-processor path
        live = None
        # (not under Pyramid Attention Broadcast: a cached branch output covers every row, so that any later step may use it)
        if (live_rows is not None and self.skip_dead_rows and default_procs and sh is None and len(self.blocks) > 1
                and not self._fp8 and not fp8 and branches is None and lite is None
                and not (mag is not None and mag.calibrate)        # (a calibrating MagCache run measures every row's full stack)
                and not (tea is not None and tea.calibrate)):      # (... and a calibrating TeaCache run every row of the head)
            l0, l1 = int(live_rows[0]), int(live_rows[1])
            if 0 <= l0 < l1 <= n and (l1 - l0) < n:
                live = (l0, l1)
        # (a per-row or per-batch field added here needs its one-element view in `_Call.element`: Pyramid Attention Broadcast
        # runs a batch's attention branches through it)
        return _Call(b=b, n=n, nr=nr, lo=lo, lpad=lpad, L=L, nf=nf, hh=hh, ww=ww, d=d, heads=heads, dh=dh, dev=dev, dt=dt,
                     eps=cfg.eps, sh=sh, tk=tk, pk=pk, ws=ws, x=ws.x[:nr], nrm=ws.n[:nr], att=ws.att[:nr], q2=ws.q2[:nr],
                     ff=ws.ff[:nr], qkv=ws.qkv[:nr], cos=cos, sin=sin, cos1=cos1, sin1=sin1, sel=sel, mod=mod, head=head,
                     text=text, qfold={"out_scale": dh ** -0.5 * o.LOG2E} if fold else {},
                     afold={"scale": o.SCALE_FOLDED} if fold else {}, fp8=fp8, default_procs=default_procs,
                     shared=shared, fbc=fbc, branches=branches, keep=None, h0=None, h1c=None, attention_kwargs=attention_kwargs,
                     live=live, win=win, sp=sp, lite=lite, mag=mag, tea=tea, ras=ras, out_buf=out_buf,
                     live_segs=live and [(bi * n + live[0], bi * n + live[1]) for bi in range(b)],
                     rows=(0, n),            # the rows of every batch element that run as queries / per-token rows ...
                     segs=[(0, nr)])         # ... and the global row ranges the per-token operations of a block run on

    # ------------------------------------------------------------------ forward: stages
    def _embed(self, c, hidden_states):
        """patch embedding (:486-487): gather + GEMM (the gather is 9 MB; every rank builds it, keeps its rows); under the
        shared prefix one element's rows only (x[:n]); with the first-block cache h0 is kept aside (block 0 updates x in place)."""
        o, x, b, n = self.ops, c.x, c.b, c.n
        patch = self.config.patch_size
        if b == 1 or c.shared:
            a_rows = o.patchify(hidden_states[0], patch)[c.lo:c.lo + n]
        else:
            a_rows = torch.cat([o.patchify(hidden_states[i], patch) for i in range(b)])
        o.gemm(a_rows, c.pk.w_patch, self.patch_embedding.bias, out=x[:n] if c.shared else x, **c.tk)
        if c.fbc is not None or c.mag is not None or c.tea is not None:
            ws = c.ws                        # h0, and a buffer for the probe's copy of h1 (MagCache and TeaCache keep h0 alone)
            if getattr(ws, "fbc_h0", None) is None:
                ws.fbc_h0 = torch.empty_like(ws.x)
            if c.fbc is not None and getattr(ws, "fbc_h1", None) is None:
                ws.fbc_h1 = torch.empty_like(ws.x)
            c.h0, c.h1c = ws.fbc_h0[:c.nr], (ws.fbc_h1[:c.nr] if c.fbc is not None else None)
            if c.shared:                     # (the embedding of the shared latent sits in the first n rows only)
                for bi in range(b):
                    c.h0[bi * n:(bi + 1) * n].copy_(x[:n])
            else:
                c.h0.copy_(x)

    def _self_attention(self, c, li, blk, e, m):
        """Block li's self-attention branch (:334-336) by the strategy this call takes.  -> True when the strategy has already
        added the branch to x; False when its result waits in `att` for `_self_attention_out`."""
        sh = c.sh
        if not c.default_procs:                       # a processor the user installed, through the plugin protocol
            if sh is not None:
                raise NotImplementedError("token-sharded execution needs the built-in MI355WanAttnProcessor")
            return self._sa_processors(c, blk, m)
        if c.ras is not None:                         # region-adaptive sampling: K and V kept in / read from the planes
            return self._sa_ras(c, li, blk, e, m)
        if c.shared and li == 0:                      # CFG batch of one latent: block 0's branch once, copied
            return self._sa_shared_prefix(c, li, blk, e, m)
        if sh is None:                                # one GPU
            return self._sa_single(c, li, blk, e, m)
        self.ops.adaln_modulate(c.x, m[:, 0], m[:, 1], c.sel, c.eps, out=c.nrm)
        if sh.heads_exchange_ok(c.heads):             # token shards <-> head shards by all-to-all
            return self._sa_heads_exchange(c, li, blk, e, m)
        if sh.kv_groups(c.heads) > 1:                 # K|V all-gather in head groups
            return self._sa_kv_head_groups(c, li, blk, e)
        return self._sa_kv_gather(c, li, blk, e)      # K|V all-gather, one attention pass or local-first partials

    def _sa_processors(self, c, blk, m):
        o = self.ops
        o.adaln_modulate(c.x, m[:, 0], m[:, 1], c.sel, c.eps, out=c.nrm)
        a = blk.attn1(c.nrm.view(c.b, c.n, c.d), rotary_emb=_CompactRope((c.cos1, c.sin1)), **(c.attention_kwargs or {}))
        _keep_copy(c, a.reshape(c.nr, c.d))
        o.gated_residual(c.x, a.reshape(c.nr, c.d), m[:, 2], c.sel, out=c.x)
        return True

    def _sa_shared_prefix(self, c, li, blk, e, m):
        """the whole branch, out-projection included, on the first element's rows; the other elements get a copy of x"""
        o, n, d, x, to_out = self.ops, c.n, c.d, c.x, blk.attn1.to_out[0]
        n1, q1, a1, sel1 = c.nrm[:n], c.qkv[:n], c.att[:n], _sel_rows(c.sel, 0, n)
        o.adaln_modulate(x[:n], m[:, 0], m[:, 1], sel1, c.eps, out=n1)
        self._lin(li, "qkv", n1, e.wqkv, e.bqkv, out=q1)
        self._qk_norm_rope(blk, q1, d, c.cos1, c.sin1, c.dh, c.qfold)
        q3 = q1.view(1, n, 3 * d)
        self._attend(o, q3[:, :, :d], q3[:, :, d:2 * d], q3[:, :, 2 * d:], c.heads, fp8=c.fp8,
                     ranges=self._window_ranges(c.win, li, (0, n)), tiles=self._sparse_tiles(c.sp, li, (0, n)),
                     out=a1.view(1, n, d), **c.afold)
        self._lin(li, "out", a1, to_out.weight, to_out.bias, o.EPI_GATED_RESIDUAL, residual=x[:n], gate=m[:, 2], sel=sel1,
                  out=x[:n])
        for bi in range(1, c.b):
            x[bi * n:(bi + 1) * n].copy_(x[:n])
        return True

    def _sa_single(self, c, li, blk, e, m):
        o, b, n, d = self.ops, c.b, c.n, c.d
        xq = self._ln_q(li, "qkv", 0, c.x, shift=m[:, 0], scale=m[:, 1], sel=c.sel, eps=c.eps)
        if xq is None:
            o.adaln_modulate(c.x, m[:, 0], m[:, 1], c.sel, c.eps, out=c.nrm)
        self._lin(li, "qkv", c.nrm, e.wqkv, e.bqkv, xq=xq, out=c.qkv)
        self._qk_norm_rope(blk, c.qkv, d, c.cos, c.sin, c.dh, c.qfold)
        q3 = c.qkv.view(b, n, 3 * d)
        s0, s1 = c.rows                  # every row is a key; under `live_rows` only the live rows of the last block are queries
        self._attend(o, q3[:, s0:s1, :d], q3[:, :, d:2 * d], q3[:, :, 2 * d:], c.heads, fp8=c.fp8,
                     ranges=self._window_ranges(c.win, li, (s0, s1)), tiles=self._sparse_tiles(c.sp, li, (s0, s1)),
                     out=c.att.view(b, n, d)[:, s0:s1], **c.afold)
        return False

    def _sa_heads_exchange(self, c, li, blk, e, m):
        """heads exchange (frameino_amd/parallel.py): q | k | v of MY tokens -> all-to-all -> all tokens of MY heads -> one
        attention launch over the whole sequence -> all-to-all back to the token owners.  -> whether the out-projection ran here."""
        o, sh, n, L, lpad, heads, dh, dt, dev = self.ops, c.sh, c.n, c.L, c.lpad, c.heads, c.dh, c.dt, c.dev
        ways = sh.ways
        hp = heads // ways
        self._lin(li, "qkv", c.nrm, e.wqkv, e.bqkv, out=c.qkv, **c.tk)
        # the heads travel in groups, every group its own all-to-all on the communicator's stream: while group g is attended
        # to, group g+1 arrives and group g-1's outputs leave.  ONE launch: RMSNorm + RoPE write q and k straight into the send
        # buffers (slice j: heads of rank j) and v follows as a scattering copy -- no permute copy of q | k | v afterwards
        lay = sh.heads_send_layout(heads, dh, lpad, dt, dev)
        self._qk_norm_rope(blk, c.qkv, c.d, c.cos, c.sin, dh, c.qfold, out=lay.flat, head_off=lay.off_qkv, head_ld=lay.ld)
        inflight = [(gi, h0, h1, (h1 - h0) * dh) + sh.all_to_all(f"qkv_recv{gi}", lay.views[gi], async_op=True)
                    for gi, (h0, h1) in enumerate(sh.head_ranges(hp))]
        # the outputs return into ONE flat [group][rank j's heads][token] buffer when the groups are equal: the
        # out-projection then reads it as K blocks (fino_gemm_blocked_a) instead of a permute copy into [token, D]
        orl = sh.heads_recv_layout(heads, dh, lpad, dt, dev) if not self._fp8 else None
        back = []
        for gi, h0, h1, dg, recv, work in inflight:                                # slice j: tokens of rank j
            if work is not None:
                work.wait()
            r3 = recv.view(1, ways * lpad, 3 * dg)[:, :L]
            oh = sh.a2a_buffer(f"o_send{gi}", (ways, lpad, dg), dt, dev)
            o.attention(r3[:, :, :dg], r3[:, :, dg:2 * dg], r3[:, :, 2 * dg:], h1 - h0,
                        out=oh.view(1, ways * lpad, dg)[:, :L], **c.afold)
            back.append((h0, h1) + sh.all_to_all(f"o_recv{gi}", oh, async_op=True))
        blocked = orl is not None and all(orv.data_ptr() == orl[gi].data_ptr() for gi, (_, _, orv, _) in enumerate(back))
        a3 = c.att.view(n, ways, hp * dh)
        for h0, h1, orv, work in back:                                             # slice j: heads of rank j
            if work is not None:
                work.wait()
            if not blocked:              # MX linears, or unequal groups: the permute copy into [token, D]
                a3[:, :, h0 * dh:h1 * dh].copy_(orv[:, :n].permute(1, 0, 2))
        if blocked:
            to_out = blk.attn1.to_out[0]
            o.gemm_blocked_a(orl, n, to_out.weight, to_out.bias, c.x, m[:, 2], c.sel, out=c.x, **c.tk)
        return blocked

    def _project_kv(self, c, li, e, fused):
        """k | v of the shard's rows into the all-gather's send buffer `kv_loc`.  `fused`: ONE q | k | v GEMM whose k | v
        columns land there (fino_gemm_split_n) -- the interleaved plan, where the OTHER branch's compute is what the gather
        flies under; else K|V alone first, so that their all-gather (RCCL over xGMI) overlaps the Q projection (`_project_q`)."""
        kv_loc = c.sh.kv_local(c.lpad, 2 * c.d, c.dt, c.dev)
        if fused:
            self.ops.gemm(c.nrm, e.wqkv, e.bqkv, out=c.q2, out2=kv_loc[:c.n], split=c.d, **c.tk)
        else:
            self._lin(li, "kv", c.nrm, e.wqkv[c.d:], e.bqkv[c.d:], out=kv_loc[:c.n], **c.tk)
        return kv_loc

    def _project_q(self, c, li, blk, e, fused):
        """q (its projection unless the fused GEMM made it) + norm_q + RoPE, in `q2`"""
        if not fused:
            self._lin(li, "q", c.nrm, e.wqkv[:c.d], e.bqkv[:c.d], out=c.q2, **c.tk)
        self.ops.rmsnorm_rope_(c.q2, blk.attn1.norm_q.weight, blk.attn1.norm_q.eps, c.cos, c.sin, c.dh, **c.qfold)

    def _sa_kv_head_groups(self, c, li, blk, e):
        """K|V all-gather in HEAD GROUPS (TokenShard.kv_head_groups): the attention of group g runs while group g+1 is still on
        the wire.  k (norm_k + RoPE) is scattered by head into [group][token][k_g | v_g] send blocks, v follows as a scattering
        copy; per group one all-gather and one attention launch over that group's heads."""
        o, sh, n, d, dh, nk = self.ops, c.sh, c.n, c.d, c.dh, blk.attn1.norm_k
        fused = sh.fused_qkv_ok() and not self._fp8
        kv_loc = self._project_kv(c, li, e, fused)
        lay = sh.kv_group_layout(c.heads, dh, c.lpad, c.dt, c.dev)
        o.rmsnorm_rope_scatter(kv_loc[:n, :d], nk.weight, nk.eps, c.cos, c.sin, dh, lay.flat, lay.off_k, lay.ld)
        o.rmsnorm_rope_scatter(kv_loc[:n, d:], None, 0.0, None, None, dh, lay.flat, lay.off_v, lay.ld)
        flying = [sh._all_gather(f"kv_all_g{gi}", v_, True) for gi, v_ in enumerate(lay.views)]
        self._project_q(c, li, blk, e, fused)
        q3, a3 = c.q2.view(1, n, d), c.att.view(1, n, d)
        for (h0, h1), (kv_all, work) in zip(lay.ranges, flying):
            if work is not None:
                work.wait()
            dg = (h1 - h0) * dh
            kv3 = kv_all.view(1, -1, 2 * dg)[:, :c.L]
            o.attention(q3[:, :, h0 * dh:h1 * dh], kv3[:, :, :dg], kv3[:, :, dg:], h1 - h0, out=a3[:, :, h0 * dh:h1 * dh],
                        **c.afold)
        return False

    def _sa_kv_gather(self, c, li, blk, e):
        """K|V all-gather: one attention launch over the gathered keys, or (TokenShard.local_first) the local keys first."""
        o, sh, n, d, dh, heads, lo, L, nk = self.ops, c.sh, c.n, c.d, c.dh, c.heads, c.lo, c.L, blk.attn1.norm_k
        fused = sh.fused_qkv_ok() and not self._fp8
        kv_loc = self._project_kv(c, li, e, fused)
        o.rmsnorm_rope_(kv_loc[:n, :d], nk.weight, nk.eps, c.cos, c.sin, dh)
        kv_all, work = sh.all_gather_kv(kv_loc)
        self._project_q(c, li, blk, e, fused)
        qv, av = c.q2.view(1, n, d), c.att.view(1, n, d)
        if not sh.local_first():
            if work is not None:
                work.wait()
            kv3 = kv_all.view(1, -1, 2 * d)[:, :L]
            o.attention(qv, kv3[:, :, :d], kv3[:, :, d:], heads, out=av, **c.afold)
            return False
        # local keys first -- nothing of it waits for the wire -- then what the gather delivered before / after the own
        # chunk; the (O, m, l) partials are merged (same softmax up to fp32 summation order)
        pf = o.attention_partial_floats(1, heads, n, dh) if hasattr(o, "attention_partial_floats") else 0
        parts = [o.attention_partial(qv, kv_loc[:n, :d][None], kv_loc[:n, d:][None], heads, out=sh.partial_buf(0, pf, c.dev),
                                     **c.afold)]
        if work is not None:
            work.wait()
        kv3 = kv_all.view(1, -1, 2 * d)
        for pi, (k0, k1) in enumerate(((0, lo), (lo + c.lpad, L))):
            if k1 > k0:
                parts.append(o.attention_partial(qv, kv3[:, k0:k1, :d], kv3[:, k0:k1, d:], heads,
                                                 out=sh.partial_buf(1 + pi, pf, c.dev), **c.afold))
        o.attention_merge(parts, 1, n, heads, dh, c.dt, out=av)
        return False

    def _self_attention_out(self, c, li, blk, m):
        """x += gate * to_out(att) on the rows that run (:336, the gated residual as the GEMM's epilogue)"""
        to_out = blk.attn1.to_out[0]
        for r0, r1 in c.segs:
            self._lin(li, "out", c.att[r0:r1], to_out.weight, to_out.bias, self.ops.EPI_GATED_RESIDUAL, residual=c.x[r0:r1],
                      gate=m[:, 2], sel=_sel_rows(c.sel, r0, r1), out=c.x[r0:r1], **c.tk, **_keep_kw(c, r0, r1))

    def _cross_attention(self, c, li, blk):
        """text cross-attention (:339-341): text K/V are replicated, nothing to exchange"""
        o, x, nrm, q2, att, segs, text = self.ops, c.x, c.nrm, c.q2, c.att, c.segs, c.text
        b, n, d, heads, n2, a2 = c.b, c.n, c.d, c.heads, blk.norm2, blk.attn2
        xq = self._ln_q(li, "q2", 1, x, weight=n2.weight, bias=n2.bias, eps=c.eps) if (n2 is not None
                                                                                       and c.default_procs) else None
        if xq is None and n2 is not None:
            for r0, r1 in segs:
                o.layernorm(x[r0:r1], n2.weight, n2.bias, c.eps, out=nrm[r0:r1])
        elif xq is None:
            nrm.copy_(x)
        if not c.default_procs:
            a = a2(nrm.view(b, n, d), encoder_hidden_states=text.txt.view(b, text.lt, d), **(c.attention_kwargs or {}))
            _keep_copy(c, a.reshape(c.nr, d))
            o.gated_residual(x, a.reshape(c.nr, d), out=x)
            return
        for r0, r1 in segs:
            self._lin(li, "q2", nrm[r0:r1], a2.to_q.weight, a2.to_q.bias, xq=xq, out=q2[r0:r1], **c.tk)
        kv = text.kv[li].view(b, text.lt, 2 * d)
        s0, s1 = c.rows
        if text.w2 is not None:
            # norm_q's statistic only (the probabilities kernel normalises q while it loads it: same rounding points, no
            # pass that rewrites q); probabilities per sample, then x += P.(V W_o^T) + b: K = heads x keys instead of D
            rr = text.rrms
            for r0, r1 in segs:
                o.row_rrms(q2[r0:r1], a2.norm_q.eps, out=rr[r0:r1])
            for i in range(b):
                r0, r1 = i * n + s0, i * n + s1
                pr = o.attention_probs(q2[r0:r1].view(1, s1 - s0, d), kv[i:i + 1, :, :d], heads, text.tail[0][i:i + 1],
                                       text.tail[1][i:i + 1], text.kp[i], out=text.pbuf[i][:s1 - s0].view(1, s1 - s0, -1),
                                       q_rrms=rr[r0:r1].view(1, s1 - s0), q_weight=a2.norm_q.weight)
                xi = x[r0:r1]
                o.gemm(pr.view(s1 - s0, -1), text.w2[li][i], a2.to_out[0].bias, o.EPI_RESIDUAL, residual=xi, out=xi, **c.tk,
                       **_keep_kw(c, r0, r1))
            return
        for r0, r1 in segs:
            o.rmsnorm_rope_(q2[r0:r1], a2.norm_q.weight, a2.norm_q.eps)
        qv, av = q2.view(b, n, d)[:, s0:s1], att.view(b, n, d)[:, s0:s1]
        if text.tail is not None:
            o.attention_tail(qv, kv[:, :, :d], kv[:, :, d:], heads, text.tail[0], text.tail[1], out=av)
        else:
            o.attention(qv, kv[:, :, :d], kv[:, :, d:], heads, out=av)
        for r0, r1 in segs:
            self._lin(li, "out2", att[r0:r1], a2.to_out[0].weight, a2.to_out[0].bias, o.EPI_RESIDUAL, residual=x[r0:r1],
                      out=x[r0:r1], **c.tk, **_keep_kw(c, r0, r1))

    # ------------------------------------------------------------------ forward: region-adaptive sampling
    def _ras_buffers(self, c):
        """the state's device buffers, allocated by its first forward: per layer the planes K | V [2, b * n, D], the kept head
        rows po [b * n, C_out], the sit-out counters, the scores and the list"""
        st, nr = c.ras.state, c.nr
        if st.planes is None:
            mk = lambda *s, dtype=c.dt: torch.empty(*s, dtype=dtype, device=c.dev)          # noqa: E731
            st.planes = [mk(2, nr, c.d) for _ in self.blocks]
            st.po = mk(nr, c.ws.po.shape[1])
            st.counters = torch.zeros(c.n, dtype=torch.int32, device=c.dev)
            st.score = mk(c.n, dtype=torch.float32)
        return st

    def _sa_ras(self, c, li, blk, e, m):
        """`_sa_single` under region-adaptive sampling.  A full forward: the same launches, the norm + RoPE stage also writing
        every row's k and v into layer li's planes (q | k | v of the attention still read in place: the bits of the uncached
        forward).  A partial forward (`c` = the compact call): the projection of the active rows alone, their k and v written
        over their rows of the planes, and q at lq = La against all n rows of the planes."""
        o, b, n, d, ras, a = self.ops, c.b, c.n, c.d, c.ras, blk.attn1
        st = self._ras_buffers(c) if ras.full else ras.state
        xq = self._ln_q(li, "qkv", 0, c.x, shift=m[:, 0], scale=m[:, 1], sel=c.sel, eps=c.eps)
        if xq is None:
            o.adaln_modulate(c.x, m[:, 0], m[:, 1], c.sel, c.eps, out=c.nrm)
        self._lin(li, "qkv", c.nrm, e.wqkv, e.bqkv, xq=xq, out=c.qkv)
        kp, vp = st.planes[li][0], st.planes[li][1]
        o.qkv_rmsnorm_rope_rows_(c.qkv, d, a.norm_q.weight, a.norm_q.eps, a.norm_k.weight, a.norm_k.eps, c.cos, c.sin, c.dh,
                                 ras.idx, kp, vp, q_out_scale=c.qfold.get("out_scale", 1.0))
        q3 = c.qkv.view(b, n, 3 * d)
        if ras.full:
            s0, s1 = c.rows
            o.attention(q3[:, s0:s1, :d], q3[:, :, d:2 * d], q3[:, :, 2 * d:], c.heads, out=c.att.view(b, n, d)[:, s0:s1], **c.afold)
        else:
            o.attention(q3[:, :, :d], kp.view(b, -1, d), vp.view(b, -1, d), c.heads, out=c.att.view(b, n, d), **c.afold)
        return False

    def _ras_partial(self, c, hidden_states):
        """A partial forward of region-adaptive sampling (`c`: the call as `_bind` made it, over all rows).  The list -- from the
        kept head rows (ops.token_score + ops.token_select; one list per call, from the batch-averaged score) or the caller's
        `_active_rows` --, then patches, cos / sin and selector rows gathered by it, every stage on the compact [b * La, D]
        buffers (the first rows of the workspace), the head's rows scattered into the kept `po`, and the whole `po` unpatchified:
        a row that did not run returns the prediction of the last forward that computed it."""
        o, ras, st, b, n, d = self.ops, c.ras, c.ras.state, c.b, c.n, c.d
        la = ras.rows
        if ras.override is not None:
            idx1 = ras.override
        else:
            if st.idx is None or st.idx.shape[0] != la:
                st.idx = torch.empty(la, dtype=torch.int32, device=c.dev)
            o.token_score(st.po, batch=b, counters=st.counters, starvation_scale=float(ras.cfg.starvation_scale),
                          eligible=st.eligible, out=st.score)
            idx1 = o.token_select(st.score, la, counters=st.counters, out=st.idx)
        ras.idx = idx = idx1 if b == 1 else torch.cat([idx1 + i * n for i in range(b)])       # rows of the [b * n, .] buffers
        nra, ws, patch = b * la, c.ws, self.config.patch_size
        patches = (o.patchify(hidden_states[0], patch) if b == 1 else
                   torch.cat([o.patchify(hidden_states[i], patch) for i in range(b)]))
        x = ws.x[:nra]
        o.gemm(o.gather_rows(patches, idx, out=ws.a[:nra]), c.pk.w_patch, self.patch_embedding.bias, out=x)
        fields = {k: getattr(c, k) for k in c.__slots__ if k != "elements"}
        fields.update(n=la, nr=nra, L=la, x=x, nrm=ws.n[:nra], att=ws.att[:nra], q2=ws.q2[:nra], ff=ws.ff[:nra], qkv=ws.qkv[:nra],
                      cos=o.gather_rows(c.cos, idx), sin=o.gather_rows(c.sin, idx), cos1=None, sin1=None,
                      sel=None if c.sel is None else o.gather_rows(c.sel.view(-1, 1), idx).view(-1),
                      shared=False, live=None, live_segs=None, rows=(0, la), segs=[(0, nra)])
        cc = _Call(**fields)
        yield
        for li, (blk, e) in enumerate(zip(self.blocks, c.pk.layers)):
            m = c.mod[:, li]
            self._sa_ras(cc, li, blk, e, m)
            self._self_attention_out(cc, li, blk, m)
            self._cross_attention(cc, li, blk)
            self._ffn(cc, li, blk, m)
            yield
        o.adaln_modulate(x, c.head[:, 0], c.head[:, 1], cc.sel, c.eps, out=cc.nrm)
        rows = o.gemm(cc.nrm, self.proj_out.weight, self.proj_out.bias, out=ws.po[:nra])
        o.scatter_rows(rows, idx, st.po)
        return self._unpatchify(c, st.po)

    # ------------------------------------------------------------------ forward: Pyramid Attention Broadcast
    def _pab_attention(self, c, li, blk, e, m):
        """Block li's two attention branches under a cache that has taken them over (`c.branches`: this forward's decisions per
        row segment and kind, a `_BranchPlan` of frameino_amd/step_cache.py -- Pyramid Attention Broadcast, TaylorSeer's default
        mode or FasterCache's self-attention part; the plan knows which, this loop does not).
        Compute: the launches of `_self_attention` / `_self_attention_out` / `_cross_attention`, the closing GEMM with `keep=`
        into the buffer the plan names (`c.keep`; a custom processor's return value is copied there), then what the plan runs
        on that y.  Re-use: none of the branch runs; the plan's one launch adds the cached or extrapolated y to the residual
        stream with the closing GEMM's epilogue arithmetic.  A kind that is not hooked runs as without the cache.  The elements
        of a batch (the CFG branches of a batched call: one context and one buffer each, and counters that may differ) take a
        hooked branch one by one, each on a one-element view of the call: per row the launches compute what the batched ones do."""
        plan, n, o = c.branches, c.n, self.ops
        stages = (("self", blk.attn1, lambda cc: self._self_attention(cc, li, blk, e, m) or self._self_attention_out(cc, li, blk, m)),
                  ("cross", blk.attn2, lambda cc: self._cross_attention(cc, li, blk)))
        for kind, module, run in stages:
            if not plan.hooked[kind]:
                run(c)
                continue
            for i in range(c.b):
                # the segment element i's rows lie in: its own (one context per element), or the joint one of a batch under one
                # context -- one decision, one [b * n, D] buffer, of which the element takes its rows
                r0, r1 = i * n, (i + 1) * n
                seg = plan.segment(r0)
                if not seg.compute[kind]:
                    gate, sel = (m[:, 2], _sel_rows(c.sel, r0, r1)) if kind == "self" else (None, None)
                    plan.reuse(o, seg, kind, li, r0, r1, c.x[r0:r1], gate, sel, module=module, fused=c.default_procs)
                    continue
                cc = c if c.b == 1 else c.element(i)
                y = plan.kept(c.ws, seg, kind, li, r0, r1)
                cc.keep = {(0, n): y}
                try:
                    run(cc)
                finally:
                    cc.keep = None
                plan.computed(o, seg, kind, li, r0, r1, y)

    def _taylor_lite_rows(self, c, po):
        """TaylorSeer in lite mode on the output head's rows `po` [b * n, C_out * prod(patch)]: a computing segment's rows
        update its factors, a predicting segment's rows are overwritten by T(p); then unpatchify"""
        o, lite = self.ops, c.lite
        for seg in lite.segs:
            if seg.compute["self"]:
                o.taylor_update(po[seg.r0:seg.r1], self._taylor_buffer(lite, seg, "out", po.shape[1], c.dev), seg.n_old, seg.k,
                                seg.n_new)
            else:
                o.taylor_predict(self._taylor_buffer(lite, seg, "out"), seg.n_old, seg.k, out=po[seg.r0:seg.r1])
        return self._unpatchify(c, po)

    def _ffn(self, c, li, blk, m):
        """feed-forward (:344-348)"""
        o, x, nrm, ff, sel = self.ops, c.x, c.nrm, c.ff, c.sel
        up, down = blk.ffn.net[0].proj, blk.ffn.net[2]
        xq = self._ln_q(li, "ff1", 0, x, shift=m[:, 3], scale=m[:, 4], sel=sel, eps=c.eps) if (li, "ff2") in self._fp8 else None
        if xq is None:
            for r0, r1 in c.segs:
                o.adaln_modulate(x[r0:r1], m[:, 3], m[:, 4], _sel_rows(sel, r0, r1), c.eps, out=nrm[r0:r1])
        # MXFP8: the adaLN emits the FFN input already quantised, and the GELU epilogue the hidden activations
        if self._ffn_mxfp8(li, nrm, xq, up.bias, down.bias, o.EPI_GATED_RESIDUAL, residual=x, gate=m[:, 5], sel=sel,
                           out=x) is None:
            for r0, r1 in c.segs:
                self._lin(li, "ff1", nrm[r0:r1], up.weight, up.bias, o.EPI_GELU_TANH, out=ff[r0:r1], **c.tk)
                self._lin(li, "ff2", ff[r0:r1], down.weight, down.bias, o.EPI_GATED_RESIDUAL, residual=x[r0:r1], gate=m[:, 5],
                          sel=_sel_rows(sel, r0, r1), out=x[r0:r1], **c.tk)

    def _output_head(self, c):
        """output head (:519-543): modulated norm, proj_out, unpatchify -> [b, C_out, F, H, W]"""
        o, nrm, sh = self.ops, c.nrm, c.sh
        for r0, r1 in c.segs:
            o.adaln_modulate(c.x[r0:r1], c.head[:, 0], c.head[:, 1], _sel_rows(c.sel, r0, r1), c.eps, out=nrm[r0:r1])
        if sh is None:
            po = c.ws.po[:c.nr]
            if c.live is not None:
                po.zero_()               # rows nobody computed: the caller asked not to read them -- zeros, not the last call's values
            for r0, r1 in c.segs:
                o.gemm(nrm[r0:r1], self.proj_out.weight, self.proj_out.bias, out=po[r0:r1])
        else:
            po_loc = sh.out_local(c.lpad, c.ws.po.shape[1], c.dt, c.dev)
            o.gemm(nrm, self.proj_out.weight, self.proj_out.bias, out=po_loc[:c.n], **c.tk)
            po = sh.all_gather_out(po_loc)[:c.L]
        if c.lite is not None:
            return self._taylor_lite_rows(c, po)
        if c.tea is not None:                # TeaCache: a calibrating run measures the head's rows; a finished context starts over
            self._teacache_head(c.tea, po)
        if c.ras is not None:                # a full forward under region-adaptive sampling keeps the head's rows
            st = c.ras.state
            st.po.copy_(po)
            st.counters.zero_()
            st.valid = True
        return self._unpatchify(c, po)

    def _unpatchify(self, c, po):
        o, cfg = self.ops, self.config
        unpatch = lambda rows: o.unpatchify(rows, cfg.out_channels, c.nf, c.hh, c.ww, cfg.patch_size)      # noqa: E731
        if c.b == 1:
            if c.out_buf is not None:                # (FasterCache: row 0 of the batched call's result)
                return o.unpatchify(po, cfg.out_channels, c.nf, c.hh, c.ww, cfg.patch_size, out=c.out_buf)[None]
            return unpatch(po)[None]
        po3 = po.view(c.b, c.L, -1)
        return torch.stack([unpatch(po3[i]) for i in range(c.b)])


class _Call:
    """What the stages of one `WanTransformer3DModel.forward_steps` call share (built by `_bind` at the first `next()`): sizes,
    the token shard, views of the workspace, tables and the switches that pick a path.  References and views only: nothing on
    the device the call would not hold anyway.  `rows` / `segs` (set for the last block under `live_rows`), `h0` / `h1c`
    (the first-block cache's buffers, set by the embedding stage) and `keep` around a branch that a step cache computes
    ({(first row, end row): the buffer that also receives the closing GEMM's y}; `elements`: the one-element views it runs a
    batch through) are the only fields written after `_bind`.  `branches`: the plan of the cache that has taken over the
    attention branches (`_BranchPlan`: Pyramid Attention Broadcast, TaylorSeer's default mode, FasterCache's self-attention
    part), else None; `lite`: the plan of TaylorSeer's lite mode -- when every segment of it predicts, `_bind` returns a call
    with the geometry, the workspace and the plan alone; `mag`: MagCache's plan for the block stack as a whole (`h0` is then
    the stack's input, kept by the embedding stage); `tea`: TeaCache's, whose decisions are taken after the embedding stage; `ras`: the plan of region-adaptive sampling -- a partial forward runs on
    a second `_Call` over the compact rows (`_ras_partial`)."""
    __slots__ = ("b", "n", "nr", "lo", "lpad", "L", "nf", "hh", "ww", "d", "heads", "dh", "dev", "dt", "eps", "sh", "tk", "pk",
                 "ws", "x", "nrm", "att", "q2", "ff", "qkv", "cos", "sin", "cos1", "sin1", "sel", "mod", "head", "text", "qfold",
                 "afold", "fp8", "default_procs", "shared", "fbc", "branches", "keep", "h0", "h1c", "attention_kwargs", "live",
                 "live_segs", "rows", "segs", "win", "sp", "lite", "mag", "tea", "ras", "out_buf", "elements")

    def __init__(self, **fields):
        self.elements = None
        self.ras = None
        self.tea = None
        for k, v in fields.items():
            setattr(self, k, v)

    def element(self, i):
        """the same call seen as batch element i alone: views of its n rows, its text, b = 1 (Pyramid Attention Broadcast runs
        a hooked attention branch element by element); built once per call and element"""
        if self.elements is None:
            self.elements = {}
        if i in self.elements:
            return self.elements[i]
        r0, r1 = i * self.n, (i + 1) * self.n
        f = {k: getattr(self, k) for k in self.__slots__ if k != "elements"}
        for k in ("x", "nrm", "att", "q2", "ff", "qkv"):
            f[k] = f[k][r0:r1]
        f.update(b=1, nr=self.n, cos=self.cos1, sin=self.sin1, sel=_sel_rows(self.sel, r0, r1), segs=[(0, self.n)],
                 text=_text_element(self.text, i, self.b, self.n, self.d), keep=None)
        self.elements[i] = _Call(**f)
        return self.elements[i]


def _live_range(live_rows, n):
    """`forward(live_rows=(lo, hi))` as a checked row range of a sequence of n rows, or None (no range, or not a proper one)"""
    if live_rows is None:
        return None
    lo, hi = int(live_rows[0]), int(live_rows[1])
    return (lo, hi) if 0 <= lo < hi <= n else None


def _sel_rows(sel, r0, r1):
    """rows [r0, r1) of the per-token modulation selector (None: every row takes table row 0)"""
    return None if sel is None else sel[r0:r1]


def _keep_kw(c, r0, r1):
    """`keep=` of the closing GEMM over rows [r0, r1) while Pyramid Attention Broadcast computes a branch, else nothing"""
    return {} if c.keep is None else {"keep": c.keep[(r0, r1)]}


def _keep_copy(c, y):
    """a custom processor's return value y [rows, D] into the buffers Pyramid Attention Broadcast keeps it in"""
    if c.keep is not None:
        for (r0, r1), buf in c.keep.items():
            buf.copy_(y[r0:r1])


def _text_element(text, i, b, n, d):
    """the text K / V (`_text_kv`) of batch element i alone"""
    lt = text.lt
    t = SimpleNamespace(txt=text.txt.view(b, lt, d)[i], kv=[kv.view(b, lt, 2 * d)[i] for kv in text.kv], lt=lt, w2=None,
                        tail=None if text.tail is None else (text.tail[0][i:i + 1], text.tail[1][i:i + 1]))
    if text.w2 is not None:
        t.w2, t.kp, t.pbuf, t.rrms = [[w[i]] for w in text.w2], text.kp[i:i + 1], text.pbuf[i:i + 1], text.rrms[i * n:(i + 1) * n]
    return t


class _CompactRope(tuple):
    """(cos, sin) already in the compact [L, Dh/2] layout; recognised by MI355WanAttnProcessor."""
    compact = True
