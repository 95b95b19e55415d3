"""MI355X-native CogVideoXTransformer3DModel (CogVideoX-5B-I2V as FrameINO fine-tunes it: 48 input channels,
`use_FrameIn=True`, learned positional embedding + 3D RoPE).

Mirror of /root/reference/architecture/cogvideox_transformer_3d.py: same constructor arguments, parameter names,
`forward(hidden_states, encoder_hidden_states, timestep, timestep_cond=None, ofs=None, image_rotary_emb=None,
attention_kwargs=None, return_dict=True)`, `attn_processors` / `set_attn_processor` / `fuse_qkv_projections` /
`unfuse_qkv_projections` (:346-444).  Arithmetic runs in libframeino_hip.so.

Layout: text and video tokens of a batch element live in ONE row-major buffer `[B, Lt+Lv, D]` (text first) -- the
reference concatenates them for attention and for the feed-forward in every block anyway (:155, attention_processor
:2826).  Per-row modulation uses a `[2B, D]` table (row 2b = video params, 2b+1 = text params) + an int32 selector, so
LayerNormZero / gates are single kernels over all rows; the gate multiply + residual is the GEMM epilogue.
"""
import math
import os
from types import SimpleNamespace

import torch
import torch.nn.functional as F
from torch import nn

from . import ops
from .attention_processor import Attention, MI355CogVideoXAttnProcessor, MI355FusedCogVideoXAttnProcessor
from .loading import FromPretrainedMixin
from .lora import LoraModelMixin
from .mx_linears import MXLinearsMixin
from .step_cache import PyramidAttentionBroadcastMixin
from .transformer_wan import FeedForward, _Config, _MLP2
from .window_attention import SelfAttentionOptionsMixin


class _LayerNormZero(nn.Module):
    def __init__(self, cond_dim, dim, affine, eps):
        super().__init__()
        self.linear = nn.Linear(cond_dim, 6 * dim)
        self.norm = nn.LayerNorm(dim, eps=eps, elementwise_affine=affine)


class _AdaLayerNorm(nn.Module):
    def __init__(self, cond_dim, out_dim, affine, eps):
        super().__init__()
        self.linear = nn.Linear(cond_dim, out_dim)
        self.norm = nn.LayerNorm(out_dim // 2, eps, affine)


class CogVideoXPatchEmbed(nn.Module):
    def __init__(self, patch_size, in_channels, embed_dim, text_embed_dim, bias, pos_shape, persistent):
        super().__init__()
        self.proj = nn.Conv2d(in_channels, embed_dim, kernel_size=(patch_size, patch_size), stride=patch_size, bias=bias)
        self.text_proj = nn.Linear(text_embed_dim, embed_dim)
        self.register_buffer("pos_embedding", torch.zeros(pos_shape), persistent=persistent)


class CogVideoXBlock(nn.Module):
    def __init__(self, dim, heads, head_dim, time_embed_dim, attention_bias, affine, eps):
        super().__init__()
        self.norm1 = _LayerNormZero(time_embed_dim, dim, affine, eps)
        self.attn1 = Attention(dim, heads=heads, dim_head=head_dim, qk_norm="layer_norm", eps=1e-6,
                               bias=attention_bias, out_bias=True, processor=MI355CogVideoXAttnProcessor())
        self.norm2 = _LayerNormZero(time_embed_dim, dim, affine, eps)
        self.ff = FeedForward(dim, 4 * dim)


def _sincos_1d(dim, pos):
    omega = 1.0 / 10000 ** (torch.arange(dim // 2, dtype=torch.float64) / (dim / 2.0))
    out = torch.outer(pos.reshape(-1).double(), omega)
    return torch.cat([torch.sin(out), torch.cos(out)], dim=1).float()


def cog_sincos_pos_embed(embed_dim, pw, ph, frames, spatial_scale, temporal_scale):
    """architecture/embeddings.py:81-150 (get_3d_sincos_pos_embed, pt path) -> [frames*ph*pw, embed_dim]."""
    ds, dtm = 3 * embed_dim // 4, embed_dim // 4
    gh = torch.arange(ph, dtype=torch.float32) / spatial_scale
    gw = torch.arange(pw, dtype=torch.float32) / spatial_scale
    grid = torch.stack(torch.meshgrid(gw, gh, indexing="xy"), dim=0).reshape(2, 1, ph, pw)
    emb_h = _sincos_1d(ds // 2, grid[0])
    emb_w = _sincos_1d(ds // 2, grid[1])
    spatial = torch.cat([emb_h, emb_w], dim=1)                                       # [ph*pw, ds]
    temporal = _sincos_1d(dtm, torch.arange(frames, dtype=torch.float32) / temporal_scale)
    spatial = spatial[None].repeat_interleave(frames, dim=0)
    temporal = temporal[:, None].repeat_interleave(ph * pw, dim=1)
    return torch.cat([temporal, spatial], dim=-1).flatten(0, 1)


class CogVideoXTransformer3DModel(nn.Module, FromPretrainedMixin, LoraModelMixin, PyramidAttentionBroadcastMixin, MXLinearsMixin,
                                  SelfAttentionOptionsMixin):
    """MX linears (enable_mxfp8_linears / enable_mxfp6_linears): four large linears of every block -- QKV, attention out, FFN
    up / down; with `enable_fp8_attention()` MXFP8 is BASELINE config 5's "fp8 MFMA path" end to end.

    fp8 attention (enable_fp8_attention): the joint text + video self-attention (attention_processor.py:2863 of the reference,
    head_dim 64: 55 % of the CogVideoX-5B step) -- K / V quantised per call with one scale per 32 elements (`fino_attn_fwd_fp8`).
    No reference counterpart: tolerance stated in tests/test_attention_fp8_gpu.py and
    tests/test_fullsize_oracle_gpu.py against fp32 and against this model's own bf16 forward.

    Window attention (enable_window_attention): a video query attends the text rows, its window and the
    sink frames; text queries and text keys stay dense (`prefix_rows` of frameino_amd/window_attention.py = the text rows).  With
    `enable_fp8_attention()` it takes `ops.attention_fp8_ranges` with the model's p_mode / smooth_k / smooth_v.  MX linears and
    LoRA work with it; a user-installed attention processor, and fp8 attention at a head_dim other than 64, are refused.

    Step caching (diffusers' CacheMixin surface: enable_cache / disable_cache / is_cache_enabled / cache_context /
    _reset_stateful_cache, and `cache_log`; frameino_amd/step_cache.py): Pyramid Attention Broadcast,
    `enable_cache(PyramidAttentionBroadcastConfig(spatial_attention_block_skip_range=2, current_timestep_callback=...))`.  Opt-in
    and approximate.  Every block's joint attn1 is the "spatial" kind; per `cache_context` and layer one [B L, D] buffer in the
    model dtype holds y = T(acc + bias) of `attn1.to_out[0]` over the joint [text | video] rows (the CFG batch of 2 is one
    segment with one decision), written by the out-projection's own epilogue (`keep=`) on a computing forward.  A re-using forward
    launches nothing of the branch -- no norm1, QKV, head norm + RoPE, attention, out-projection -- and adds the cached y with the
    staged epilogue's arithmetic (`ops.gated_residual(staged=True)`).  With the cache enabled the LAST block runs all L rows
    (`skip_dead_rows` is off: the cache must hold every row for the forwards that re-use it); the returned rows and the
    `live_frames` zeros are what they are without it.  A user-installed processor is cached by its return value.  MX linears,
    fp8 attention, LoRA and window attention combine with it: the cache stores whatever the branch produced.  At BASELINE
    config 5 the buffers are 42 x 235 MB = 9.9 GB.  `FirstBlockCacheConfig` is refused."""
    _loader_name = "load_cogvideox_transformer"
    _window_table_cache = "_pos_cache"
    _fp8_window_walk = True       # fino_attn_fwd_fp8_ranges (head_dim 64; any other is refused by `_window_refusals`)

    def __init__(self, num_attention_heads=30, attention_head_dim=64, in_channels=16, out_channels=16,
                 flip_sin_to_cos=True, freq_shift=0, time_embed_dim=512, ofs_embed_dim=None, text_embed_dim=4096,
                 num_layers=30, dropout=0.0, attention_bias=True, sample_width=90, sample_height=60, sample_frames=49,
                 patch_size=2, patch_size_t=None, temporal_compression_ratio=4, max_text_seq_length=226,
                 activation_fn="gelu-approximate", timestep_activation_fn="silu", norm_elementwise_affine=True,
                 norm_eps=1e-5, spatial_interpolation_scale=1.875, temporal_interpolation_scale=1.0,
                 use_rotary_positional_embeddings=False, use_learned_positional_embeddings=False, patch_bias=True,
                 extra_encoder_cond_channels=-1, use_FrameIn=False):
        super().__init__()
        if patch_size_t is not None or ofs_embed_dim:
            raise NotImplementedError("CogVideoX-1.5 (patch_size_t / ofs) is not on FrameINO's path")
        if not use_rotary_positional_embeddings:
            raise NotImplementedError("FrameINO fine-tunes CogVideoX-5B (RoPE); the 2B variant is not on its path")
        inner = num_attention_heads * attention_head_dim
        self.inner_dim = inner
        self.config = _Config(num_attention_heads=num_attention_heads, attention_head_dim=attention_head_dim,
                              in_channels=in_channels, out_channels=out_channels, flip_sin_to_cos=flip_sin_to_cos,
                              freq_shift=freq_shift, time_embed_dim=time_embed_dim, ofs_embed_dim=ofs_embed_dim,
                              text_embed_dim=text_embed_dim, num_layers=num_layers, sample_width=sample_width,
                              sample_height=sample_height, sample_frames=sample_frames, patch_size=patch_size,
                              patch_size_t=patch_size_t, temporal_compression_ratio=temporal_compression_ratio,
                              max_text_seq_length=max_text_seq_length, norm_elementwise_affine=norm_elementwise_affine,
                              norm_eps=norm_eps, spatial_interpolation_scale=spatial_interpolation_scale,
                              temporal_interpolation_scale=temporal_interpolation_scale,
                              use_rotary_positional_embeddings=use_rotary_positional_embeddings,
                              use_learned_positional_embeddings=use_learned_positional_embeddings,
                              use_FrameIn=use_FrameIn)
        pph, ppw = sample_height // patch_size, sample_width // patch_size
        ptf = (sample_frames - 1) // temporal_compression_ratio + 1
        self.patch_embed = CogVideoXPatchEmbed(patch_size, in_channels, inner, text_embed_dim, patch_bias,
                                               (1, max_text_seq_length + pph * ppw * ptf, inner),
                                               use_learned_positional_embeddings)
        if not use_learned_positional_embeddings:
            pe = cog_sincos_pos_embed(inner, ppw, pph, ptf, spatial_interpolation_scale, temporal_interpolation_scale)
            self.patch_embed.pos_embedding[:, max_text_seq_length:].copy_(pe)
        self.time_embedding = _MLP2(inner, time_embed_dim)
        self.transformer_blocks = nn.ModuleList([
            CogVideoXBlock(inner, num_attention_heads, attention_head_dim, time_embed_dim, attention_bias,
                           norm_elementwise_affine, norm_eps) for _ in range(num_layers)])
        self.norm_final = nn.LayerNorm(inner, norm_eps, norm_elementwise_affine)
        self.norm_out = _AdaLayerNorm(time_embed_dim, 2 * inner, norm_elementwise_affine, norm_eps)
        self.proj_out = nn.Linear(inner, patch_size * patch_size * out_channels)
        self._packed = None
        self._pos_cache = {}
        self.ops = ops            # kernel front end (tests inject a CPU stand-in)
        self._init_self_attention_options()
        # q leaves its LayerNorm + RoPE kernel multiplied by head_dim**-0.5 * log2(e) and the attention kernels take q.k as
        # the exp2 argument (FINO_ATTN_SCALE_FOLDED): at head_dim 64 that selects the 4-wave kernel with the running maximum
        # folded into its MFMAs (-5 % per step).  Video rows: one rounding of q.c instead of q; the 226 text rows (LayerNorm
        # only, already rounded) are rounded twice.  False: q as the reference rounds it, scale applied to the logits.
        self.fold_softmax_scale = True
        # in the last block, rows nobody reads afterwards (text rows; frames beyond forward(live_frames=)) are keys / values only
        self.skip_dead_rows = os.environ.get("FINO_SKIP_DEAD_ROWS", "1") != "0"
        self.original_attn_processors = None

    # ---- reference surface (:346-444) ----
    @property
    def dtype(self):
        return self.proj_out.weight.dtype

    @property
    def device(self):
        return self.proj_out.weight.device

    @property
    def attn_processors(self):
        return {f"transformer_blocks.{i}.attn1.processor": b.attn1.processor
                for i, b in enumerate(self.transformer_blocks)}

    def set_attn_processor(self, processor):
        count = len(self.transformer_blocks)
        if isinstance(processor, dict) and len(processor) != count:
            raise ValueError(f"A dict of processors was passed, but the number of processors {len(processor)} does not "
                             f"match the number of attention layers: {count}. Please make sure to pass {count} "
                             f"processor classes.")
        for i, b in enumerate(self.transformer_blocks):
            b.attn1.set_processor(processor[f"transformer_blocks.{i}.attn1.processor"] if isinstance(processor, dict)
                                  else processor)
        self._packed = None

    def fuse_qkv_projections(self):
        self.original_attn_processors = self.attn_processors
        for b in self.transformer_blocks:
            b.attn1.fuse_projections(fuse=True)
        self.set_attn_processor(MI355FusedCogVideoXAttnProcessor())

    def unfuse_qkv_projections(self):
        if self.original_attn_processors is not None:
            self.set_attn_processor(self.original_attn_processors)

    def load_reference_state_dict(self, sd, dtype=None):
        own = self.state_dict()
        missing = [k for k in own if k not in sd]
        if missing:
            raise KeyError(f"state-dict is missing {missing[:5]}")
        with torch.no_grad():
            for k, t in list(self.named_parameters()) + list(self.named_buffers()):
                t.data = sd[k].to(dtype or sd[k].dtype).to(t.device).contiguous()
        self.reset_caches()
        return self

    def reset_caches(self):
        """Drop everything derived from the parameters (packed / fused copies, MX weights, positional tables, the step cache's
        buffers); called whenever the parameters may have changed or moved.  Returns whether MX linears were on (the next forward
        re-quantises)."""
        had_fp8 = self._mx_invalidate()
        self._reset_stateful_cache()
        self._packed = None
        self._pos_cache.clear()           # (the window-attention range tables live here too: `_window_table_cache`)
        return had_fp8

    def _apply(self, fn, *args, **kwargs):          # .to() / .cuda() / .half()
        out = super()._apply(fn, *args, **kwargs)
        if hasattr(self, "_pos_cache"):
            self.reset_caches()
        return out

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self.reset_caches()
        return out

    # ---- packing ----
    def _mx_linear_weights(self, pk):
        for li, (blk, e) in enumerate(zip(self.transformer_blocks, pk.layers)):
            for key, w in (("qkv", e.wqkv), ("out", blk.attn1.to_out[0].weight), ("ff1", blk.ff.net[0].proj.weight),
                           ("ff2", blk.ff.net[2].weight)):
                yield li, key, w

    def enable_sparse_attention(self, config):
        raise NotImplementedError("sparse attention (enable_sparse_attention) is not wired on this model: the joint text + video "
                                  "sequence needs its own forced tiles (the Wan DiT has it)")

    def _window_refusals(self, fp8, default_procs, shard=None):
        what = "window attention (enable_window_attention)"
        if not default_procs:
            raise NotImplementedError(f"{what} with a user-installed attention processor: the windows are applied by the "
                                      f"built-in MI355CogVideoXAttnProcessor path only")
        if fp8 and self.config.attention_head_dim != 64:
            raise NotImplementedError(f"{what} with fp8 attention at head_dim {self.config.attention_head_dim}: the fp8 range "
                                      f"walk (fino_attn_fwd_fp8_ranges) exists for head_dim 64 only")

    def _qkv_heads(self, ops, li, blk, e, x2, t1, sel, b, L, lt, cos, sin, qfold):
        """the head of block li's attention branch over all rows: norm1 (CogVideoXLayerNormZero, or emitted directly as the
        linear's MXFP8 activations), the fused QKV projection, per-head LayerNorm + RoPE on q and k -> q | k | v [B, L, 3D]"""
        c = self.config
        d, heads, dh = self.inner_dim, c.num_attention_heads, c.attention_head_dim
        xq1 = self._ln_q(li, "qkv", 2, x2, weight=e.n1w, bias=e.n1b, shift=t1[:, 0], scale=t1[:, 1], sel=sel, eps=c.norm_eps)
        n = None if xq1 is not None else ops.layernorm_zero(x2, e.n1w, e.n1b, t1[:, 0], t1[:, 1], sel, c.norm_eps)
        qkv = self._lin(li, "qkv", n, e.wqkv, e.bqkv, xq=xq1).view(b, L, 3 * d)
        nq, nk = blk.attn1.norm_q, blk.attn1.norm_k
        ops.headnorm_rope_(qkv[:, :, :d], heads, dh, nq.weight, nq.bias, nq.eps, cos, sin, rope_row0=lt, **qfold)
        ops.headnorm_rope_(qkv[:, :, d:2 * d], heads, dh, nk.weight, nk.bias, nk.eps, cos, sin, rope_row0=lt)
        return qkv

    def _attention_branch(self, ops, win, fp8, li, blk, e, x2, t1, sel, b, L, lt, cos, sin, qfold, afold, default_procs,
                          image_rotary_emb, attention_kwargs, kept):
        """the first half of block li over all rows: x2 += gate * attn1(norm1(x2)) in place.  `kept` (Pyramid Attention
        Broadcast, a computing forward): the [B L, D] buffer that also receives the branch output y = T(acc + bias) -- from the
        out-projection's epilogue, or a user-installed processor's return value"""
        c = self.config
        d, heads = self.inner_dim, c.num_attention_heads
        if default_procs:
            qkv = self._qkv_heads(ops, li, blk, e, x2, t1, sel, b, L, lt, cos, sin, qfold)
            att = self._attend(ops, qkv[:, :, :d], qkv[:, :, d:2 * d], qkv[:, :, 2 * d:], heads, fp8=fp8,
                               ranges=self._window_ranges(win, li, (0, L)), **afold)
            keep = {} if kept is None else {"keep": kept}
            self._lin(li, "out", att.view(b * L, d), blk.attn1.to_out[0].weight, blk.attn1.to_out[0].bias,
                      ops.EPI_GATED_RESIDUAL_STAGED, residual=x2, gate=t1[:, 2], sel=sel, out=x2, **keep)
        else:
            n3 = ops.layernorm_zero(x2, e.n1w, e.n1b, t1[:, 0], t1[:, 1], sel, c.norm_eps).view(b, L, d)
            ah, ae = blk.attn1(hidden_states=n3[:, lt:], encoder_hidden_states=n3[:, :lt],
                               image_rotary_emb=image_rotary_emb, **(attention_kwargs or {}))
            y = torch.cat([ae, ah], dim=1).reshape(b * L, d)
            if kept is not None:
                y = kept.copy_(y)
            ops.gated_residual(x2, y, t1[:, 2], sel, out=x2, staged=True)

    def _default_processors(self):
        return all(type(b.attn1.processor) in (MI355CogVideoXAttnProcessor, MI355FusedCogVideoXAttnProcessor)
                   for b in self.transformer_blocks)

    def _pack(self):
        pk = SimpleNamespace(layers=[])
        f32 = lambda t: None if t is None else t.detach().float().contiguous()     # noqa: E731
        for b in self.transformer_blocks:
            a = b.attn1
            e = SimpleNamespace()
            e.wqkv = torch.cat([a.to_q.weight, a.to_k.weight, a.to_v.weight]).detach().contiguous()
            e.bqkv = torch.cat([a.to_q.bias, a.to_k.bias, a.to_v.bias]).detach().contiguous() \
                if a.to_q.bias is not None else None
            e.n1w, e.n1b = f32(b.norm1.norm.weight), f32(b.norm1.norm.bias)
            e.n2w, e.n2b = f32(b.norm2.norm.weight), f32(b.norm2.norm.bias)
            pk.layers.append(e)
        # all 2*layers LayerNormZero projections + norm_out as ONE skinny GEMM weight
        ws = [m.linear.weight for b in self.transformer_blocks for m in (b.norm1, b.norm2)] + [self.norm_out.linear.weight]
        bs = [m.linear.bias for b in self.transformer_blocks for m in (b.norm1, b.norm2)] + [self.norm_out.linear.bias]
        pk.wmod = torch.cat(ws).detach().contiguous()
        pk.bmod = torch.cat(bs).detach().contiguous()
        pk.w_patch = self.patch_embed.proj.weight.detach().reshape(self.inner_dim, -1).contiguous()
        pk.nfw, pk.nfb = f32(self.norm_final.weight), f32(self.norm_final.bias)
        pk.now, pk.nob = f32(self.norm_out.norm.weight), f32(self.norm_out.norm.bias)
        self._packed = pk
        return pk

    def _pos_embeds(self, num_frames, height, width, text_len, dtype):
        """architecture/embeddings.py:764-802 (FrameIn first-frame PE reuse, trilinear resize off the default size).
        Step-invariant: built once per geometry (the reference rebuilds and re-interpolates it every forward)."""
        key = (num_frames, height, width, text_len, dtype)
        if key in self._pos_cache:
            return self._pos_cache[key]
        c = self.config
        pos = self.patch_embed.pos_embedding
        ps, tcr, maxt = c.patch_size, c.temporal_compression_ratio, c.max_text_seq_length
        post = (c.sample_frames - 1) // tcr + 1
        pph, ppw = c.sample_height // ps, c.sample_width // ps
        seq = height * width * num_frames // (ps * ps)
        if c.use_FrameIn:
            first = (pos.shape[1] - maxt) // (num_frames - 1)
            pos = torch.cat([pos, pos[:, text_len:text_len + first].clone()], dim=1)
        if c.sample_height != height or c.sample_width != width or c.sample_frames != (num_frames - 1) * tcr + 1:
            if c.use_FrameIn:
                post += 1
            d = pos.shape[-1]
            pw_ = pos[:, text_len:].view(1, post, pph, ppw, d).permute(0, 4, 1, 2, 3)
            pw_ = F.interpolate(pw_, size=[post, height // ps, width // ps], mode="trilinear", align_corners=False)
            pw_ = pw_.permute(0, 2, 3, 4, 1).reshape(1, -1, d)
            pos = torch.cat([pos[:, :text_len], pw_], dim=1)[:, :text_len + seq]
        out = pos[0].to(dtype).contiguous()
        self._pos_cache[key] = out
        return out

    # ---- forward (:446-562) ----
    @torch.no_grad()
    def forward(self, hidden_states, encoder_hidden_states, timestep, timestep_cond=None, ofs=None,
                image_rotary_emb=None, attention_kwargs=None, return_dict=True, live_frames=None, id_frames=0):
        """`live_frames=k` (round 6): the caller reads the prediction of the first k latent frames only -- the FrameINO loop drops
        the identity frame appended on the frame axis (pipeline_cogvideox_i2v_motion_FrameINO.py:866-881, :896).  In the LAST block
        the other frames' tokens then serve as keys / values only, and so do the TEXT rows on every call (the model returns video
        rows only, :531-542): their attention queries, out-projection and feed-forward are skipped; dropped frames come back ZERO.
        Every returned row is computed exactly as without it.  With a step cache enabled (`enable_cache`) the last block runs
        all rows -- the cache holds every row's branch output -- and the same rows and zeros are returned.
        `id_frames` (window attention only, `enable_window_attention`): the trailing latent frames that are identity-reference
        frames; every query sees them, like `config.sink_frames`."""
        ops = self.ops
        if timestep_cond is not None:
            raise NotImplementedError("timestep_cond is never passed on the FrameINO path")
        if attention_kwargs is not None:
            attention_kwargs = dict(attention_kwargs)
        # LoRA scale (:460-465): adapters are merged into the weights, a changed scale re-merges them here (frameino_amd/lora.py)
        self._lora_apply(attention_kwargs.pop("scale", None) if attention_kwargs is not None else None)
        self._mx_requantise_if_pending()
        pk = self._packed or self._pack()
        default_procs = self._default_processors()
        if self._window is not None:             # what window attention refuses, before anything is launched
            self._window_refusals(self.fp8_attention, default_procs)
        c = self.config
        b, nf, ch, hh, ww = hidden_states.shape
        d, heads, dh, ps = self.inner_dim, c.num_attention_heads, c.attention_head_dim, c.patch_size
        dev, dt = hidden_states.device, hidden_states.dtype
        lt = encoder_hidden_states.shape[1]
        lv = nf * (hh // ps) * (ww // ps)
        L = lt + lv
        # sliding-window self-attention over frames: this forward's decision (the timestep callback is read here, once)
        win = self._window_begin(nf, (hh // ps) * (ww // ps), lt, id_frames, dev)
        fp8 = self.fp8_attention and dh == 64     # this call's self-attention takes fp8 operands
        # Pyramid Attention Broadcast: this forward's decision for every block's attn1 (callback read once, nothing launched yet);
        # the call's rows are ONE segment under the current cache_context
        pab = self._pab_begin(b, L, d, dt, dev)
        seg = pab.segs[0] if pab is not None and pab.hooked["self"] else None

        # 1. time embedding (:477-483): sinusoid fp32 -> T -> MLP in T
        half = d // 2
        expo = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32, device=dev) / (half - c.freq_shift))
        ang = timestep.reshape(-1).float()[:, None] * expo[None]
        t_emb = torch.cat([torch.sin(ang), torch.cos(ang)], dim=-1)
        if c.flip_sin_to_cos:
            t_emb = torch.cat([t_emb[:, half:], t_emb[:, :half]], dim=-1)
        te = self.time_embedding
        h1 = ops.skinny_linear(t_emb.to(dt).float().contiguous(), te.linear_1.weight, te.linear_1.bias).to(dt)
        emb = ops.skinny_linear(F.silu(h1).float().contiguous(), te.linear_2.weight, te.linear_2.bias).to(dt)   # [B, E]
        # every LayerNormZero / AdaLayerNorm projection of silu(emb) in one launch -> [B, (2*layers*6 + 2) * D] in T
        mods = ops.skinny_linear(F.silu(emb).float().contiguous(), pk.wmod, pk.bmod).to(dt).float()
        nl = c.num_layers
        lnz = mods[:, :2 * nl * 6 * d].view(b, 2 * nl, 2, 3, d)                      # [B, norm, video|text, (shift,scale,gate), D]
        tables = lnz.permute(1, 0, 2, 3, 4).reshape(2 * nl, 2 * b, 3, d).contiguous()   # row 2b = video, 2b+1 = text
        out_mod = mods[:, 2 * nl * 6 * d:].view(b, 2, d).contiguous()                # (shift, scale) of norm_out
        sel = torch.zeros(b, L, dtype=torch.int32, device=dev)
        sel[:, :lt] = 1
        sel += 2 * torch.arange(b, device=dev, dtype=torch.int32)[:, None]
        sel = sel.reshape(-1).contiguous()

        # 2. patch embedding (:494) into the joint buffer [B, Lt+Lv, D]
        x = torch.empty(b, L, d, dtype=dt, device=dev)
        pe = self.patch_embed
        pos = self._pos_embeds(nf, hh, ww, lt, dt)
        for i in range(b):
            ops.gemm(encoder_hidden_states[i], pe.text_proj.weight, pe.text_proj.bias, out=x[i, :lt])
            a = ops.patchify(hidden_states[i].permute(1, 0, 2, 3).contiguous(), (1, ps, ps))
            ops.gemm(a, pk.w_patch, pe.proj.bias, out=x[i, lt:])
            ops.gated_residual(x[i], pos, out=x[i])
        x2 = x.view(b * L, d)
        cos = sin = None
        if image_rotary_emb is not None:
            cos, sin = (t.to(dev).float().contiguous() for t in image_rotary_emb)

        fold = self.fold_softmax_scale and hasattr(ops, "SCALE_FOLDED")
        qfold = {"out_scale": dh ** -0.5 * ops.LOG2E} if fold else {}
        afold = {"scale": ops.SCALE_FOLDED} if fold else {}
        # rows of the joint sequence whose output anyone reads after the last block: the video rows of the live frames
        tpf = (hh // ps) * (ww // ps)
        kf = nf if live_frames is None else max(1, min(int(live_frames), nf))
        r0, r1 = lt, lt + kf * tpf
        skip_dead = (self.skip_dead_rows and default_procs and not self._fp8 and not self.fp8_attention and len(self.transformer_blocks) > 1
                     and (r1 - r0) < L)
        if not skip_dead:
            kf, r0, r1 = nf, lt, L
        # Pyramid Attention Broadcast: the cache holds every row of every block's branch, so the last block runs all L rows; what
        # is returned (the live frames' rows, zeros for the others) stays
        skip_dead_block = skip_dead and pab is None
        # 3. blocks (:503-529)
        for li, (blk, e) in enumerate(zip(self.transformer_blocks, pk.layers)):
            t1, t2 = tables[2 * li], tables[2 * li + 1]                              # [2B, 3, D]
            if skip_dead_block and li == len(self.transformer_blocks) - 1:
                # LAST block: every row is a key / value, only rows [r0, r1) of each sample are queries and go on
                # (MX linears are off here -- `skip_dead` -- so the shared head takes its model-dtype norm1 and GEMM)
                qkv = self._qkv_heads(ops, li, blk, e, x2, t1, sel, b, L, lt, cos, sin, qfold)
                att = self._attend(ops, qkv[:, r0:r1, :d], qkv[:, :, d:2 * d], qkv[:, :, 2 * d:], heads, fp8=fp8,
                                   ranges=self._window_ranges(win, li, (r0, r1)), **afold)      # [B, r1 - r0, D]
                for i in range(b):
                    xs, ss = x2[i * L + r0:i * L + r1], sel[i * L + r0:i * L + r1]
                    self._lin(li, "out", att[i], blk.attn1.to_out[0].weight, blk.attn1.to_out[0].bias,
                              ops.EPI_GATED_RESIDUAL_STAGED, residual=xs, gate=t1[:, 2], sel=ss, out=xs)
                    n = ops.layernorm_zero(xs, e.n2w, e.n2b, t2[:, 0], t2[:, 1], ss, c.norm_eps)
                    ff = self._lin(li, "ff1", n, blk.ff.net[0].proj.weight, blk.ff.net[0].proj.bias, ops.EPI_GELU_TANH)
                    self._lin(li, "ff2", ff, blk.ff.net[2].weight, blk.ff.net[2].bias, ops.EPI_GATED_RESIDUAL_STAGED,
                              residual=xs, gate=t2[:, 2], sel=ss, out=xs)
                continue
            if seg is not None and not seg.compute["self"]:
                # Pyramid Attention Broadcast, a re-using forward: nothing of the attention branch runs; the y the last computing
                # forward kept goes through the arithmetic of the out-projection's staged epilogue
                pab.reuse(ops, seg, "self", li, 0, b * L, x2, t1[:, 2], sel, fused=False, staged=True)
            else:
                # (... a computing forward: the out-projection also writes y = T(acc + bias) into this layer's buffer)
                kept = None if seg is None else pab.kept(None, seg, "self", li, 0, b * L)
                self._attention_branch(ops, win, fp8, li, blk, e, x2, t1, sel, b, L, lt, cos, sin, qfold, afold, default_procs,
                                       image_rotary_emb, attention_kwargs, kept)
            xq2 = (self._ln_q(li, "ff1", 2, x2, weight=e.n2w, bias=e.n2b, shift=t2[:, 0], scale=t2[:, 1], sel=sel, eps=c.norm_eps)
                   if (li, "ff2") in self._fp8 else None)
            n = None if xq2 is not None else ops.layernorm_zero(x2, e.n2w, e.n2b, t2[:, 0], t2[:, 1], sel, c.norm_eps)
            if self._ffn_mxfp8(li, n, xq2, blk.ff.net[0].proj.bias, blk.ff.net[2].bias, ops.EPI_GATED_RESIDUAL_STAGED,
                               residual=x2, gate=t2[:, 2], sel=sel, out=x2) is None:
                ff = self._lin(li, "ff1", n, blk.ff.net[0].proj.weight, blk.ff.net[0].proj.bias, ops.EPI_GELU_TANH)
                self._lin(li, "ff2", ff, blk.ff.net[2].weight, blk.ff.net[2].bias, ops.EPI_GATED_RESIDUAL_STAGED,
                          residual=x2, gate=t2[:, 2], sel=sel, out=x2)

        # 4. final norms + projection (:531-542) on the video rows
        outs = []
        for i in range(b):
            v = ops.layernorm(x[i, lt:r1], pk.nfw, pk.nfb, c.norm_eps)
            v = ops.layernorm_zero(v, pk.now, pk.nob, out_mod[i, 0], out_mod[i, 1], None, c.norm_eps)
            y = ops.gemm(v, self.proj_out.weight, self.proj_out.bias)                # [Lv, p*p*Cout] (c, dh, dw) columns
            y = y.view(kf, hh // ps, ww // ps, c.out_channels, ps, ps).permute(0, 3, 1, 4, 2, 5)
            outs.append(y.reshape(kf, c.out_channels, hh, ww))
        out = torch.stack(outs)
        if kf < nf:                                                                  # frames nobody reads: zeros
            out = torch.cat([out, out.new_zeros((b, nf - kf) + tuple(out.shape[2:]))], dim=1)
        if not return_dict:
            return (out,)
        return SimpleNamespace(sample=out)
