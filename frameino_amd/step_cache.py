"""Step caching of the Wan DiT: diffusers' `CacheMixin` (diffusers/models/cache_utils.py), which the reference's
WanTransformer3DModel inherits (architecture/transformer_wan.py:28, :353) and whose state its FrameINO loop keys by
`cache_context("cond")` / `("uncond")` (pipelines/pipeline_wan_i2v_motion_FrameINO.py:862, :873), with six of its configs:
`FirstBlockCacheConfig` (diffusers/hooks/first_block_cache.py), `PyramidAttentionBroadcastConfig`
(diffusers/hooks/pyramid_attention_broadcast.py), `TaylorSeerCacheConfig` (diffusers/hooks/taylorseer_cache.py),
`FasterCacheConfig` (diffusers/hooks/faster_cache.py), `MagCacheConfig` (diffusers/hooks/mag_cache.py) and `TeaCacheConfig`.
One at a time: a second `enable_cache` raises, as in diffusers.

Layout.  Every config has ONE policy class below (`_FirstBlockPolicy`, `_PabPolicy`, `_TaylorSeerPolicy`, `_FasterCachePolicy`,
`_MagCachePolicy`, `_TeaCachePolicy`) that
states what is particular to it -- the attributes a duck-typed config must carry, its validation, its enable-time warnings and
defaults, its label in messages, why a captured step cannot contain it, whether a batch may run under it, whether it takes over
the attention branches -- and the entry points a forward asks (`segments` around the stack's first block, `lite` around the whole
stack, `branches` for the attention branches, `magcache` around the block stack between the embedding and the output head).  `StepCacheMixin.enable_cache` is a lookup over the model's `_cache_policies`
and stores the chosen policy next to the config; the `_pab_on` / `_taylor_on` / ... flags are read-only views of it.  The
attention branches of a forward run under ONE plan, whichever cache made it: `_BroadcastPlan` (Pyramid Attention Broadcast) or
`_TaylorPlan` (TaylorSeer's default mode, FasterCache's self-attention part), which say where a computing branch's output is kept,
what follows it, and which single launch stands for a branch that does not run.  What a cache does not combine with is one
method of the model, `_cache_refusals`, called from `enable_cache`, from where the other feature is enabled and from the forward.

First-block caching.  The rule, per forward under context c (T = the model dtype; h0 = input of block 0, h1 = its output, hN = the last block's):

    r = T(h1 - h0)
    compute  if  head_residual is None  or  diff > threshold,   diff = float(T(T(mean|T(r - p)|) / T(mean|p|))),  p = head_residual
    compute: head_residual = r, blocks 1 .. N-1 run, tail_residual = T(hN - h1)
    skip:    head_residual unchanged, blocks 1 .. N-1 do not run, the stack's output is T(tail_residual + h1)

The output head runs in both cases.  The means cover every element of the call's [B, L, D] rows under that context (a direct
batch-B call makes one joint decision).  On the GPU one probe kernel (ops.step_cache_probe) writes r and the two fp32 sums;
the host reads them -- the one host sync of the rule, where diffusers calls `.item()` -- and rounds as torch does (`decide`).

Pyramid Attention Broadcast.  Every attention module (on this model: "spatial" = every block's attn1, "cross" = every block's
attn2; there is no temporal attention layer) has, per context, an `iteration` (from 0) and a `cache` (empty at first).  A forward
of that module under context c:

    t        = current_timestep_callback()
    in_range = lo < t < hi                       (strict on both sides)
    compute  = cache is empty or iteration == 0 or not in_range or iteration % block_skip_range == 0      (`pab_decide`)
    output   = module(...) if compute else cache
    cache    = output ;  iteration += 1          (in both cases, also outside the timestep range)

"Output" is the attention module's return value y = T(acc + bias) of its out-projection, before the gate multiply and the
residual add.  The decision is a function of the step counter and the timestep alone: all modules of a kind advance in lockstep,
so one counter per (context, kind) stands for them, the callback is read once per forward, and nothing on the device is read.
A kind whose `*_block_skip_range` is None is never hooked and always computes.  The model asks `_pab_begin` for a forward's
decisions and `_pab_buffer` for a layer's `[rows, D]` cache.

TaylorSeer.  This project's restatement with diffusers' names (diffusers is not vendored by the reference): the rule below is the
contract, and the decision sits in one pure function, `taylorseer_decide`, so that it can be aligned with diffusers in one place.
Per context, s = the 0-based count of forwards since the last reset, W = disable_cache_before_step, N = cache_interval,
A = disable_cache_after_step:

    compute  if  no factor yet  or  s < W  or  (s - (W - 1)) % N == 0  or  (A is not None and s >= A)         else predict

Per (context, hooked tensor) the state is up to max_order + 1 factor planes f_0 .. f_max [rows, D] in the factor dtype F
(`taylor_factors_dtype`, None = the model dtype), the count n of valid planes and s_last, the last computing forward.
A computing forward that sees y, delta = s - s_last forwards after the last one (ops.taylor_update):

    g_0 = F(y);   g_{i+1} = F((float(g_i) - float(f_i)) / float(delta))  for i < min(n, max_order);   f = g, n = min(n + 1, max_order + 1)

A predicting forward, k = s - s_last forwards after it, with c_i = float32(k**i / i!) (ops.taylor_predict):

    p = float(f_0);   p = p + float(f_i) * c_i  for i = 1 .. n - 1        (every operation one fp32 operation)

Default mode hooks what Pyramid Attention Broadcast keeps, the return value y = T(acc + bias) of every block's attn1 and attn2
out-projection: a computing forward is the uncached forward plus one update launch per (layer, kind, segment); a predicting one
runs neither attention branch and adds p to the residual stream with the closing GEMM's epilogue arithmetic,
x = T(fma(p, gate, x)) / x = T(p + x).  Lite mode (`use_lite_mode`) hooks the output head's rows alone: a predicting forward
runs no embedding, no block and no head, it writes T(p) and unpatchifies.  The decision reads the step counter alone -- no
device data, no timestep callback.  `cache_log` gets `(context, s, computed)` per forward.  The model asks `_taylor_begin` for
a forward's decisions and `_taylor_buffer` for a hooked tensor's factor planes; the state's lifetime is Pyramid Attention
Broadcast's.  Selecting modules by `cache_identifiers` / `skip_predict_identifiers` is not implemented.

FasterCache.  This project's restatement with diffusers' names (`FasterCacheConfig`, diffusers/hooks/faster_cache.py; diffusers is
not vendored by the reference): the rule below is the contract, and every decision sits in a pure function
(`fastercache_uncond_decide`, `fastercache_weights`, `fastercache_attention_decide`).  State per context, "cond" and "uncond" as
the loop names them; i = the 0-based count of forwards of that context since the last reset (for "uncond" a skipped forward
counts too), t = float(current_timestep_callback()), read once per forward.

  The unconditional branch.  "uncond" skips its stack iff  has_delta and i > 0 and lo < t < hi (unconditional_batch_timestep_skip_range)
  and i % unconditional_batch_skip_range != 0 and not is_guidance_distilled (a skip range of None: never).  With c, u the model's
  returned predictions [C, F, H, W] of one step under "cond" / "uncond" and LP the radial low-pass of every (c, f) plane (the
  2-D DFT bins with fy^2 + fx^2 <= (min(H, W) // 5)^2 kept):
    computing step (both ran):  D = float(u) - float(c), DL = LP(D), DH = D - DL (fp32; ops.fastercache_delta), aL = aH = 1
    skipping step:              wL = low_frequency_weight_callback(model), or alpha_low_frequency while t lies strictly inside
                                low_frequency_weight_update_timestep_range, else 1 (wH likewise); aL = f32(aL * wL),
                                aH = f32(aH * wH) -- the weights compound over consecutive skips --, and
                                u' = T((float(c) + aL * DL) + aH * DH)  (ops.fastercache_apply) on this step's c
  The model's forward knows three call shapes: batch 2 with `_cache_contexts=("cond", "uncond")` (a skipping step launches the
  stack for the "cond" element alone and row 1 of the result is u'); sequential calls under `cache_context("cond")` then
  `("uncond")` (the "uncond" call of a skipping step returns u' from the conditional prediction the state holds -- by
  reference -- for the same i, RuntimeError if "cond" has not run forward i); anything else: this part is inert.

  Self-attention, on TaylorSeer's hook points and kernels.  The hooked tensor is every block's attn1 return value
  y = T(acc + bias); attn2 always computes.  A forward computes iff spatial_attention_block_skip_range is None or there is no
  plane yet or t is not strictly inside spatial_attention_timestep_skip_range or i % N == 0 or this context did not run its
  stack at forward i - 1.  A computing forward: ops.taylor_update(y, planes, n, delta=1, n_new=min(n + 1, 2)), so f_0 = y_1 and
  f_1 = T(y_1 - y_0); a skipping one runs no attn1 branch and adds ops.taylor_predict(planes, n, coef=[1, w]),
  w = float(attention_weight_callback(attn1 module)), to the residual stream with TaylorSeer's epilogue forms.

  `cache_log` gets `(context, i, t, stack_ran, attention_computed)` per forward and context; the state's lifetime is Pyramid
  Attention Broadcast's.  Temporal attention, module selection by identifier and `tensor_format` other than "BCFHW" match
  nothing on this model.

MagCache.  This project's restatement with diffusers' names (`MagCacheConfig`; diffusers is not installed where this is built, so
parity with it is unpinned by construction): the rule below is the contract, and the decision sits in one pure function,
`magcache_decide`, with no tensor in it.  It skips the WHOLE block stack of a step: with x_in the stack's input (after the patch
embedding) and r = T(x_out - x_in) of the last computing forward, a skipping forward's stack output is T(x_in + r).  Per context the
state is (acc_ratio = 1.0, acc_steps = 0, acc_err = 0.0, has_residual); N = num_inference_steps, R = int(retention_ratio * N + 0.5),
g = ratios[s] (1.0 beyond the curve's end), s = the 0-based count of forwards of the context:

    calibrate: compute.    s < R: compute, the accumulators untouched.    Otherwise:
    acc_ratio *= g;  acc_steps += 1;  acc_err += |1 - acc_ratio|
    skip  iff  has_residual and acc_err <= threshold and acc_steps <= max_skip_steps,  else compute and reset the three

A computing forward stores the residual (ops.step_cache_residual) and sets has_residual, a skipping one leaves it untouched.  When a
context's counter reaches N it starts over -- counter 0, accumulators reset, residual dropped --, as after `_reset_stateful_cache()`.
`mag_ratios` is the per-model curve, the mean over tokens of ||r_t|| / ||r_{t-1}||: a sequence or tensor, resampled to N by nearest
index (`magcache_resample`), or a mapping from cache context to a curve (an unnamed context takes the "cond" entry).  In calibrate
mode every forward computes and one launch (ops.magcache_calibrate) stores the residual and measures, over the rows of the context's
segment, ratio = mean(||r_t|| / (||r_{t-1}|| + 1e-8)) and cos_dist = mean(1 - <r_t, r_{t-1}> / max(||r_t|| ||r_{t-1}||, 1e-8)) -- norms
over the residuals as rounded to the model dtype, in fp32; the first forward records (1, 0) -- into row s of a [N, 2] fp64 device
buffer, which is read ONCE, when the context starts over or the state is reset, and filed as `magcache_calibration[context]`
(`save_mag_ratios` / `load_mag_ratios`).  cos_dist is report-only.  `cache_log` gets `(context, s, computed, acc_err, acc_steps)`, the
accumulators after the decision; `(context, s, True, None, None)` in calibrate mode.  The model asks `_magcache_begin` for a forward's
decisions and `_magcache_finish` after the stack.

TeaCache (`TeaCacheConfig`).  This project's restatement (diffusers is not installed where this is built, so parity with it is
unpinned by construction, as for MagCache): the rule below is the contract, and the decision sits in one pure function,
`teacache_decide`, with no tensor in it.  Like MagCache it skips the WHOLE block stack of a step and re-uses the stack's residual
r = T(x_out - h0) of the last computing forward, T(h0 + r); unlike MagCache it decides from the data, and unlike first-block
caching BEFORE block 0 runs.  Per context, N = num_inference_steps, s = the 0-based count of forwards, h0 = the stack's input:

    m = T(LN(h0) * (1 + scale[sel]) + shift[sel])    block 0's norm1 modulation, bit for bit ops.adaln_modulate's
    d = sum|float(m) - float(p)| / sum|float(p)|     p = the context's plane of its previous forward; two fp64 sums, the quotient
                                                     in Python float; the plane becomes m on EVERY forward
    compute  if  calibrate  or  no plane / residual yet  or  s < ret_steps  or  s >= cutoff_steps (None: N - 1)       acc = 0
    otherwise acc += P(d)  (Horner in Python float, `coefficients` highest power first, as numpy.poly1d)
    skip  iff  acc < rel_l1_thresh and fewer than max_skip_steps (None: no cap) forwards were skipped in a row,
    else compute and acc = 0         (a NaN or inf d computes)

One launch per segment (ops.teacache_probe) forms m, measures it against the plane and stores it over the plane; the host reads
the sums of all segments of the call ONCE, and not at all when every segment computes unconditionally.  `coefficients`: 1 to 8
finite floats, or a mapping from cache context to such a sequence (an unnamed context takes the "cond" entry).  When s reaches N
the context starts over.  In calibrate mode every forward computes, the input sums and the same two sums over the head's output
rows (the probe's plain mode) go into row s of a [N, 4] fp64 device buffer, which is read ONCE, when the context starts over or
the state is reset, and filed as `teacache_calibration[context] = {"rel_l1_in", "rel_l1_out"}` (`fit_teacache_coefficients`,
`save_teacache` / `load_teacache`).  `cache_log` gets `(context, s, computed, d, acc)`: d None where nothing was compared, acc the
value after the decision.  The model asks `_teacache_begin` before the embedding, `_teacache_probe` after it, `_teacache_finish`
after the stack and `_teacache_head` after the output head.

Region-adaptive sampling (`RegionAdaptiveSamplingConfig`, a config of this project; after RAS, Liu et al. 2025, "Region-Adaptive
Sampling for Diffusion Transformers").  The one policy that removes work along the TOKEN axis: a partial forward runs only the La
active token rows of every batch element through the embedding, the blocks and the head; the other rows keep the prediction of
the last forward that computed them and serve every layer's self-attention as keys and values from per-layer K / V planes.  Per
state, s = the 0-based count of forwards since the last reset, W = warmup_steps, N = full_step_interval, E = full_steps_at_end,
T = num_inference_steps (`ras_decide`, a function of s alone):

    full  if  s < W  or  s >= T - E  or  (s - (W - 1)) % N == 0  or  sample_ratio >= 1  or  there are no K / V planes yet

A full forward is the uncached forward (without the shared CFG prefix) whose norm + RoPE stage also writes every layer's K and V
into the planes, and whose head rows `po` are kept; the sit-out counters go to 0.  A partial forward first makes its list from the
kept `po` -- ops.token_score (per row the population standard deviation of its C_out values, averaged over the batch elements
of the call, times exp(starvation_scale * counter); rows outside `live_rows` score -inf, `always_active` rows +inf) and
ops.token_select (the La = max(1, round(sample_ratio * n_eligible)) largest, ties to the lower index, ascending; counters 0 for
the listed rows, + 1 for the others) -- gathers the patch, cos / sin and selector rows, runs every per-token stage on the compact
[b * La, D] buffers with q at lq = La against the planes just refreshed at the active rows (ops.qkv_rmsnorm_rope_rows_), scatters
the head's rows into `po` and returns the unpatchified `po`.  One state per CALL: a batch whose elements are named by
`_cache_contexts` (the pipeline's CFG batch) shares one list, one counter vector and one set of [b * n, D] planes, filed under the
tuple of the names; a call under one `cache_context` files under that name.  State: per layer two planes K (after norm and RoPE)
and V [b * n, D], `po` [b * n, C_out], counters int32 [n] -- 2 planes per context and layer, 9.1 GB for the two contexts of the
30-layer model at 12320 tokens.  Past T forwards every forward is full until the state is reset.  `cache_log` gets
`(context, s, full, rows_run)` per forward and context.  The model asks `_ras_begin` for a forward's decision.

The CogVideoX DiT (`PyramidAttentionBroadcastMixin`) takes Pyramid Attention Broadcast alone, with the same rule and state: its one
attention layer per block, the joint text + video attn1, is the "spatial" kind, and a call's whole batch is one segment under one
context (diffusers' CogVideoX pipelines run the CFG batch under `cache_context("cond_uncond")`).
"""
import contextlib
import dataclasses
import json
import warnings
from types import SimpleNamespace
from typing import Any, Callable, Optional, Tuple

import torch


@dataclasses.dataclass
class FirstBlockCacheConfig:
    """diffusers.FirstBlockCacheConfig: blocks 1 .. N-1 are skipped while the relative L1 change of the first block's residual
    stays at or below `threshold`."""
    threshold: float = 0.05


@dataclasses.dataclass
class PyramidAttentionBroadcastConfig:
    """diffusers.PyramidAttentionBroadcastConfig: an attention kind with a `*_block_skip_range` N recomputes on every N-th
    forward while the timestep lies strictly inside its `*_timestep_skip_range`, and hands out its previous output otherwise.
    `current_timestep_callback` returns the denoising loop's current timestep (`lambda: pipe.current_timestep`).  The temporal
    fields match no layer of the Wan DiT; the `*_block_identifiers` are accepted and ignored (attn1 / attn2 are the layers)."""
    spatial_attention_block_skip_range: Optional[int] = None
    temporal_attention_block_skip_range: Optional[int] = None
    cross_attention_block_skip_range: Optional[int] = None
    spatial_attention_timestep_skip_range: Tuple[int, int] = (100, 800)
    temporal_attention_timestep_skip_range: Tuple[int, int] = (100, 800)
    cross_attention_timestep_skip_range: Tuple[int, int] = (100, 800)
    spatial_attention_block_identifiers: Tuple[str, ...] = ("blocks", "transformer_blocks", "single_transformer_blocks")
    temporal_attention_block_identifiers: Tuple[str, ...] = ("temporal_transformer_blocks",)
    cross_attention_block_identifiers: Tuple[str, ...] = ("blocks", "transformer_blocks")
    current_timestep_callback: Optional[Callable[[], Any]] = None


@dataclasses.dataclass
class TaylorSeerCacheConfig:
    """diffusers.TaylorSeerCacheConfig: after `disable_cache_before_step` warm-up forwards every `cache_interval`-th forward
    computes and refreshes the finite-difference factors (up to `max_order` of them, kept in `taylor_factors_dtype`, None = the
    model dtype); the forwards between extrapolate.  From `disable_cache_after_step` on every forward computes.
    `use_lite_mode` predicts the model's output rows instead of every attention branch's.  Selection of modules by
    `skip_predict_identifiers` / `cache_identifiers` is not implemented: anything but None is refused at `enable_cache`."""
    cache_interval: int = 5
    disable_cache_before_step: int = 3
    disable_cache_after_step: Optional[int] = None
    max_order: int = 1
    taylor_factors_dtype: Optional[torch.dtype] = None
    skip_predict_identifiers: Optional[Tuple[str, ...]] = None
    cache_identifiers: Optional[Tuple[str, ...]] = None
    use_lite_mode: bool = False



@dataclasses.dataclass
class FasterCacheConfig:
    """diffusers.FasterCacheConfig: the unconditional CFG branch runs on every `unconditional_batch_skip_range`-th step while the
    timestep lies strictly inside `unconditional_batch_timestep_skip_range` and is rebuilt in between from the conditional
    prediction plus the frequency-split difference of the last step that ran both; every block's self-attention recomputes on
    every `spatial_attention_block_skip_range`-th forward inside `spatial_attention_timestep_skip_range` and is extrapolated
    from its last two outputs in between.  The temporal fields match no layer of the Wan DiT; the `*_block_identifiers` are
    accepted and ignored."""
    spatial_attention_block_skip_range: Optional[int] = 2
    temporal_attention_block_skip_range: Optional[int] = None
    spatial_attention_timestep_skip_range: Tuple[int, int] = (-1, 681)
    temporal_attention_timestep_skip_range: Tuple[int, int] = (-1, 681)
    low_frequency_weight_update_timestep_range: Tuple[int, int] = (99, 901)
    high_frequency_weight_update_timestep_range: Tuple[int, int] = (-1, 301)
    alpha_low_frequency: float = 1.1
    alpha_high_frequency: float = 1.1
    unconditional_batch_skip_range: Optional[int] = 5
    unconditional_batch_timestep_skip_range: Tuple[int, int] = (-1, 641)
    spatial_attention_block_identifiers: Tuple[str, ...] = ("blocks", "transformer_blocks", "single_transformer_blocks")
    temporal_attention_block_identifiers: Tuple[str, ...] = ("temporal_transformer_blocks",)
    attention_weight_callback: Optional[Callable[[Any], float]] = None
    low_frequency_weight_callback: Optional[Callable[[Any], float]] = None
    high_frequency_weight_callback: Optional[Callable[[Any], float]] = None
    tensor_format: str = "BCFHW"
    is_guidance_distilled: bool = False
    current_timestep_callback: Optional[Callable[[], Any]] = None


@dataclasses.dataclass
class MagCacheConfig:
    """diffusers.MagCacheConfig: after the first `int(retention_ratio * num_inference_steps + 0.5)` steps the whole block stack
    of a step is skipped -- its output is its input plus the stack's residual of the last computing step -- while the error
    accumulated from `mag_ratios` (the per-step mean ratio of the residual's per-token magnitude to the previous step's) stays
    at or below `threshold` and at most `max_skip_steps` steps were skipped in a row.  `mag_ratios`: a sequence or tensor of
    floats, resampled by nearest index to `num_inference_steps`, or (this project's extension) a mapping from cache context to
    such a curve; `calibrate=True` runs every step and records the curve (`model.magcache_calibration`)."""
    threshold: float = 0.06
    max_skip_steps: int = 3
    retention_ratio: float = 0.2
    num_inference_steps: int = 28
    mag_ratios: Any = None
    calibrate: bool = False


@dataclasses.dataclass
class TeaCacheConfig:
    """TeaCache (Liu et al. 2024, "Timestep Embedding Tells: It's Time to Cache for Video Diffusion Model"): the whole block
    stack of a step is skipped -- its output is its input plus the stack's residual of the last computing step -- while the
    accumulated estimate of the output's change stays below `rel_l1_thresh`.  The estimate of one step is a polynomial
    (`coefficients`, highest power first, as numpy.poly1d; a sequence of 1 to 8 floats or a mapping from cache context to one)
    of the relative L1 distance between this step's timestep-modulated input of block 0 and the previous step's.  The first
    `ret_steps` forwards and those from `cutoff_steps` on (None: the last of `num_inference_steps`) always compute;
    `max_skip_steps` caps the skips in a row (None: no cap).  `calibrate=True` runs every step and records the pairs the
    polynomial is fitted to (`model.teacache_calibration`, `fit_teacache_coefficients`)."""
    rel_l1_thresh: float = 0.2
    coefficients: Any = None
    num_inference_steps: int = 50
    ret_steps: int = 1
    cutoff_steps: Optional[int] = None
    max_skip_steps: Optional[int] = None
    calibrate: bool = False


@dataclasses.dataclass
class RegionAdaptiveSamplingConfig:
    """Region-adaptive sampling (a config of this project, not of diffusers): on most steps only a fixed fraction of the token
    rows -- those whose prediction is moving most -- run through the model; the rest keep their last prediction and serve the
    self-attention from per-layer K / V planes.  A partial step runs La = max(1, round(sample_ratio * n_eligible)) rows per batch
    element.  Full steps: the first `warmup_steps`, the last `full_steps_at_end` of `num_inference_steps`, and every
    `full_step_interval`-th counted from the last warm-up step.  A row that has sat out k consecutive partial steps has its score
    multiplied by exp(starvation_scale * k).  `always_active`: a bool [L] mask of rows that are on every list (they count
    towards La; more of them than La: ValueError at the first forward).  Memory: two [rows, D] planes per cache context and
    layer (9.1 GB for the two CFG contexts of the 30-layer model at 12320 tokens)."""
    sample_ratio: float = 0.5
    full_step_interval: int = 5
    warmup_steps: int = 4
    full_steps_at_end: int = 2
    num_inference_steps: int = 50
    starvation_scale: float = 0.1
    always_active: Optional[torch.Tensor] = None


# the other configs diffusers' CacheMixin applies: recognised, not implemented here (none is left)
_OTHER_DIFFUSERS_CONFIGS = ()
_TEA_DEFAULTS = {f.name: f.default for f in dataclasses.fields(TeaCacheConfig)}
TEA_FORMAT = "frameino_amd.teacache"
TEA_MAX_COEFFICIENTS = 8
_MAG_DEFAULTS = {f.name: f.default for f in dataclasses.fields(MagCacheConfig)}
MAG_FORMAT = "frameino_amd.mag_ratios"
_FASTER_DEFAULTS = {f.name: f.default for f in dataclasses.fields(FasterCacheConfig)}
FASTER_CONTEXTS = ("cond", "uncond")    # the cache contexts of the denoising loop the unconditional-branch rule pairs
TAYLOR_MAX_ORDER = 3                     # ops.TAYLOR_MAX_PLANES - 1

_PAB_RANGES = ("spatial_attention_block_skip_range", "temporal_attention_block_skip_range", "cross_attention_block_skip_range")
# the attention kinds of the Wan DiT: (key, block-skip field, timestep-range field)
PAB_KINDS = (("self", "spatial_attention_block_skip_range", "spatial_attention_timestep_skip_range"),
             ("cross", "cross_attention_block_skip_range", "cross_attention_timestep_skip_range"))


def taylorseer_decide(s, n_factors, cfg):
    """True: forward `s` (0-based, per cache context, since the last reset) computes and refreshes the factors; False: it
    predicts.  A function of the step counter alone.  With W = disable_cache_before_step, N = cache_interval and
    A = disable_cache_after_step: compute if there is no factor yet, during the warm-up (s < W), on every N-th forward counted
    from the last warm-up forward ((s - (W - 1)) % N == 0), and from A on."""
    w, n = int(cfg.disable_cache_before_step), int(cfg.cache_interval)
    after = getattr(cfg, "disable_cache_after_step", None)
    return n_factors == 0 or s < w or (s - (w - 1)) % n == 0 or (after is not None and s >= after)


def ras_decide(s, cfg, has_cache=True):
    """True: forward `s` (0-based, per state, since the last reset) under region-adaptive sampling is FULL; False: it runs the
    active rows only.  A function of the step counter alone.  With W = warmup_steps, N = full_step_interval,
    E = full_steps_at_end and T = num_inference_steps: full during the warm-up (s < W), at the end (s >= T - E), on every N-th
    forward counted from the last warm-up forward ((s - (W - 1)) % N == 0), whenever sample_ratio >= 1, and while there are no
    K / V planes yet (`has_cache` False)."""
    w, n = int(cfg.warmup_steps), int(cfg.full_step_interval)
    end = int(cfg.num_inference_steps) - int(cfg.full_steps_at_end)
    return (not has_cache) or float(cfg.sample_ratio) >= 1.0 or s < w or s >= end or (s - (w - 1)) % n == 0


def ras_active_count(sample_ratio, n_eligible):
    """La: the rows a partial forward runs per batch element"""
    return max(1, int(round(float(sample_ratio) * int(n_eligible))))


def _fc(cfg, name):
    """a field of a FasterCache config, diffusers' default where a duck-typed object lacks it"""
    return getattr(cfg, name, _FASTER_DEFAULTS[name])


def _f32(x):
    """x rounded to fp32 (nearest even), as a Python float"""
    return float(torch.tensor(float(x), dtype=torch.float32))


def _strictly_inside(t, rng):
    return rng[0] < t < rng[1]


def fastercache_uncond_decide(i, t, has_delta, cfg):
    """True: forward `i` (0-based, since the last reset) of the "uncond" context at timestep `t` SKIPS its stack and is rebuilt
    from the conditional prediction.  Skip iff there is a delta, i > 0, t lies strictly inside
    `unconditional_batch_timestep_skip_range`, i is no multiple of `unconditional_batch_skip_range`, the model is not
    guidance-distilled and the skip range is not None."""
    n = _fc(cfg, "unconditional_batch_skip_range")
    if n is None or bool(_fc(cfg, "is_guidance_distilled")) or not has_delta or i <= 0:
        return False
    return _strictly_inside(t, _fc(cfg, "unconditional_batch_timestep_skip_range")) and i % int(n) != 0


def fastercache_weights(t, a_low, a_high, cfg, model=None):
    """(aL, aH) of a skipping step at timestep `t` from the weights so far: aL = f32(aL * wL) with
    wL = low_frequency_weight_callback(model) if given, else alpha_low_frequency while t lies strictly inside
    `low_frequency_weight_update_timestep_range`, else 1 (aH likewise): the weights compound over consecutive skips."""
    out = []
    for a, cb, alpha, rng in ((a_low, "low_frequency_weight_callback", "alpha_low_frequency",
                               "low_frequency_weight_update_timestep_range"),
                              (a_high, "high_frequency_weight_callback", "alpha_high_frequency",
                               "high_frequency_weight_update_timestep_range")):
        call = _fc(cfg, cb)
        if call is not None:
            w = float(call(model))
        else:
            w = float(_fc(cfg, alpha)) if _strictly_inside(t, _fc(cfg, rng)) else 1.0
        out.append(float(torch.tensor(float(a), dtype=torch.float32) * torch.tensor(w, dtype=torch.float32)))
    return tuple(out)


def fastercache_attention_decide(i, t, n_planes, ran_prev, cfg):
    """True: forward `i` of a context at timestep `t` COMPUTES its self-attention branches.  Compute iff
    `spatial_attention_block_skip_range` (N) is None, or no plane is kept yet, or t is not strictly inside
    `spatial_attention_timestep_skip_range`, or i % N == 0, or the context did not run its stack at forward i - 1 (an "uncond"
    forward that runs on every fifth step must not extrapolate outputs that old)."""
    n = _fc(cfg, "spatial_attention_block_skip_range")
    if n is None or n_planes == 0 or not ran_prev:
        return True
    return (not _strictly_inside(t, _fc(cfg, "spatial_attention_timestep_skip_range"))) or i % int(n) == 0


def _mc(cfg, name):
    """a field of a MagCache config, diffusers' default where a duck-typed object lacks it"""
    return getattr(cfg, name, _MAG_DEFAULTS[name])


MAG_FRESH = (1.0, 0, 0.0, False)        # (acc_ratio, acc_steps, acc_err, has_residual) of a context that starts over


def magcache_retention(cfg):
    """R: the first R forwards of a context always compute"""
    return int(float(_mc(cfg, "retention_ratio")) * int(_mc(cfg, "num_inference_steps")) + 0.5)


def magcache_decide(s, state, cfg, ratios):
    """(compute, state') of forward `s` (0-based, per cache context) from state = (acc_ratio, acc_steps, acc_err, has_residual)
    and the context's curve `ratios` (1.0 beyond its end).  A function of the step counter and the curve alone: no tensor in
    it.  In calibrate mode and during the first R forwards: compute, the accumulators untouched.  Otherwise acc_ratio *= g,
    acc_steps += 1, acc_err += |1 - acc_ratio|; skip iff there is a residual and acc_err <= threshold and
    acc_steps <= max_skip_steps, else compute and reset the three.  A computing forward leaves has_residual set."""
    acc_ratio, acc_steps, acc_err, has_residual = state
    if bool(_mc(cfg, "calibrate")) or s < magcache_retention(cfg):
        return True, (acc_ratio, acc_steps, acc_err, True)
    g = float(ratios[s]) if ratios is not None and s < len(ratios) else 1.0
    acc_ratio, acc_steps = acc_ratio * g, acc_steps + 1
    acc_err = acc_err + abs(1.0 - acc_ratio)
    if has_residual and acc_err <= float(_mc(cfg, "threshold")) and acc_steps <= int(_mc(cfg, "max_skip_steps")):
        return False, (acc_ratio, acc_steps, acc_err, True)
    return True, MAG_FRESH[:3] + (True,)


def magcache_resample(ratios, n):
    """`ratios` at `n` steps by nearest index: src[round(i * (len - 1) / (n - 1))], for n == 1 the last element; as it is when
    the length is n already"""
    src = [float(v) for v in (ratios.tolist() if isinstance(ratios, torch.Tensor) else ratios)]
    if len(src) == n:
        return src
    if n == 1:
        return [src[-1]]
    return [src[int(round(i * (len(src) - 1) / (n - 1)))] for i in range(n)]


def magcache_curve(cfg, context):
    """the curve of cache context `context`: `mag_ratios` itself, or its entry of a per-context mapping -- for a context the
    mapping does not name, its "cond" entry, ValueError if it has none --, resampled to `num_inference_steps`; None in
    calibrate mode without a curve"""
    ratios = _mc(cfg, "mag_ratios")
    if ratios is None:
        return None
    if hasattr(ratios, "keys"):
        if context in ratios:
            ratios = ratios[context]
        elif "cond" in ratios:
            ratios = ratios["cond"]
        else:
            raise ValueError(f"MagCacheConfig.mag_ratios names the cache contexts {sorted(ratios.keys())}: no curve for context "
                             f"{context!r} and no \"cond\" entry to use instead")
    return magcache_resample(ratios, int(_mc(cfg, "num_inference_steps")))


def save_mag_ratios(path, calibration):
    """the per-context curves of a calibrating run (`model.magcache_calibration`: {context: {"mag_ratios": [...],
    "cos_dist": [...]}}, or {context: [...]}) as plain JSON"""
    ctxs = {}
    for name, entry in calibration.items():
        entry = entry if hasattr(entry, "keys") else {"mag_ratios": entry}
        ctxs[str(name)] = {k: [float(v) for v in entry[k]] for k in ("mag_ratios", "cos_dist") if entry.get(k) is not None}
    with open(path, "w") as f:
        json.dump({"format": MAG_FORMAT, "version": 1, "contexts": ctxs}, f, indent=1)


def load_mag_ratios(path):
    """-> {context: [ratios]} as `save_mag_ratios` wrote it: what `MagCacheConfig(mag_ratios=...)` takes"""
    with open(path) as f:
        d = json.load(f)
    if not isinstance(d, dict) or d.get("format") != MAG_FORMAT or not isinstance(d.get("contexts"), dict):
        raise ValueError(f"{path}: not a file of save_mag_ratios")
    return {name: [float(v) for v in entry["mag_ratios"]] for name, entry in d["contexts"].items()}


def _tc(cfg, name):
    """a field of a TeaCache config, the default where a duck-typed object lacks it"""
    return getattr(cfg, name, _TEA_DEFAULTS[name])


TEA_FRESH = (0.0, 0, False)             # (acc, skipped in a row, ready) of a context that starts over


def teacache_coefficients(cfg, context="cond"):
    """the polynomial of cache context `context`, highest power first: `coefficients` itself, or its entry of a per-context
    mapping -- for a context the mapping does not name, its "cond" entry, ValueError if it has none; None in calibrate mode
    without coefficients"""
    coef = _tc(cfg, "coefficients")
    if coef is None:
        return None
    if hasattr(coef, "keys"):
        if context in coef:
            coef = coef[context]
        elif "cond" in coef:
            coef = coef["cond"]
        else:
            raise ValueError(f"TeaCacheConfig.coefficients names the cache contexts {sorted(coef.keys())}: no polynomial for "
                             f"context {context!r} and no \"cond\" entry to use instead")
    return [float(v) for v in (coef.tolist() if isinstance(coef, torch.Tensor) else coef)]


def teacache_poly(coefficients, d):
    """P(d) by Horner's scheme in Python float, `coefficients` highest power first (numpy.poly1d's order)"""
    p = 0.0
    for c in coefficients:
        p = p * d + c
    return p


def teacache_cutoff(cfg):
    """forwards from this one on always compute: `cutoff_steps`, None = num_inference_steps - 1 (the last step)"""
    cut = _tc(cfg, "cutoff_steps")
    return int(_tc(cfg, "num_inference_steps")) - 1 if cut is None else int(cut)


def teacache_unconditional(s, state, cfg):
    """True: forward `s` computes whatever the data say -- in calibrate mode, without a plane or a residual, during the first
    `ret_steps` forwards and from `cutoff_steps` on.  Such a forward compares nothing, so nothing is read on the host."""
    return bool(_tc(cfg, "calibrate")) or not state[2] or s < int(_tc(cfg, "ret_steps")) or s >= teacache_cutoff(cfg)


def teacache_decide(s, state, cfg, d, context="cond"):
    """(compute, state') of forward `s` (0-based, per cache context) from state = (acc, skipped in a row, ready) and the
    relative L1 distance `d` of this forward's modulated input to the previous one's (None: nothing was compared).  A function
    of numbers alone: no tensor in it.  An unconditional compute (`teacache_unconditional`) sets acc = 0.  Otherwise
    acc += P(d) with the context's polynomial; skip iff acc < rel_l1_thresh and fewer than `max_skip_steps` forwards were
    skipped in a row (None: no cap), else compute and acc = 0.  A NaN or inf d computes: a skip needs acc < thresh to be true.
    Every forward leaves `ready` set: it stores the plane, and the first one of a context computes and stores the residual."""
    acc, skipped, _ = state
    if teacache_unconditional(s, state, cfg) or d is None:
        return True, (0.0, 0, True)
    acc = acc + teacache_poly(teacache_coefficients(cfg, context), float(d))
    cap = _tc(cfg, "max_skip_steps")
    if acc < float(_tc(cfg, "rel_l1_thresh")) and (cap is None or skipped < int(cap)):
        return False, (acc, skipped + 1, True)
    return True, (0.0, 0, True)


def fit_teacache_coefficients(calibrations, degree=4):
    """{context: [degree + 1 coefficients, highest power first]} from one or more calibrating runs
    (`model.teacache_calibration`: {context: {"rel_l1_in": [...], "rel_l1_out": [...]}}; a list of such dicts pools the runs per
    context): numpy.polyfit of the output's relative L1 change over the modulated input's, over every step that has both
    (a context's first step compares nothing and is left out)."""
    import numpy as np
    runs = [calibrations] if hasattr(calibrations, "keys") else list(calibrations)
    pairs = {}
    for run in runs:
        for name, entry in run.items():
            xs, ys = entry["rel_l1_in"], entry["rel_l1_out"]
            if len(xs) != len(ys):
                raise ValueError(f"fit_teacache_coefficients: context {name!r}: {len(xs)} input and {len(ys)} output distances")
            for x, y in zip(xs, ys):
                if x is not None and y is not None and x == x and y == y and abs(x) != float("inf") and abs(y) != float("inf"):
                    pairs.setdefault(str(name), []).append((float(x), float(y)))
    degree = int(degree)
    if not 0 <= degree < TEA_MAX_COEFFICIENTS:
        raise ValueError(f"fit_teacache_coefficients: degree = {degree}: 0 .. {TEA_MAX_COEFFICIENTS - 1}")
    out = {}
    for name, pts in pairs.items():
        if len(pts) <= degree:
            raise ValueError(f"fit_teacache_coefficients: context {name!r} has {len(pts)} measured steps, a polynomial of degree "
                             f"{degree} needs more than {degree}")
        x, y = np.asarray(pts, dtype=np.float64).T
        out[name] = [float(c) for c in np.polyfit(x, y, degree)]
    if not out:
        raise ValueError("fit_teacache_coefficients: no measured step in the calibration")
    return out


def save_teacache(path, coefficients=None, calibration=None):
    """per-context polynomials ({context: [...]}, or one sequence, filed under "cond") and / or the measurements of a calibrating
    run (`model.teacache_calibration`) as plain JSON"""
    ctxs = {}
    if coefficients is not None:
        coefficients = coefficients if hasattr(coefficients, "keys") else {"cond": coefficients}
        for name, coef in coefficients.items():
            ctxs.setdefault(str(name), {})["coefficients"] = [float(v) for v in coef]
    for name, entry in (calibration or {}).items():
        for k in ("rel_l1_in", "rel_l1_out"):
            ctxs.setdefault(str(name), {})[k] = [None if v is None else float(v) for v in entry[k]]
    with open(path, "w") as f:
        json.dump({"format": TEA_FORMAT, "version": 1, "contexts": ctxs}, f, indent=1)


def load_teacache(path):
    """-> {context: [coefficients]} as `save_teacache` wrote it: what `TeaCacheConfig(coefficients=...)` takes.  A file that
    holds measurements alone is fitted first (`fit_teacache_coefficients`, degree 4)."""
    with open(path) as f:
        d = json.load(f)
    if not isinstance(d, dict) or d.get("format") != TEA_FORMAT or not isinstance(d.get("contexts"), dict):
        raise ValueError(f"{path}: not a file of save_teacache")
    ctxs = d["contexts"]
    out = {name: [float(v) for v in entry["coefficients"]] for name, entry in ctxs.items() if "coefficients" in entry}
    rest = {name: entry for name, entry in ctxs.items() if name not in out and "rel_l1_in" in entry}
    if rest:
        out.update(fit_teacache_coefficients(rest))
    if not out:
        raise ValueError(f"{path}: neither coefficients nor measurements in it")
    return out


def pab_decide(iteration, timestep, has_cache, block_skip_range, timestep_skip_range):
    """True: the attention module computes on this forward; False: it hands out its cached output."""
    lo, hi = timestep_skip_range
    in_range = lo < timestep < hi
    return (not has_cache) or iteration == 0 or not in_range or iteration % block_skip_range == 0


def decide(sum_abs_diff, sum_abs_prev, numel, dtype, threshold):
    """(diff, compute) from the probe's fp32 sums, rounded as torch rounds `(r - p).abs().mean() / p.abs().mean()` in `dtype`:
    each mean T(S / N) (fp32 division, one rounding to T), their quotient in T, then a Python float comparison -- NaN skips,
    inf computes."""
    a = (torch.tensor(float(sum_abs_diff), dtype=torch.float32) / numel).to(dtype)
    q = (torch.tensor(float(sum_abs_prev), dtype=torch.float32) / numel).to(dtype)
    diff = float(a / q)
    return diff, diff > threshold


# ---------------------------------------------------------------------- one policy per config
class _CachePolicy:
    """What one cache config states once.  Never instantiated: the class is the policy object a model stores.
    `name`: the config's class name; `required`: the attributes a duck-typed config must carry; `label`: its name in messages
    (`attention_label`: of the part that takes over the attention branches, `instead`: what to use where that part is refused);
    `why_eager`: why one captured step cannot contain it; `batched`: whether the pipeline may run it with a batch > 1;
    `reads_timestep_on_host`: whether it reads the timestep callback several times per step (the loop then keeps a host copy of
    the schedule, so that those reads do not wait for the device)."""
    name = label = attention_label = instead = why_eager = None
    required = ()
    batched = True
    reads_timestep_on_host = False

    @classmethod
    def missing(cls):
        attrs = ", ".join(f"`{a}`" for a in cls.required)
        return NotImplementedError(f"{cls.name}: this object carries the name but not the attributes of diffusers' {cls.name} "
                                   f"that are needed here ({attrs}), so it cannot be applied")

    @classmethod
    def capture_refusal(cls):
        return RuntimeError(f"use_hip_graph=True with {cls.label}: {cls.why_eager}, which one captured step cannot contain (the "
                            f"loop runs eagerly; use_hip_graph=None or False)")

    @staticmethod
    def validate(config, model):
        """ValueError / NotImplementedError for a config this model cannot apply"""

    @staticmethod
    def prepare(config):
        """the enable-time warnings and defaults"""

    @staticmethod
    def loop_begins(config, num_steps):
        """what the sampler loop has to hear once per `denoise`, given the call's step count (a warning, mostly)"""

    @staticmethod
    def hooks_attention(config):
        """whether it takes over the attention branches of the forward"""
        return False

    @classmethod
    def takes_windows(cls, config):
        """whether it runs beside window / sparse attention: unless stated otherwise, when it leaves the attention branches alone"""
        return not cls.hooks_attention(config)

    @classmethod
    def takes_any_processor(cls, config):
        """whether it runs with a user-installed attention processor: unless stated otherwise, likewise"""
        return not cls.hooks_attention(config)

    @staticmethod
    def takes_fp8_attention(config):
        """whether it runs with fp8 self-attention"""
        return True

    # the places of a forward a cache can sit in; None: not there
    @staticmethod
    def segments(model, b, n, contexts):
        """around block 0 and the rest of the stack (`_step_cache_probe` / `_step_cache_finish`): the row segments"""

    @staticmethod
    def lite(model, b, n, d_out, dtype, device, contexts):
        """around the whole stack, on the output head's rows: a plan"""

    @staticmethod
    def branches(model, b, n, d, dtype, device, contexts, faster):
        """in the attention branches of every block: a `_BranchPlan`"""

    @staticmethod
    def magcache(model, b, n, d, dtype, device, contexts):
        """around the block stack, between the embedding and the output head, on the residual stream's rows: a plan"""

    @staticmethod
    def ras(model, b, n, d, d_out, dtype, device, contexts, live, active_rows):
        """along the token axis of the whole forward (region-adaptive sampling): a plan"""

    @staticmethod
    def teacache(model, b, n, d, dtype, device, contexts):
        """around the block stack like `magcache`, decided after the embedding from a probe of block 0's input: a plan"""


class _FirstBlockPolicy(_CachePolicy):
    name, required, label = "FirstBlockCacheConfig", ("threshold",), "first-block caching"
    why_eager = "every step decides on the host between block 0 and block 1 whether the other blocks run"
    batched = False             # diffusers decides jointly over a batch; the pipeline runs the samples one at a time

    @staticmethod
    def validate(config, model):
        if len(model.blocks) < 2:
            raise ValueError(f"FirstBlockCache needs a head block and at least one more block; this model has "
                             f"{len(model.blocks)} block(s), so the head block would also be the tail block")

    @staticmethod
    def segments(model, b, n, contexts):
        return model._context_segments(b, n, contexts)


class _PabPolicy(_CachePolicy):
    name, required, label = "PyramidAttentionBroadcastConfig", _PAB_RANGES + ("current_timestep_callback",), "Pyramid Attention Broadcast"
    instead = "first-block caching is"
    why_eager = "which attention branches a step runs changes from step to step on the host's schedule"

    @staticmethod
    def validate(config, model):
        if config.current_timestep_callback is None:
            raise ValueError("The `current_timestep_callback` function must be provided in the configuration to apply "
                             "Pyramid Attention Broadcast: it returns the denoising loop's current timestep "
                             "(`lambda: pipe.current_timestep`).")

    @staticmethod
    def prepare(config):
        if all(getattr(config, a) is None for a in _PAB_RANGES):
            warnings.warn("Pyramid Attention Broadcast requires one or more of `spatial_attention_block_skip_range`, "
                          "`temporal_attention_block_skip_range` or `cross_attention_block_skip_range` to be set; "
                          "defaulting to `spatial_attention_block_skip_range=2`.", stacklevel=3)
            config.spatial_attention_block_skip_range = 2

    @staticmethod
    def hooks_attention(config):
        return True

    @staticmethod
    def takes_any_processor(config):      # (a processor's return value is what it keeps and hands out)
        return True

    @staticmethod
    def branches(model, b, n, d, dtype, device, contexts, faster):
        return model._pab_begin(b, n, d, dtype, device, contexts)


class _TaylorSeerPolicy(_CachePolicy):
    name, required = "TaylorSeerCacheConfig", ("cache_interval", "disable_cache_before_step", "max_order")
    label = attention_label = "TaylorSeer caching"
    instead = "first-block caching is"
    why_eager = "whether a step computes or predicts changes from step to step on the host's schedule"

    @staticmethod
    def validate(config, model):
        """ValueError for a field outside its range, NotImplementedError for the module selection that is not built"""
        def whole(name, lo, hi=None, optional=False):
            v = getattr(config, name, None)
            if v is None and optional:
                return
            if isinstance(v, bool) or not isinstance(v, int) or v < lo or (hi is not None and v > hi):
                raise ValueError(f"TaylorSeerCacheConfig.{name} = {v!r}: need an integer of at least {lo}"
                                 + (f" and at most {hi}" if hi is not None else "") + (" or None" if optional else ""))
        whole("cache_interval", 1)
        whole("disable_cache_before_step", 1)
        whole("disable_cache_after_step", 0, optional=True)
        whole("max_order", 0, TAYLOR_MAX_ORDER)
        fdt = getattr(config, "taylor_factors_dtype", None)
        if fdt is not None and fdt not in (torch.bfloat16, torch.float16, torch.float32):
            raise ValueError(f"TaylorSeerCacheConfig.taylor_factors_dtype = {fdt!r}: torch.bfloat16, torch.float16, torch.float32 or "
                             f"None (the model dtype)")
        for name in ("skip_predict_identifiers", "cache_identifiers"):
            if getattr(config, name, None) is not None:
                raise NotImplementedError(f"TaylorSeerCacheConfig.{name}: selecting modules by identifier is not implemented; the "
                                          f"hooked tensors are every block's attn1 / attn2 output, or the model's output rows in "
                                          f"lite mode (pass None)")

    @staticmethod
    def hooks_attention(config):
        return not getattr(config, "use_lite_mode", False)

    @staticmethod
    def takes_windows(config):            # (lite mode too: its predicted output rows have not been measured over windows)
        return False

    @staticmethod
    def lite(model, b, n, d_out, dtype, device, contexts):
        return model._taylor_begin(b, n, d_out, dtype, device, contexts) if model._taylor_lite else None

    @staticmethod
    def branches(model, b, n, d, dtype, device, contexts, faster):
        return None if model._taylor_lite else model._taylor_begin(b, n, d, dtype, device, contexts)


class _FasterCachePolicy(_CachePolicy):
    name = "FasterCacheConfig"
    required = ("spatial_attention_block_skip_range", "unconditional_batch_skip_range", "current_timestep_callback")
    label, attention_label = "FasterCache", "FasterCache's self-attention extrapolation"
    instead = "`spatial_attention_block_skip_range=None` keeps its unconditional-branch part alone, which is"
    why_eager = ("whether a step runs the unconditional branch and its self-attention branches changes from step to step on the "
                 "host's schedule")
    reads_timestep_on_host = True       # up to three times per step

    @staticmethod
    def validate(config, model):
        """ValueError for a field outside its range or a missing `current_timestep_callback`"""
        for name in ("spatial_attention_block_skip_range", "temporal_attention_block_skip_range", "unconditional_batch_skip_range"):
            v = _fc(config, name)
            if v is not None and (isinstance(v, bool) or not isinstance(v, int) or v < 1):
                raise ValueError(f"FasterCacheConfig.{name} = {v!r}: need an integer of at least 1, or None")
        for name in ("spatial_attention_timestep_skip_range", "temporal_attention_timestep_skip_range",
                     "unconditional_batch_timestep_skip_range", "low_frequency_weight_update_timestep_range",
                     "high_frequency_weight_update_timestep_range"):
            v = _fc(config, name)
            ok = isinstance(v, (tuple, list)) and len(v) == 2 and all(isinstance(e, (int, float)) and not isinstance(e, bool)
                                                                      and e == e for e in v)
            if not ok or not v[0] < v[1]:
                raise ValueError(f"FasterCacheConfig.{name} = {v!r}: need a pair (lo, hi) of numbers with lo < hi")
        for name in ("alpha_low_frequency", "alpha_high_frequency"):
            v = _fc(config, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not (0.0 <= float(v) < float("inf")):
                raise ValueError(f"FasterCacheConfig.{name} = {v!r}: need a finite number of at least 0")
        for name in ("attention_weight_callback", "low_frequency_weight_callback", "high_frequency_weight_callback"):
            v = _fc(config, name)
            if v is not None and not callable(v):
                raise ValueError(f"FasterCacheConfig.{name} = {v!r}: need a callable or None")
        if _fc(config, "tensor_format") != "BCFHW":
            raise ValueError(f"FasterCacheConfig.tensor_format = {_fc(config, 'tensor_format')!r}: this model's predictions are "
                             f'"BCFHW" (the low-pass runs over the (H, W) planes)')
        if config.current_timestep_callback is None:
            raise ValueError("The `current_timestep_callback` function must be provided in the configuration to apply FasterCache: "
                             "it returns the denoising loop's current timestep (`lambda: pipe.current_timestep`).")

    @staticmethod
    def prepare(config):
        if _fc(config, "spatial_attention_block_skip_range") is not None and _fc(config, "attention_weight_callback") is None:
            warnings.warn("FasterCacheConfig: no `attention_weight_callback` provided; defaulting to 0.5 for every "
                          "attention module.", stacklevel=3)

    @staticmethod
    def hooks_attention(config):
        return _fc(config, "spatial_attention_block_skip_range") is not None

    @staticmethod
    def branches(model, b, n, d, dtype, device, contexts, faster):
        return model._faster_attention_plan(faster, b, n, d, dtype, device)


class _MagCachePolicy(_CachePolicy):
    name = "MagCacheConfig"
    required = ("threshold", "max_skip_steps", "retention_ratio", "num_inference_steps", "mag_ratios", "calibrate")
    label = "MagCache"
    why_eager = "whether a step runs its block stack or re-uses the last residual changes from step to step on the host's schedule"

    @staticmethod
    def validate(config, model):
        """ValueError for a field outside its range, a curve that is no curve, or neither a curve nor `calibrate`"""
        def number(name, ok, need):
            v = getattr(config, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not ok(v):
                raise ValueError(f"MagCacheConfig.{name} = {v!r}: need {need}")
        number("threshold", lambda v: 0.0 <= v < float("inf"), "a finite number of at least 0")
        number("retention_ratio", lambda v: 0.0 <= v <= 1.0, "a number between 0 and 1")
        for name, lo in (("max_skip_steps", 0), ("num_inference_steps", 1)):
            v = getattr(config, name)
            if isinstance(v, bool) or not isinstance(v, int) or v < lo:
                raise ValueError(f"MagCacheConfig.{name} = {v!r}: need an integer of at least {lo}")
        ratios = config.mag_ratios
        if ratios is None:
            if not config.calibrate:
                raise ValueError("MagCacheConfig.mag_ratios is None and calibrate is False: MagCache needs the model's curve.  "
                                 "Run the clip once with MagCacheConfig(calibrate=True, num_inference_steps=N), take the curves "
                                 "from `transformer.magcache_calibration` (save_mag_ratios / load_mag_ratios) and pass them as "
                                 "`mag_ratios`.")
            return
        if hasattr(ratios, "keys") and not len(ratios):
            raise ValueError("MagCacheConfig.mag_ratios is an empty mapping: need one curve per cache context")
        for ctx, curve in (ratios.items() if hasattr(ratios, "keys") else ((None, ratios),)):
            where = "MagCacheConfig.mag_ratios" + ("" if ctx is None else f"[{ctx!r}]")
            try:
                values = [float(v) for v in (curve.tolist() if isinstance(curve, torch.Tensor) else curve)]
            except (TypeError, ValueError):
                raise ValueError(f"{where} = {curve!r}: need a sequence or tensor of floats") from None
            if not values or not all(0.0 < v < float("inf") for v in values):
                raise ValueError(f"{where}: need at least one ratio, every one finite and above 0")

    @staticmethod
    def loop_begins(config, num_steps):
        planned = int(config.num_inference_steps)
        if planned != num_steps:            # once per call: the curve is indexed by the step counter
            warnings.warn(f"MagCache: this call runs {num_steps} steps, the config says num_inference_steps={planned}; "
                          f"its curve (`mag_ratios`, resampled to {planned} entries) is misaligned with the loop and a "
                          f"context starts over after {planned} forwards.  Build the config with the call's step count.",
                          stacklevel=4)

    @staticmethod
    def magcache(model, b, n, d, dtype, device, contexts):
        return model._magcache_begin(b, n, d, dtype, device, contexts)


class _TeaCachePolicy(_CachePolicy):
    name = "TeaCacheConfig"
    required = ("rel_l1_thresh", "coefficients", "num_inference_steps")
    label = "TeaCache"
    why_eager = ("whether a step runs its block stack or re-uses the last residual is decided on the host from what the step's "
                 "probe measured")

    @staticmethod
    def validate(config, model):
        """ValueError for a field outside its range, coefficients that are no polynomial, or neither coefficients nor
        `calibrate`"""
        v = config.rel_l1_thresh
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not (0.0 <= v < float("inf")):
            raise ValueError(f"TeaCacheConfig.rel_l1_thresh = {v!r}: need a finite number of at least 0")
        for name, lo, optional in (("num_inference_steps", 1, False), ("ret_steps", 0, False), ("cutoff_steps", 0, True),
                                   ("max_skip_steps", 0, True)):
            v = _tc(config, name)
            if v is None and optional:
                continue
            if isinstance(v, bool) or not isinstance(v, int) or v < lo:
                raise ValueError(f"TeaCacheConfig.{name} = {v!r}: need an integer of at least {lo}" + (" or None" if optional else ""))
        coef = config.coefficients
        if coef is None:
            if not _tc(config, "calibrate"):
                raise ValueError("TeaCacheConfig.coefficients is None and calibrate is False: TeaCache needs the model's polynomial.  "
                                 "Run the clip once with TeaCacheConfig(calibrate=True, num_inference_steps=N), fit "
                                 "`transformer.teacache_calibration` (fit_teacache_coefficients; save_teacache / load_teacache) and "
                                 "pass the result as `coefficients`.")
            return
        if hasattr(coef, "keys") and not len(coef):
            raise ValueError("TeaCacheConfig.coefficients is an empty mapping: need one polynomial per cache context")
        for ctx, poly in (coef.items() if hasattr(coef, "keys") else ((None, coef),)):
            where = "TeaCacheConfig.coefficients" + ("" if ctx is None else f"[{ctx!r}]")
            try:
                values = [float(c) for c in (poly.tolist() if isinstance(poly, torch.Tensor) else poly)]
            except (TypeError, ValueError):
                raise ValueError(f"{where} = {poly!r}: need a sequence of floats, highest power first") from None
            if not 1 <= len(values) <= TEA_MAX_COEFFICIENTS or not all(abs(c) < float("inf") for c in values):
                raise ValueError(f"{where}: need 1 to {TEA_MAX_COEFFICIENTS} coefficients, every one finite")

    @staticmethod
    def loop_begins(config, num_steps):
        planned = int(config.num_inference_steps)
        if planned != num_steps:            # once per call: the last step and the start-over are counted from the config's figure
            warnings.warn(f"TeaCache: this call runs {num_steps} steps, the config says num_inference_steps={planned}; the "
                          f"forwards that always compute (`cutoff_steps`, None = {planned} - 1) are misaligned with the loop and "
                          f"a context starts over after {planned} forwards.  Build the config with the call's step count.",
                          stacklevel=4)

    @staticmethod
    def teacache(model, b, n, d, dtype, device, contexts):
        return model._teacache_begin(b, n, d, dtype, device, contexts)


class _RegionAdaptivePolicy(_CachePolicy):
    name = "RegionAdaptiveSamplingConfig"
    required = ("sample_ratio", "full_step_interval", "warmup_steps", "full_steps_at_end", "num_inference_steps",
                "starvation_scale", "always_active")
    label = attention_label = "region-adaptive sampling"
    instead = "first-block caching is"
    why_eager = "whether a step runs every token row or the active ones alone changes from step to step on the host's schedule"
    batched = True              # (the list comes from the call's own rows: the samples of a batch run one at a time, as under PAB)

    @staticmethod
    def validate(config, model):
        """ValueError for a field outside its range or a mask that is no bool vector"""
        r = config.sample_ratio
        if isinstance(r, bool) or not isinstance(r, (int, float)) or not (0.0 < float(r) <= 1.0):
            raise ValueError(f"RegionAdaptiveSamplingConfig.sample_ratio = {r!r}: need a number in (0, 1]")
        for name, lo in (("full_step_interval", 1), ("warmup_steps", 1), ("full_steps_at_end", 0), ("num_inference_steps", 1)):
            v = getattr(config, name)
            if isinstance(v, bool) or not isinstance(v, int) or v < lo:
                raise ValueError(f"RegionAdaptiveSamplingConfig.{name} = {v!r}: need an integer of at least {lo}")
        v = config.starvation_scale
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not (0.0 <= float(v) < float("inf")):
            raise ValueError(f"RegionAdaptiveSamplingConfig.starvation_scale = {v!r}: need a finite number of at least 0")
        m = config.always_active
        if m is not None and (not isinstance(m, torch.Tensor) or m.dtype != torch.bool or m.dim() != 1):
            raise ValueError(f"RegionAdaptiveSamplingConfig.always_active: need a bool [L] tensor or None, got "
                             f"{type(m).__name__}" + (f" {m.dtype} {tuple(m.shape)}" if isinstance(m, torch.Tensor) else ""))

    @staticmethod
    def loop_begins(config, num_steps):
        planned = int(config.num_inference_steps)
        if planned != num_steps:            # once per call: the full steps at the end are counted from the config's figure
            warnings.warn(f"region-adaptive sampling: this call runs {num_steps} steps, the config says "
                          f"num_inference_steps={planned}; its full steps at the end sit at forwards {planned} - "
                          f"full_steps_at_end and later, and every forward from {planned} on is full.  Build the config "
                          f"with the call's step count.", stacklevel=4)

    @staticmethod
    def hooks_attention(config):          # (the self-attention reads the planes: no window, no tile mask, no user processor)
        return True

    @staticmethod
    def takes_fp8_attention(config):      # (the planes are kept in the model dtype and read by the bf16 / fp16 kernel)
        return False

    @staticmethod
    def ras(model, b, n, d, d_out, dtype, device, contexts, live, active_rows):
        return model._ras_begin(b, n, d, d_out, dtype, device, contexts, live, active_rows)


_POLICIES = {p.name: p for p in (_FirstBlockPolicy, _PabPolicy, _TaylorSeerPolicy, _FasterCachePolicy, _MagCachePolicy,
                                 _TeaCachePolicy, _RegionAdaptivePolicy)}


# ---------------------------------------------------------------------- one plan for the attention branches of a forward
def _pab_buffer(seg, kind, layer, d=None, dtype=None, device=None):
    """the cache of attention module (kind, layer) under the segment's context: [rows, D] in the model dtype, allocated by
    the first forward that computes (pass d / dtype / device); a reuse step finds it there (KeyError: it never computed)"""
    buf = seg.state.buffers.get((kind, layer))
    if buf is None:
        if d is None:
            raise KeyError(f"Pyramid Attention Broadcast: no cached output of the {kind}-attention of block {layer} under "
                           f"context {seg.name!r}")
        buf = seg.state.buffers[(kind, layer)] = torch.empty((seg.r1 - seg.r0, d), dtype=dtype, device=device)
    return buf


def _taylor_buffer(plan, seg, key, d=None, device=None):
    """the factor planes of hooked tensor `key` ((kind, layer), or "out" in lite mode) under the segment's context:
    [max_order + 1, rows, D] in the factor dtype, allocated by the first forward that computes (pass d / device); a
    predicting step finds them there (KeyError: it never computed)"""
    buf = seg.state.buffers.get(key)
    if buf is None:
        if d is None:
            raise KeyError(f"TaylorSeer: no factors of {key!r} under context {seg.name!r}")
        buf = seg.state.buffers[key] = torch.empty((plan.planes, seg.r1 - seg.r0, d), dtype=plan.factor_dtype, device=device)
    return buf


class _BranchPlan:
    """One forward's decisions for the attention branches a cache has taken over, made before anything is launched: `.hooked[kind]`,
    and `.segs` = one entry per row segment (a batch element under its own context, or the whole batch under one) with `.name`,
    `.r0`, `.r1`, `.state` and `.compute[kind]`.  `d`, `dtype`, `device`: of the hooked rows.  For the rows [r0, r1) of the call
    that one launch of a branch covers (inside one segment) a plan answers: `kept` -- where a computing branch's
    y = T(acc + bias) is kept (the closing GEMM's `keep=`); `computed` -- what runs after that branch; `reuse` -- the one launch
    that stands for a branch that does not run, x += gate * y' / x += y' with the closing GEMM's epilogue arithmetic."""
    taylor, lite = None, False

    def __init__(self, hooked, d, dtype, device, **fields):
        self.segs, self.hooked, self.d, self.dtype, self.device = [], hooked, d, dtype, device
        vars(self).update(fields)

    def segment(self, row):
        """the segment row `row` of the call lies in"""
        return next(s for s in self.segs if s.r0 <= row < s.r1)


class _BroadcastPlan(_BranchPlan):
    """Pyramid Attention Broadcast: y stays in the segment's [rows, D] buffer of (kind, layer) and is handed out as it is"""

    def kept(self, ws, seg, kind, layer, r0, r1):
        buf = _pab_buffer(seg, kind, layer, self.d, self.dtype, self.device)
        return buf if (r0, r1) == (seg.r0, seg.r1) else buf[r0 - seg.r0:r1 - seg.r0]

    def computed(self, ops, seg, kind, layer, r0, r1, y):
        pass

    def reuse(self, ops, seg, kind, layer, r0, r1, x, gate, sel, module=None, fused=True, **epilogue):
        """bit for bit what the step that computed y wrote: the fused epilogues multiply-add once (`ops.pab_broadcast`), a
        custom processor's result (and a staged epilogue's, `staged=True`) went through `ops.gated_residual`"""
        buf = _pab_buffer(seg, kind, layer)
        y = buf if (r0, r1) == (seg.r0, seg.r1) else buf[r0 - seg.r0:r1 - seg.r0]
        (ops.pab_broadcast if fused else ops.gated_residual)(x, y, gate, sel, out=x, **epilogue)


class _TaylorPlan(_BranchPlan):
    """TaylorSeer's default mode and FasterCache's self-attention part: y waits in the workspace's one [n, D] scratch for the
    update launch that folds it into the factor planes of (kind, layer); a branch that does not run is extrapolated from them.
    Per segment also `.s` (this forward's number), `.k` (its distance to the last computing forward: the `delta` of an update,
    the offset of a prediction) and `.n_old` / `.n_new` (the valid planes before and after a computing forward).  `weight`
    (FasterCache): the prediction is f_0 + w * f_1, w = weight(attention module), instead of the Taylor series in k."""
    weight = None

    def kept(self, ws, seg, kind, layer, r0, r1):
        if getattr(ws, "taylor_y", None) is None:
            ws.taylor_y = torch.empty((r1 - r0, self.d), dtype=self.dtype, device=self.device)
        return ws.taylor_y

    def computed(self, ops, seg, kind, layer, r0, r1, y):
        f = _taylor_buffer(self, seg, (kind, layer), self.d, self.device)[:, r0 - seg.r0:r1 - seg.r0]
        ops.taylor_update(y, f, seg.n_old, seg.k, seg.n_new)

    def reuse(self, ops, seg, kind, layer, r0, r1, x, gate, sel, module=None, fused=True):
        f = _taylor_buffer(self, seg, (kind, layer))[:, r0 - seg.r0:r1 - seg.r0]
        coef = {} if self.weight is None else {"coef": [1.0, self.weight(module)]}
        ops.taylor_predict(f, seg.n_old, seg.k, x, gate, sel, out=x, **coef)


class StepCacheMixin:
    """diffusers' CacheMixin surface (enable_cache / disable_cache / is_cache_enabled / _reset_stateful_cache) over the policies
    in `_cache_policies`.  `enable_cache` looks the config's policy up, lets it validate, asks the model what it cannot be
    combined with (`_cache_refusals`) and stores it next to the config; the forward asks the stored policy for its entry points
    (`segments` / `lite` / `branches` / `magcache`), which lead to `_step_cache_segments` + `_step_cache_probe` + `_step_cache_finish`
    (first-block caching), `_pab_begin`, `_taylor_begin`, `_faster_begin` + `_faster_attention_plan` and `_magcache_begin` +
    `_magcache_finish`.

    State per cache-context name (`_cache_state`: made at first use, and again when the rows, width, dtype or device change);
    `cache_log` holds one row per forward and context since the last reset; it survives the reset at the end of a pipeline call,
    so the call's decisions can be read after it.
    First-block caching: the head residual (plus a spare buffer the next probe writes into), the tail residual and a step
    counter; log rows `(context, step, diff, computed)` (diff None: no previous residual).
    Pyramid Attention Broadcast: per kind a counter, per (kind, layer) a [rows, D] buffer in the model dtype, allocated by the
    first forward that computes; log rows `(context, iteration, float(timestep), self_attention_computed,
    cross_attention_computed)`.
    TaylorSeer: a counter, the number of valid factor planes and the last computing forward, per hooked tensor a
    [max_order + 1, rows, D] buffer in the factor dtype, allocated by the first forward that computes; log rows
    `(context, step, computed)`.
    FasterCache: a counter, the self-attention planes, the context's last prediction (by reference) and, for "uncond", the
    delta and its weights; log rows `(context, i, t, stack_ran, attention_computed)`.
    MagCache: a counter, the three accumulators, the stack's residual [rows, D] and, in calibrate mode, the [N, 2] fp64 rows;
    log rows `(context, s, computed, acc_err, acc_steps)`.
    TeaCache: a counter, (acc, skips in a row, ready), the modulated-input plane [rows, D], the stack's residual [rows, D] and,
    in calibrate mode, the head-row plane and the [N, 4] fp64 rows; log rows `(context, s, computed, d, acc)`."""
    _cache_policies = (_FirstBlockPolicy, _PabPolicy, _TaylorSeerPolicy, _FasterCachePolicy, _MagCachePolicy,
                       _TeaCachePolicy, _RegionAdaptivePolicy)
    magcache_calibration = None     # {context: {"mag_ratios": [...], "cos_dist": [...]}} once a calibrating context finished
    teacache_calibration = None     # {context: {"rel_l1_in": [...], "rel_l1_out": [...]}} likewise
    _step_cache_config = None
    _step_cache_policy = None
    _step_cache_states = None
    _step_cache_log_fresh = True
    _faster_defer_delta = False
    cache_log = ()

    @property
    def is_cache_enabled(self):
        return self._step_cache_config is not None

    def enable_cache(self, config):
        if self.is_cache_enabled:
            raise ValueError(f"Caching has already been enabled with {type(self._step_cache_config)}. To apply a new caching "
                             f"technique, please disable the existing one first.")
        name = type(config).__name__
        policy = _POLICIES.get(name)
        if policy not in self._cache_policies:
            if policy is not None or name in _OTHER_DIFFUSERS_CONFIGS or (
                    name.endswith("CacheConfig") and type(config).__module__.split(".")[0] == "diffusers"):
                *some, last = [p.name for p in self._cache_policies]
                have = f"{', '.join(some)} and {last} are" if some else f"{last} is"
                raise NotImplementedError(f"{name} is not implemented on {type(self).__name__}; {have}")
            raise ValueError(f"Cache config {type(config)} is not supported.")
        if not all(hasattr(config, a) for a in policy.required):
            raise policy.missing()
        policy.validate(config, self)
        self._cache_refusals(policy, config, enabling=True)
        policy.prepare(config)
        self._step_cache_config, self._step_cache_policy = config, policy
        self._reset_stateful_cache()

    def disable_cache(self):
        if self._step_cache_config is None:
            warnings.warn("Caching techniques have not been enabled, so there's nothing to disable.", stacklevel=2)
            return
        self._step_cache_config = None
        del self._step_cache_policy               # (the class's None again: the model is as it was before `enable_cache`)
        self._reset_stateful_cache()

    def _cache_refusals(self, policy=None, config=None, **where):
        """NotImplementedError for what this model does not combine with a step cache; a model with such limits states them
        here, once, for both orders (WanTransformer3DModel)"""

    def _reset_stateful_cache(self, recurse=True):
        """drop every context's state (diffusers' maybe_free_model_hooks calls this at the end of a pipeline call); the next
        forward starts a new `cache_log`.  A calibrating MagCache context files what it has recorded first."""
        for name, st in (self._step_cache_states or {}).items():
            self._magcache_file(name, st)
            self._teacache_file(name, st)
        self._step_cache_states = {}
        self._step_cache_log_fresh = True

    # the flags tests, tools, window_attention.py and the pipelines read: views of the stored policy
    _pab_on = property(lambda self: self._step_cache_policy is _PabPolicy)
    _taylor_on = property(lambda self: self._step_cache_policy is _TaylorSeerPolicy)
    _taylor_lite = property(lambda self: self._taylor_on and not _TaylorSeerPolicy.hooks_attention(self._step_cache_config))
    _faster_on = property(lambda self: self._step_cache_policy is _FasterCachePolicy)
    _faster_attention = property(lambda self: self._faster_on and _FasterCachePolicy.hooks_attention(self._step_cache_config))
    _mag_on = property(lambda self: self._step_cache_policy is _MagCachePolicy)
    _tea_on = property(lambda self: self._step_cache_policy is _TeaCachePolicy)
    _ras_on = property(lambda self: self._step_cache_policy is _RegionAdaptivePolicy)

    # ---------------------------------------------------------------- used by the forward
    def _context_segments(self, b, n, contexts):
        """[(context, first row, end row)] of the call's [b * n, D] rows: one segment per batch element when `contexts` names one
        context each (the pipeline's CFG-batched call), else one joint segment under the current `cache_context`."""
        if contexts is not None:
            contexts = tuple(contexts)
            if len(contexts) != b or len(set(contexts)) != b:
                raise ValueError(f"_cache_contexts {contexts}: need {b} distinct names, one per batch element")
            return [(c, i * n, (i + 1) * n) for i, c in enumerate(contexts)]
        if self._ctx_name is None:
            raise ValueError("No context is set. Please set a context before retrieving the state.")
        return [(self._ctx_name, 0, b * n)]

    def _cache_state(self, name, key, fresh):
        """the state of context `name`: a step counter plus the fields `fresh()` returns, made at first use and again whenever
        `key` -- shape, dtype, device -- changes; the first forward after a reset starts a new `cache_log`"""
        if self._step_cache_log_fresh or not isinstance(self.cache_log, list):
            self.cache_log = []
            self._step_cache_log_fresh = False
        if self._step_cache_states is None:
            self._step_cache_states = {}
        st = self._step_cache_states.get(name)
        if st is None or st.key != key:
            st = self._step_cache_states[name] = SimpleNamespace(key=key, steps=0, **fresh())
        return st

    # ---------------------------------------------------------------- first-block caching
    def _step_cache_segments(self, b, n, contexts=None):
        """None unless first-block caching is on (nothing extra is allocated or launched), else `_context_segments`"""
        return None if self._step_cache_policy is None else self._step_cache_policy.segments(self, b, n, contexts)

    def _step_cache_probe(self, segs, h0, h1, h1_copy):
        """after block 0: probe, one host read, decide.  Returns one bool per segment (True: compute blocks 1 .. N-1)."""
        d, dt, dev = h1.shape[1], h1.dtype, h1.device
        sts = [self._cache_state(name, (r1 - r0, d, dt, str(dev)), lambda: dict(head=None, spare=None, tail=None))
               for name, r0, r1 in segs]
        for (name, r0, r1), st in zip(segs, sts):
            if st.spare is None:
                st.spare = torch.empty((r1 - r0, d), dtype=dt, device=dev)
        sums = self.ops.step_cache_probe([h0[r0:r1] for _, r0, r1 in segs], [h1[r0:r1] for _, r0, r1 in segs],
                                         [st.head for st in sts], [st.spare for st in sts],
                                         [h1_copy[r0:r1] for _, r0, r1 in segs]).tolist()     # the host read
        thr = float(self._step_cache_config.threshold)
        out = []
        for (name, r0, r1), st, (sa, sq) in zip(segs, sts, sums):
            if st.head is None or st.tail is None:
                diff, compute = None, True
            else:
                diff, compute = decide(sa, sq, (r1 - r0) * d, dt, thr)
            self.cache_log.append((name, st.steps, diff, compute))
            st.steps += 1
            if compute:
                st.head, st.spare = st.spare, st.head
            out.append(compute)
        return out

    def _step_cache_finish(self, segs, computes, x, h1_copy):
        """after the last block (or right after block 0 when every segment skips): a computed segment stores its tail residual
        T(hN - h1); a skipped one takes T(tail + h1) as the stack's output, its state untouched."""
        o = self.ops
        for (name, r0, r1), compute in zip(segs, computes):
            st = self._step_cache_states[name]
            if compute:
                if st.tail is None:
                    st.tail = torch.empty_like(st.head)
                o.step_cache_residual(x[r0:r1], h1_copy[r0:r1], out=st.tail, subtract=True)
            else:
                o.step_cache_residual(st.tail, h1_copy[r0:r1], out=x[r0:r1], subtract=False)

    # ---------------------------------------------------------------- Pyramid Attention Broadcast
    def _pab_begin(self, b, n, d, dtype, device, contexts=None):
        """The decisions of one forward, taken before anything is launched: None when Pyramid Attention Broadcast is off, else
        a `_BroadcastPlan`.  Reads the timestep callback ONCE (a device tensor costs its one host read here, not one per
        layer), advances every hooked kind's counter and appends to `cache_log`.  A context whose rows, width, dtype or
        device changed starts over (the model switches `live_rows` off under this cache, so there is no live-row range to
        key on)."""
        if not self._pab_on:
            return None
        cfg = self._step_cache_config
        segs = self._context_segments(b, n, contexts)
        t = float(cfg.current_timestep_callback())
        hooked = {kind: getattr(cfg, rng) is not None for kind, rng, _ in PAB_KINDS}
        plan = _BroadcastPlan(hooked, d, dtype, device, timestep=t)
        for name, r0, r1 in segs:
            st = self._cache_state(name, (r1 - r0, d, dtype, str(device)), lambda: dict(iteration={k: 0 for k in hooked}, buffers={}))
            compute = {}
            for kind, rng, tsr in PAB_KINDS:
                if not hooked[kind]:
                    compute[kind] = True
                    continue
                has_cache = any(k == kind for k, _ in st.buffers)
                compute[kind] = pab_decide(st.iteration[kind], t, has_cache, getattr(cfg, rng), getattr(cfg, tsr))
                st.iteration[kind] += 1
            self.cache_log.append((name, st.steps, t, compute["self"], compute["cross"]))
            st.steps += 1
            plan.segs.append(SimpleNamespace(name=name, r0=r0, r1=r1, state=st, compute=compute))
        return plan

    _pab_buffer = staticmethod(_pab_buffer)

    # ---------------------------------------------------------------- TaylorSeer
    def _taylor_begin(self, b, n, d, dtype, device, contexts=None):
        """The decisions of one forward under TaylorSeer, taken before anything is launched: None when it is off, else a
        `_TaylorPlan` (both kinds hooked and decided alike) with `.taylor` (the config), `.planes`, `.factor_dtype` and `.lite`.
        `d` / `dtype`: width and dtype of the hooked rows (lite mode: the output head's).  Advances every context's counter,
        moves `n` and `s_last` of a computing context on, and appends `(context, s, computed)` to `cache_log`.  A context
        whose rows, width, dtype or device changed starts over."""
        if not self._taylor_on:
            return None
        cfg = self._step_cache_config
        segs = self._context_segments(b, n, contexts)
        planes = int(cfg.max_order) + 1
        fdt = getattr(cfg, "taylor_factors_dtype", None) or dtype
        plan = _TaylorPlan({"self": True, "cross": True}, d, dtype, device, taylor=cfg, planes=planes, factor_dtype=fdt,
                           lite=self._taylor_lite)
        for name, r0, r1 in segs:
            st = self._cache_state(name, (r1 - r0, d, dtype, str(device)), lambda: dict(n=0, s_last=None, buffers={}))
            s = st.steps
            compute = bool(taylorseer_decide(s, st.n, cfg))
            k = 0 if st.s_last is None else s - st.s_last
            seg = SimpleNamespace(name=name, r0=r0, r1=r1, state=st, compute={"self": compute, "cross": compute}, s=s, k=k,
                                  n_old=st.n, n_new=min(st.n + 1, planes) if compute else st.n)
            self.cache_log.append((name, s, compute))
            st.steps += 1
            if compute:
                st.n, st.s_last = seg.n_new, s
            plan.segs.append(seg)
        return plan

    _taylor_buffer = staticmethod(_taylor_buffer)

    # ---------------------------------------------------------------- FasterCache
    def _faster_will_skip(self):
        """whether the NEXT "uncond" forward of the denoising loop skips its stack (nothing is advanced): the loop's two-stream
        path asks before it forks"""
        if not self._faster_on:
            return False
        cfg = self._step_cache_config
        st = (self._step_cache_states or {}).get("uncond")
        if st is None:
            return False
        return bool(fastercache_uncond_decide(st.steps, float(cfg.current_timestep_callback()), st.has_delta, cfg))

    def _faster_begin(self, b, shape, dtype, device, contexts=None):
        """The decisions of one forward under FasterCache, taken before anything is launched: None when it is off, else a
        plan with `.t` (the timestep callback, read ONCE), `.mode` -- "batched" (batch 2 as ("cond", "uncond")), "cond" /
        "uncond" (a batch-1 call under that cache context) or None (any other call: the unconditional-branch rule is inert) --,
        `.skip` (this call's "uncond" does not run the stack) and `.entries` = one per context of the call with `.name`,
        `.state`, `.i`, `.stack` (whether its stack runs) and `.compute` (whether its self-attention branches compute).
        Advances every context's counter and appends `(context, i, t, stack_ran, attention_computed)` to `cache_log`."""
        if not self._faster_on:
            return None
        cfg = self._step_cache_config
        names = tuple(name for name, _, _ in self._context_segments(b, 1, contexts))
        t = float(cfg.current_timestep_callback())
        mode = None
        if _fc(cfg, "unconditional_batch_skip_range") is not None and not bool(_fc(cfg, "is_guidance_distilled")):
            if contexts is not None and names == FASTER_CONTEXTS:
                mode = "batched"
            elif contexts is None and b == 1 and names[0] in FASTER_CONTEXTS:
                mode = names[0]
        key = (tuple(shape), dtype, str(device), b if contexts is None else 1)
        plan = SimpleNamespace(t=t, mode=mode, skip=False, entries=[], cfg=cfg)
        for name in names:
            st = self._cache_state(name, key, lambda: dict(
                ran_prev=False, n=0, buffers={},                              # the self-attention planes
                out=None, out_i=-1,                                           # this context's last prediction, by reference
                d_low=None, d_high=None, has_delta=False, a_low=1.0, a_high=1.0))     # ("uncond": the delta and its weights)
            i = st.steps
            stack = True
            if name == "uncond" and mode in ("batched", "uncond"):
                stack = not fastercache_uncond_decide(i, t, st.has_delta, cfg)
                plan.skip = not stack
            compute = stack and bool(fastercache_attention_decide(i, t, st.n, st.ran_prev, cfg))
            self.cache_log.append((name, i, t, stack, compute))
            st.steps += 1
            plan.entries.append(SimpleNamespace(name=name, state=st, i=i, stack=stack, compute=compute))
            st.ran_prev = stack
        return plan

    def _faster_attention_plan(self, faster, b, n, d, dtype, device):
        """the self-attention decisions of the forward as a `_TaylorPlan`, for the contexts whose stack runs: only the "self"
        kind is hooked, a computing segment updates two planes with delta 1, a skipping one predicts with the coefficients
        [1, w] (`_faster_weight`); None when the self-attention is not hooked"""
        if not self._faster_attention:
            return None
        entries = [e for e in faster.entries if e.stack]
        joint = len(entries) == 1 and b > 1                      # a batch under one context: one segment for all rows
        plan = _TaylorPlan({"self": True, "cross": False}, d, dtype, device, taylor=faster.cfg, planes=2, factor_dtype=dtype,
                           weight=self._faster_weight)
        for j, e in enumerate(entries):
            st = e.state
            r0, r1 = (0, b * n) if joint else (j * n, (j + 1) * n)
            n_new = min(st.n + 1, 2) if e.compute else st.n
            plan.segs.append(SimpleNamespace(name=e.name, r0=r0, r1=r1, state=st, compute={"self": e.compute, "cross": True},
                                             s=e.i, k=1, n_old=st.n, n_new=n_new))
            if e.compute:
                st.n = n_new
        return plan

    def _faster_weight(self, module):
        cb = _fc(self._step_cache_config, "attention_weight_callback")
        return 0.5 if cb is None else float(cb(module))

    def _faster_pair(self, entry, out):
        """a context of the ("cond", "uncond") pair ran its stack at forward i and returned `out` [C, F, H, W] (kept by
        reference): once both have, the delta of that step is taken (ops.fastercache_delta) and the weights start at 1"""
        st = entry.state
        st.out, st.out_i = out, entry.i
        if not self._faster_defer_delta:
            self._faster_delta_now()

    @contextlib.contextmanager
    def _cfg_two_streams(self, main, streams):
        """One denoising step's CFG branches on two side streams: fork them off `main` at entry, join them at exit.  Under
        FasterCache the delta of the step reads both predictions: it is deferred while the branches run and taken here, after
        `main` waits for both."""
        for s in streams:
            s.wait_stream(main)
        self._faster_defer_delta = self._faster_on
        try:
            yield
        finally:
            self._faster_defer_delta = False
        for s in streams:
            main.wait_stream(s)
        if self._faster_on:
            self._faster_delta_now()

    def _faster_delta_now(self):
        states = self._step_cache_states or {}
        c, u = states.get("cond"), states.get("uncond")
        if c is None or u is None or c.out is None or u.out is None or c.out_i != u.out_i or getattr(u, "delta_i", -1) == u.out_i:
            return
        if c.out.shape != u.out.shape:
            return
        planes = c.out.numel() // max(c.out.shape[-1] * c.out.shape[-2], 1)
        if not self.ops.fastercache_supported(planes, c.out.shape[-2], c.out.shape[-1]):
            raise NotImplementedError(f"FasterCache: the low-pass kernel takes planes of at most 16384 elements, the model's "
                                      f"prediction has {tuple(c.out.shape[-2:])} ones (unconditional_batch_skip_range=None "
                                      f"keeps the unconditional branch on every step)")
        if u.d_low is None or u.d_low.shape != u.out.shape:
            u.d_low = torch.empty(u.out.shape, dtype=torch.float32, device=u.out.device)
            u.d_high = torch.empty_like(u.d_low)
        self.ops.fastercache_delta(u.out, c.out, u.d_low, u.d_high)
        u.has_delta, u.a_low, u.a_high, u.delta_i = True, 1.0, 1.0, u.out_i
        u.out = None                              # (only the conditional prediction is needed again)

    def _faster_rebuild(self, plan, cond_out, out=None):
        """u' of a skipping step from this step's conditional prediction: the weights move on, one apply launch"""
        u = self._step_cache_states["uncond"]
        u.a_low, u.a_high = fastercache_weights(plan.t, u.a_low, u.a_high, plan.cfg, self)
        return self.ops.fastercache_apply(cond_out, u.d_low, u.d_high, u.a_low, u.a_high, out=out)


    # ---------------------------------------------------------------- MagCache
    def _magcache_begin(self, b, n, d, dtype, device, contexts=None):
        """The decisions of one forward under MagCache, taken before anything is launched: None when it is off, else a plan
        with `.calibrate` and `.segs` = one entry per row segment with `.name`, `.r0`, `.r1`, `.state`, `.s` (this forward's
        number), `.compute` and `.had_residual` (whether an earlier forward of the context left a residual).  Reads the step
        counter and the context's curve alone.  Advances every context's counter and accumulators and appends
        `(context, s, computed, acc_err, acc_steps)` -- the accumulators after the decision; `(context, s, True, None, None)`
        in calibrate mode -- to `cache_log`.  A context whose rows, width, dtype or device changed starts over, and so does
        one whose counter has reached `num_inference_steps`."""
        if not self._mag_on:
            return None
        cfg = self._step_cache_config
        segs = self._context_segments(b, n, contexts)
        curves = [magcache_curve(cfg, name) for name, _, _ in segs]        # (an unnamed context raises before anything counts)
        steps, calibrate = int(_mc(cfg, "num_inference_steps")), bool(_mc(cfg, "calibrate"))
        plan = SimpleNamespace(segs=[], calibrate=calibrate, steps=steps, d=d, dtype=dtype, device=device)
        for (name, r0, r1), ratios in zip(segs, curves):
            fresh = lambda: dict(acc=MAG_FRESH, residual=None, stats=None)          # noqa: E731
            st = self._cache_state(name, (r1 - r0, d, dtype, str(device)), fresh)
            if st.steps >= steps:
                self._magcache_start_over(name)
                st = self._cache_state(name, (r1 - r0, d, dtype, str(device)), fresh)
            s, had = st.steps, st.acc[3]
            compute, st.acc = magcache_decide(s, st.acc, cfg, ratios)
            self.cache_log.append((name, s, True, None, None) if calibrate else (name, s, compute, st.acc[2], st.acc[1]))
            st.steps += 1
            plan.segs.append(SimpleNamespace(name=name, r0=r0, r1=r1, state=st, s=s, compute=compute, had_residual=had))
        return plan

    def _magcache_finish(self, plan, x, x_in):
        """after the last block (or right after the embedding when every segment skips), x_in = the stack's input [rows, D]:
        a computing segment stores the stack's residual T(x - x_in) -- in calibrate mode with the one launch that also measures
        it against the previous one (ops.magcache_calibrate, into row s of the context's [N, 2] fp64 device buffer; nothing is
        read here) --, a skipping one takes T(x_in + r) as the stack's output, its residual untouched.  A context whose counter
        has reached `num_inference_steps` starts over."""
        o = self.ops
        for seg in plan.segs:
            st, r0, r1 = seg.state, seg.r0, seg.r1
            if seg.compute:
                if st.residual is None:
                    st.residual = torch.empty((r1 - r0, plan.d), dtype=plan.dtype, device=plan.device)
                if plan.calibrate and st.stats is None:          # row s = (ratio, cos_dist); a context's first step: (1, 0)
                    st.stats = torch.zeros((plan.steps, 2), dtype=torch.float64, device=plan.device)
                    st.stats[:, 0] = 1.0
                if plan.calibrate and seg.had_residual:
                    o.magcache_calibrate(x[r0:r1], x_in[r0:r1], st.residual, st.residual, st.stats[seg.s])
                else:
                    o.step_cache_residual(x[r0:r1], x_in[r0:r1], out=st.residual, subtract=True)
            else:
                if st.residual is None:
                    raise KeyError(f"MagCache: no residual under context {seg.name!r}")
                o.step_cache_residual(st.residual, x_in[r0:r1], out=x[r0:r1], subtract=False)
            if st.steps >= plan.steps and self._step_cache_states.get(seg.name) is st:
                self._magcache_start_over(seg.name)

    def _magcache_start_over(self, name):
        """context `name` has run its `num_inference_steps` forwards: counter 0, accumulators reset, residual dropped; a
        calibrating context files its curve first"""
        st = self._step_cache_states.pop(name, None)
        if st is not None:
            self._magcache_file(name, st)

    def _magcache_file(self, name, st):
        """`magcache_calibration[name]` from the rows a calibrating context has recorded: the ONE host read of a calibrating
        call (per context), when the context starts over or the state is reset"""
        stats = getattr(st, "stats", None)
        if stats is None or st.steps < 1:
            return
        rows = stats[:st.steps].tolist()
        self.magcache_calibration = dict(self.magcache_calibration or {})
        self.magcache_calibration[name] = {"mag_ratios": [r[0] for r in rows], "cos_dist": [r[1] for r in rows]}

    # ---------------------------------------------------------------- TeaCache
    def _teacache_begin(self, b, n, d, dtype, device, contexts=None):
        """One forward under TeaCache, before anything is launched: None when it is off, else a plan with `.calibrate` and
        `.segs` = one entry per row segment with `.name`, `.r0`, `.r1`, `.state`, `.s` (this forward's number),
        `.unconditional` (it computes whatever the probe measures: `teacache_unconditional`) and `.compute` -- None here: the
        decision needs the embedding (`_teacache_probe`).  Advances every context's counter.  A context whose rows, width,
        dtype or device changed starts over, and so does one whose counter has reached `num_inference_steps`."""
        if not self._tea_on:
            return None
        cfg = self._step_cache_config
        segs = self._context_segments(b, n, contexts)
        for name, _, _ in segs:                 # (an unnamed context raises before anything counts)
            teacache_coefficients(cfg, name)
        steps, calibrate = int(_tc(cfg, "num_inference_steps")), bool(_tc(cfg, "calibrate"))
        plan = SimpleNamespace(segs=[], calibrate=calibrate, steps=steps, d=d, dtype=dtype, device=device)
        for name, r0, r1 in segs:
            fresh = lambda: dict(acc=TEA_FRESH, plane=None, residual=None, tea_stats=None, out_plane=None)      # noqa: E731
            st = self._cache_state(name, (r1 - r0, d, dtype, str(device)), fresh)
            if st.steps >= steps:
                self._teacache_start_over(name)
                st = self._cache_state(name, (r1 - r0, d, dtype, str(device)), fresh)
            s = st.steps
            st.steps += 1
            plan.segs.append(SimpleNamespace(name=name, r0=r0, r1=r1, state=st, s=s, compute=None,
                                             unconditional=teacache_unconditional(s, st.acc, cfg)))
        return plan

    def _teacache_probe(self, plan, h0, shift, scale, sel, eps):
        """after the embedding, h0 = the stack's input [rows, D]; shift / scale / sel / eps: block 0's `norm1` modulation as
        `ops.adaln_modulate` takes it.  One probe launch per segment (ops.teacache_probe) leaves the modulated input in the
        context's plane and the two sums of its distance to the previous one on the device; ONE host read covers every
        segment of the call -- none when every segment computes unconditionally --, then `teacache_decide` per segment and
        `(context, s, computed, d, acc)` to `cache_log`.  In calibrate mode the sums go straight into row s of the context's
        [N, 4] fp64 device buffer and nothing is read."""
        o, cfg = self.ops, self._step_cache_config
        sums = torch.empty((len(plan.segs), 2), dtype=torch.float64, device=plan.device)      # (every launch writes its row)
        for i, seg in enumerate(plan.segs):
            st, r0, r1 = seg.state, seg.r0, seg.r1
            had = st.plane is not None
            if not had:
                st.plane = torch.empty((r1 - r0, plan.d), dtype=plan.dtype, device=plan.device)
            stats = sums[i]
            if plan.calibrate:              # row s = (sum |m - p|, sum |p|, the same two over the head's rows); step 0: zeros
                if st.tea_stats is None:
                    st.tea_stats = torch.zeros((plan.steps, 4), dtype=torch.float64, device=plan.device)
                stats = st.tea_stats[seg.s, 0:2]
            o.teacache_probe(h0[r0:r1], st.plane, stats, shift, scale, None if sel is None else sel[r0:r1], eps,
                             compare=had and (plan.calibrate or not seg.unconditional))
        host = None if all(seg.unconditional for seg in plan.segs) else sums.tolist()        # the host read
        for i, seg in enumerate(plan.segs):
            st, dist = seg.state, None
            if not seg.unconditional:
                sa, sq = host[i]
                dist = sa / sq if sq else (float("inf") if sa else float("nan"))
            seg.compute, st.acc = teacache_decide(seg.s, st.acc, cfg, dist, seg.name)
            self.cache_log.append((seg.name, seg.s, seg.compute, dist, st.acc[0]))

    def _teacache_finish(self, plan, x, x_in):
        """after the last block (or right after the probe when every segment skips), x_in = the stack's input [rows, D]: a
        computing segment stores the stack's residual T(x - x_in), a skipping one takes T(x_in + r) as the stack's output, its
        residual untouched"""
        o = self.ops
        for seg in plan.segs:
            st, r0, r1 = seg.state, seg.r0, seg.r1
            if seg.compute:
                if st.residual is None:
                    st.residual = torch.empty((r1 - r0, plan.d), dtype=plan.dtype, device=plan.device)
                o.step_cache_residual(x[r0:r1], x_in[r0:r1], out=st.residual, subtract=True)
            else:
                if st.residual is None:
                    raise KeyError(f"TeaCache: no residual under context {seg.name!r}")
                o.step_cache_residual(st.residual, x_in[r0:r1], out=x[r0:r1], subtract=False)

    def _teacache_head(self, plan, po):
        """after the output head, po = its rows [rows, C_out * prod(patch)]: a calibrating run measures them against the previous
        forward's (the probe's plain mode, into columns 2 and 3 of row s; nothing is read here).  A context whose counter has
        reached `num_inference_steps` starts over."""
        for seg in plan.segs:
            st = seg.state
            if plan.calibrate:
                had = st.out_plane is not None
                if not had:
                    st.out_plane = torch.empty((seg.r1 - seg.r0, po.shape[1]), dtype=po.dtype, device=po.device)
                self.ops.teacache_probe(po[seg.r0:seg.r1], st.out_plane, st.tea_stats[seg.s, 2:4], compare=had)
            if st.steps >= plan.steps and self._step_cache_states.get(seg.name) is st:
                self._teacache_start_over(seg.name)

    def _teacache_start_over(self, name):
        """context `name` has run its `num_inference_steps` forwards: counter 0, accumulator reset, plane and residual dropped;
        a calibrating context files its measurements first"""
        st = self._step_cache_states.pop(name, None)
        if st is not None:
            self._teacache_file(name, st)

    def _teacache_file(self, name, st):
        """`teacache_calibration[name]` from the rows a calibrating context has recorded: the ONE host read of a calibrating
        call (per context), when the context starts over or the state is reset.  Entry s is the relative L1 distance of forward
        s to forward s - 1, of the modulated input and of the head's output rows; None where nothing was compared (s = 0)."""
        stats = getattr(st, "tea_stats", None)
        if stats is None or st.steps < 1:
            return
        rows = stats[:st.steps].tolist()
        quot = lambda a, q: a / q if q else None        # noqa: E731
        self.teacache_calibration = dict(self.teacache_calibration or {})
        self.teacache_calibration[name] = {"rel_l1_in": [quot(r[0], r[1]) for r in rows],
                                           "rel_l1_out": [quot(r[2], r[3]) for r in rows]}


    # ---------------------------------------------------------------- region-adaptive sampling
    def _ras_begin(self, b, n, d, d_out, dtype, device, contexts=None, live=None, active_rows=None):
        """The decision of one forward under region-adaptive sampling, taken before anything is launched: None when it is off,
        else a plan with `.full`, `.state` (ONE per call: filed under the context name, or under the tuple of the names of a
        batch whose elements are named), `.rows` (La of a partial forward, n of a full one), `.override` (the list a caller
        passed as `_active_rows`: that forward is partial whatever the schedule says, and the counters stay) and `.cfg`.
        `live`: the (lo, hi) rows the caller reads -- the others are not eligible.  Advances the counter and appends
        `(context, s, full, rows_run)` per context of the call to `cache_log`.  A state whose batch, rows, widths, dtype or
        device changed starts over."""
        if not self._ras_on:
            return None
        cfg = self._step_cache_config
        names = tuple(name for name, _, _ in self._context_segments(b, n, contexts))
        st = self._cache_state(names[0] if len(names) == 1 else names, (b, n, d, d_out, dtype, str(device)),
                               lambda: dict(planes=None, po=None, counters=None, score=None, idx=None, eligible=None,
                                            eligible_key=None, n_always=0, valid=False))
        lo, hi = (0, n) if live is None else live
        key = (lo, hi, id(cfg.always_active))
        if st.eligible_key != key:           # one host read per state: how many rows the mask pins
            elig = torch.zeros(n, dtype=torch.uint8, device=device)
            elig[lo:hi] = 1
            st.n_always = 0
            if cfg.always_active is not None:
                mask = cfg.always_active.to(device)
                if mask.shape[0] != n:
                    raise ValueError(f"RegionAdaptiveSamplingConfig.always_active has {mask.shape[0]} entries, the forward "
                                     f"{n} token rows")
                pinned = mask & (elig == 1)
                elig[pinned] = 2
                st.n_always = int(pinned.sum())
            st.eligible, st.eligible_key = elig, key
        la = ras_active_count(cfg.sample_ratio, hi - lo)
        if st.n_always > la:
            raise ValueError(f"RegionAdaptiveSamplingConfig.always_active pins {st.n_always} of the {hi - lo} eligible token rows, "
                             f"a partial step runs La = {la} (sample_ratio = {cfg.sample_ratio}): raise sample_ratio or shrink "
                             f"the mask")
        s = st.steps
        override = None
        if active_rows is not None:
            if not st.valid:
                raise RuntimeError("forward(_active_rows=...): a partial forward needs the K / V planes of a full forward of this "
                                   "state first")
            override = active_rows.to(device=device, dtype=torch.int32).contiguous()
            if override.dim() != 1 or not 1 <= override.shape[0] <= n:
                raise ValueError(f"_active_rows: need a list of 1 .. {n} row indices, got {tuple(override.shape)}")
            full, rows = False, int(override.shape[0])
        else:
            full = bool(ras_decide(s, cfg, st.valid))
            rows = n if full else la
        for name in names:
            self.cache_log.append((name, s, full, rows))
        st.steps += 1
        return SimpleNamespace(full=full, state=st, rows=rows, override=override, cfg=cfg, idx=None, names=names)


class PyramidAttentionBroadcastMixin(StepCacheMixin):
    """The same surface for a model that implements Pyramid Attention Broadcast alone (CogVideoXTransformer3DModel), plus
    diffusers' `cache_context(name)`: every other config is refused by name.  The model's only attention layer is each
    block's joint text + video `attn1`, the "spatial" kind; `temporal_*` and `cross_*` ranges match no layer: a config that sets
    only those is accepted, hooks nothing and says so once.  `_pab_begin` / `_pab_buffer` and the `cache_log` rows are the Wan
    model's -- the last field, the cross-attention's decision, is always True here."""
    _cache_policies = (_PabPolicy,)
    _ctx_name = None

    @contextlib.contextmanager
    def cache_context(self, name):
        prev, self._ctx_name = self._ctx_name, name
        try:
            yield
        finally:
            self._ctx_name = prev

    def enable_cache(self, config):
        super().enable_cache(config)
        if config.spatial_attention_block_skip_range is None:
            warnings.warn(f"Pyramid Attention Broadcast: `spatial_attention_block_skip_range` is None and the temporal / cross "
                          f"ranges match no attention layer of {type(self).__name__} (its only one is the joint attn1 of every "
                          f"block, the spatial kind): this config hooks nothing and every forward computes.", stacklevel=2)
