"""Step caching of the Wan DiT: diffusers' `CacheMixin` (diffusers/models/cache_utils.py), which the reference's
WanTransformer3DModel inherits (architecture/transformer_wan.py:28, :353) and whose state its FrameINO loop keys by
`cache_context("cond")` / `("uncond")` (pipelines/pipeline_wan_i2v_motion_FrameINO.py:862, :873), with two of its configs:
`FirstBlockCacheConfig` (diffusers/hooks/first_block_cache.py) and `PyramidAttentionBroadcastConfig`
(diffusers/hooks/pyramid_attention_broadcast.py).  One at a time: a second `enable_cache` raises, as in diffusers.

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

The CogVideoX DiT (`PyramidAttentionBroadcastMixin`) takes Pyramid Attention Broadcast alone, with the same rule and state: its one
attention layer per block, the joint text + video attn1, is the "spatial" kind, and a call's whole batch is one segment under one
context (diffusers' CogVideoX pipelines run the CFG batch under `cache_context("cond_uncond")`).
"""
import contextlib
import dataclasses
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


# the other configs diffusers' CacheMixin applies: recognised, not implemented here
_OTHER_DIFFUSERS_CONFIGS = ("FasterCacheConfig", "TaylorSeerCacheConfig", "MagCacheConfig", "TeaCacheConfig")

_PAB_NAME = "PyramidAttentionBroadcastConfig"
_PAB_RANGES = ("spatial_attention_block_skip_range", "temporal_attention_block_skip_range", "cross_attention_block_skip_range")
# the attention kinds of the Wan DiT: (key, block-skip field, timestep-range field)
PAB_KINDS = (("self", "spatial_attention_block_skip_range", "spatial_attention_timestep_skip_range"),
             ("cross", "cross_attention_block_skip_range", "cross_attention_timestep_skip_range"))


def _is_fbc_config(config):
    return type(config).__name__ == "FirstBlockCacheConfig" and hasattr(config, "threshold")


def _is_pab_config(config):
    return type(config).__name__ == _PAB_NAME and all(hasattr(config, a) for a in _PAB_RANGES + ("current_timestep_callback",))


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


class FirstBlockCacheMixin:
    """diffusers' CacheMixin surface (enable_cache / disable_cache / is_cache_enabled / _reset_stateful_cache) for
    FirstBlockCache and Pyramid Attention Broadcast.  For the first the model calls `_step_cache_segments`, `_step_cache_probe`
    and `_step_cache_finish` from its forward; for the second `_pab_begin` (once per forward) and `_pab_buffer`.

    State per cache-context name: the head residual (plus a spare buffer the next probe writes into), the tail residual, and a
    step counter.  `cache_log` holds `(context, step, diff, computed)` for every forward since the last reset (diff None: no
    previous residual); it survives the reset at the end of a pipeline call, so the call's decisions can be read after it.

    Pyramid Attention Broadcast: per context and kind a counter, per (kind, layer) a [rows, D] buffer in the model dtype,
    allocated by the first forward that computes; `cache_log` holds `(context, iteration, float(timestep),
    self_attention_computed, cross_attention_computed)` for every forward and context, with the same lifetime."""
    _cache_configs_implemented = "FirstBlockCacheConfig and PyramidAttentionBroadcastConfig are"
    _step_cache_config = None
    _step_cache_states = None
    _step_cache_log_fresh = True
    cache_log = ()

    @property
    def is_cache_enabled(self):
        return self._step_cache_config is not None

    def enable_cache(self, config):
        if self.is_cache_enabled:
            raise ValueError(f"Caching has already been enabled with {type(self._step_cache_config)}. To apply a new caching "
                             f"technique, please disable the existing one first.")
        name = type(config).__name__
        if _is_fbc_config(config):
            if len(self.blocks) < 2:
                raise ValueError(f"FirstBlockCache needs a head block and at least one more block; this model has "
                                 f"{len(self.blocks)} block(s), so the head block would also be the tail block")
            self._step_cache_config = config
            self._reset_stateful_cache()
            return
        if _is_pab_config(config):
            if config.current_timestep_callback is None:
                raise ValueError("The `current_timestep_callback` function must be provided in the configuration to apply "
                                 "Pyramid Attention Broadcast: it returns the denoising loop's current timestep "
                                 "(`lambda: pipe.current_timestep`).")
            if all(getattr(config, a) is None for a in _PAB_RANGES):
                warnings.warn("Pyramid Attention Broadcast requires one or more of `spatial_attention_block_skip_range`, "
                              "`temporal_attention_block_skip_range` or `cross_attention_block_skip_range` to be set; "
                              "defaulting to `spatial_attention_block_skip_range=2`.", stacklevel=2)
                config.spatial_attention_block_skip_range = 2
            self._step_cache_config = config
            self._reset_stateful_cache()
            return
        if name == _PAB_NAME:
            raise NotImplementedError(f"{name}: this object carries the name but not the `*_block_skip_range` and "
                                      f"`current_timestep_callback` attributes of diffusers' config, so it cannot be applied")
        if name in _OTHER_DIFFUSERS_CONFIGS or (name.endswith("CacheConfig") and
                                                 type(config).__module__.split(".")[0] == "diffusers"):
            raise NotImplementedError(f"{name} is not implemented on this model; {self._cache_configs_implemented}")
        raise ValueError(f"Cache config {type(config)} is not supported.")

    def disable_cache(self):
        if self._step_cache_config is None:
            warnings.warn("Caching techniques have not been enabled, so there's nothing to disable.", stacklevel=2)
            return
        self._step_cache_config = None
        self._reset_stateful_cache()

    def _reset_stateful_cache(self, recurse=True):
        """drop every context's state (diffusers' maybe_free_model_hooks calls this at the end of a pipeline call); the next
        forward starts a new `cache_log`"""
        self._step_cache_states = {}
        self._step_cache_log_fresh = True

    # ---------------------------------------------------------------- used by the forward
    def _step_cache_segments(self, b, n, contexts=None):
        """None when no cache is enabled, else [(context, first row, end row)] of the call's [b * n, D] rows: one segment per
        batch element when `contexts` names one context each (the pipeline's CFG-batched call), else one joint segment under
        the current `cache_context`."""
        if self._step_cache_config is None or self._pab_on:
            return None                       # (Pyramid Attention Broadcast: the first-block code stays inert)
        return self._context_segments(b, n, contexts)

    def _context_segments(self, b, n, contexts):
        if contexts is not None:
            contexts = tuple(contexts)
            if len(contexts) != b or len(set(contexts)) != b:
                raise ValueError(f"_cache_contexts {contexts}: need {b} distinct names, one per batch element")
            return [(c, i * n, (i + 1) * n) for i, c in enumerate(contexts)]
        if self._ctx_name is None:
            raise ValueError("No context is set. Please set a context before retrieving the state.")
        return [(self._ctx_name, 0, b * n)]

    def _step_cache_probe(self, segs, h0, h1, h1_copy):
        """after block 0: probe, one host read, decide.  Returns one bool per segment (True: compute blocks 1 .. N-1)."""
        if self._step_cache_log_fresh or not isinstance(self.cache_log, list):
            self.cache_log = []
            self._step_cache_log_fresh = False
        if self._step_cache_states is None:
            self._step_cache_states = {}
        d, dt, dev = h1.shape[1], h1.dtype, h1.device
        sts = []
        for name, r0, r1 in segs:
            key = (r1 - r0, d, dt, str(dev))
            st = self._step_cache_states.get(name)
            if st is None or st.key != key:          # first use, or another shape / dtype / device: start over
                st = self._step_cache_states[name] = SimpleNamespace(key=key, head=None, spare=None, tail=None, steps=0)
            if st.spare is None:
                st.spare = torch.empty((r1 - r0, d), dtype=dt, device=dev)
            sts.append(st)
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
    @property
    def _pab_on(self):
        return self._step_cache_config is not None and _is_pab_config(self._step_cache_config)

    def _pab_begin(self, b, n, d, dtype, device, contexts=None):
        """The decisions of one forward, taken before anything is launched: None when Pyramid Attention Broadcast is off, else
        `.segs` = one entry per row segment (`_step_cache_segments`' segments) with `.name`, `.r0`, `.r1`, `.state` and
        `.compute[kind]`, and `.hooked[kind]`.  Reads the timestep callback ONCE (a device tensor costs its one host read here,
        not one per layer), advances every hooked kind's counter and appends to `cache_log`.  A context whose rows, width,
        dtype or device changed starts over (the model switches `live_rows` off under this cache, so there is no live-row
        range to key on)."""
        if not self._pab_on:
            return None
        cfg = self._step_cache_config
        segs = self._context_segments(b, n, contexts)
        t = float(cfg.current_timestep_callback())
        if self._step_cache_log_fresh or not isinstance(self.cache_log, list):
            self.cache_log = []
            self._step_cache_log_fresh = False
        if self._step_cache_states is None:
            self._step_cache_states = {}
        hooked = {kind: getattr(cfg, rng) is not None for kind, rng, _ in PAB_KINDS}
        plan = SimpleNamespace(segs=[], hooked=hooked, timestep=t)
        for name, r0, r1 in segs:
            key = (r1 - r0, d, dtype, str(device))
            st = self._step_cache_states.get(name)
            if st is None or st.key != key:
                st = self._step_cache_states[name] = SimpleNamespace(key=key, steps=0, iteration={k: 0 for k in hooked},
                                                                     buffers={})
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

    @staticmethod
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


class PyramidAttentionBroadcastMixin(FirstBlockCacheMixin):
    """The same surface for a model that implements Pyramid Attention Broadcast alone (CogVideoXTransformer3DModel), plus
    diffusers' `cache_context(name)`.  `FirstBlockCacheConfig` is refused by name.  The model's only attention layer is each
    block's joint text + video `attn1`, the "spatial" kind; `temporal_*` and `cross_*` ranges match no layer: a config that sets
    only those is accepted, hooks nothing and says so once.  `_pab_begin` / `_pab_buffer` and the `cache_log` rows are the Wan
    model's -- the last field, the cross-attention's decision, is always True here."""
    _cache_configs_implemented = "PyramidAttentionBroadcastConfig is"
    _ctx_name = None

    @contextlib.contextmanager
    def cache_context(self, name):
        prev, self._ctx_name = self._ctx_name, name
        try:
            yield
        finally:
            self._ctx_name = prev

    def enable_cache(self, config):
        if not self.is_cache_enabled and _is_fbc_config(config):
            raise NotImplementedError(f"FirstBlockCacheConfig is not implemented on {type(self).__name__}; "
                                      f"{self._cache_configs_implemented}")
        super().enable_cache(config)
        if self._pab_on and config.spatial_attention_block_skip_range is None:
            warnings.warn(f"Pyramid Attention Broadcast: `spatial_attention_block_skip_range` is None and the temporal / cross "
                          f"ranges match no attention layer of {type(self).__name__} (its only one is the joint attn1 of every "
                          f"block, the spatial kind): this config hooks nothing and every forward computes.", stacklevel=2)
