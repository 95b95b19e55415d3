"""First-block caching of the Wan DiT: diffusers' `CacheMixin` with `FirstBlockCacheConfig`
(diffusers/hooks/first_block_cache.py, diffusers/models/cache_utils.py), which the reference's WanTransformer3DModel inherits
(architecture/transformer_wan.py:28, :353) and which its FrameINO loop keys by `cache_context("cond")` / `("uncond")`
(pipelines/pipeline_wan_i2v_motion_FrameINO.py:862, :873).

The rule, per forward under context c (T = the model dtype; h0 = input of block 0, h1 = its output, hN = the last block's):

    r = T(h1 - h0)
    compute  if  head_residual is None  or  diff > threshold,   diff = float(T(T(mean|T(r - p)|) / T(mean|p|))),  p = head_residual
    compute: head_residual = r, blocks 1 .. N-1 run, tail_residual = T(hN - h1)
    skip:    head_residual unchanged, blocks 1 .. N-1 do not run, the stack's output is T(tail_residual + h1)

The output head runs in both cases.  The means cover every element of the call's [B, L, D] rows under that context (a direct
batch-B call makes one joint decision).  On the GPU one probe kernel (ops.step_cache_probe) writes r and the two fp32 sums;
the host reads them -- the one host sync of the rule, where diffusers calls `.item()` -- and rounds as torch does (`decide`).
"""
import dataclasses
import warnings
from types import SimpleNamespace

import torch


@dataclasses.dataclass
class FirstBlockCacheConfig:
    """diffusers.FirstBlockCacheConfig: blocks 1 .. N-1 are skipped while the relative L1 change of the first block's residual
    stays at or below `threshold`."""
    threshold: float = 0.05


# the other configs diffusers' CacheMixin applies: recognised, not implemented here
_OTHER_DIFFUSERS_CONFIGS = ("PyramidAttentionBroadcastConfig", "FasterCacheConfig", "TaylorSeerCacheConfig", "MagCacheConfig",
                            "TeaCacheConfig")


def _is_fbc_config(config):
    return type(config).__name__ == "FirstBlockCacheConfig" and hasattr(config, "threshold")


def decide(sum_abs_diff, sum_abs_prev, numel, dtype, threshold):
    """(diff, compute) from the probe's fp32 sums, rounded as torch rounds `(r - p).abs().mean() / p.abs().mean()` in `dtype`:
    each mean T(S / N) (fp32 division, one rounding to T), their quotient in T, then a Python float comparison -- NaN skips,
    inf computes."""
    a = (torch.tensor(float(sum_abs_diff), dtype=torch.float32) / numel).to(dtype)
    q = (torch.tensor(float(sum_abs_prev), dtype=torch.float32) / numel).to(dtype)
    diff = float(a / q)
    return diff, diff > threshold


class FirstBlockCacheMixin:
    """diffusers' CacheMixin surface (enable_cache / disable_cache / is_cache_enabled / _reset_stateful_cache), FirstBlockCache
    only.  The model calls `_step_cache_segments`, `_step_cache_probe` and `_step_cache_finish` from its forward.

    State per cache-context name: the head residual (plus a spare buffer the next probe writes into), the tail residual, and a
    step counter.  `cache_log` holds `(context, step, diff, computed)` for every forward since the last reset (diff None: no
    previous residual); it survives the reset at the end of a pipeline call, so the call's decisions can be read after it."""
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
        if name in _OTHER_DIFFUSERS_CONFIGS or (name.endswith("CacheConfig") and
                                                 type(config).__module__.split(".")[0] == "diffusers"):
            raise NotImplementedError(f"{name} is not implemented on this model; FirstBlockCacheConfig is")
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
        if self._step_cache_config is None:
            return None
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
