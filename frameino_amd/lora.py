"""LoRA adapters for the Wan and CogVideoX DiTs, merged into the weights on the GPU (fino_lora_merge).

The reference's transformers inherit diffusers' PeftAdapterMixin and its pipelines WanLoraLoaderMixin /
CogVideoXLoraLoaderMixin (architecture/transformer_wan.py:23-24, :463-476; pipelines/pipeline_wan_i2v_motion_FrameINO.py:26,
:134; pipelines/pipeline_cogvideox_i2v_motion_FrameINO.py:26, :166).  Here an adapter is never a runtime low-rank branch:
its factors are merged into the linear weights, so a denoise step runs the same kernels on the same buffers with or without
one.  How it works:

  * loading parses and stores the factors (host tensors); nothing merges then;
  * the merge is lazy: the next forward with the parameters on the GPU (or `fuse_lora()`) merges every active adapter at
    its current scale (call scale x adapter weight x alpha / r) in one fino_lora_merge call per weight, then calls the
    model's `reset_caches()` (fused QKV / KV, Cog's stacked `wmod`, text K/V caches, MXFP8 weights are rebuilt);
  * before its first merge a parameter's base value is copied to a non-persistent buffer (it follows `.to()`, stays out
    of `state_dict()`); every merge starts from that copy, so unloading / disabling restores the base bits exactly and a
    new scale never accumulates rounding;
  * while a merge is active `state_dict()` returns the MERGED weights.

Key layouts accepted: diffusers / PEFT (`[transformer.]<module>.lora_A.weight` / `lora_B.weight`, the PEFT folder form
`adapter_model.safetensors` + `adapter_config.json`), and for Wan the original Wan-repo / kohya layout
(`diffusion_model.blocks.N.self_attn.q.lora_down.weight` ..., `.alpha`, `.diff_b`, `.diff`).  Anything not understood is an
error that names the keys: nothing is dropped silently.
"""
import contextlib
import functools
import inspect
import json
import math
import os
import re

import torch

WEIGHT_NAMES = ("pytorch_lora_weights.safetensors", "adapter_model.safetensors")

# original Wan-repo module names -> the diffusers names of this package's WanTransformer3DModel
_WAN_BLOCK = {
    "self_attn.q": "attn1.to_q", "self_attn.k": "attn1.to_k", "self_attn.v": "attn1.to_v", "self_attn.o": "attn1.to_out.0",
    "self_attn.norm_q": "attn1.norm_q", "self_attn.norm_k": "attn1.norm_k",
    "cross_attn.q": "attn2.to_q", "cross_attn.k": "attn2.to_k", "cross_attn.v": "attn2.to_v", "cross_attn.o": "attn2.to_out.0",
    "cross_attn.norm_q": "attn2.norm_q", "cross_attn.norm_k": "attn2.norm_k",
    "ffn.0": "ffn.net.0.proj", "ffn.2": "ffn.net.2", "norm3": "norm2",
}
_WAN_TOP = {
    "head.head": "proj_out", "text_embedding.0": "condition_embedder.text_embedder.linear_1",
    "text_embedding.2": "condition_embedder.text_embedder.linear_2",
    "time_embedding.0": "condition_embedder.time_embedder.linear_1",
    "time_embedding.2": "condition_embedder.time_embedder.linear_2", "time_projection.1": "condition_embedder.time_proj",
}
_CONV_TARGETS = ("patch_embedding", "patch_embed.proj")
_SUFFIXES = (("lora_A.weight", "A"), ("lora_B.weight", "B"), ("lora_down.weight", "A"), ("lora_up.weight", "B"),
             ("alpha", "alpha"), ("diff_b", "diff_b"), ("diff", "diff"))


class LoraError(ValueError):
    """An adapter this package cannot apply exactly as given (the message names the keys)."""


# ---------------------------------------------------------------------------------------------- reading
def read_adapter(src, weight_name=None):
    """(state dict, adapter_config dict or None) from a state dict, a .safetensors / .bin file or a local folder."""
    if isinstance(src, dict):
        return dict(src), None
    path = str(src)
    config = None
    if os.path.isdir(path):
        from .loading import _local_folder
        folder = _local_folder(path)
        names = [weight_name] if weight_name else [n for n in WEIGHT_NAMES if os.path.exists(os.path.join(folder, n))]
        if not names or not os.path.exists(os.path.join(folder, names[0])):
            raise OSError(f"{folder!r} holds none of {[weight_name] if weight_name else list(WEIGHT_NAMES)}; "
                          f"pass weight_name= for another file name")
        cfg = os.path.join(folder, "adapter_config.json")
        if os.path.exists(cfg):
            with open(cfg) as f:
                config = json.load(f)
        path = os.path.join(folder, names[0])
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(path), config
    return torch.load(path, map_location="cpu", weights_only=True), config


def _check_config(config):
    if not config:
        return
    for k in ("rank_pattern", "alpha_pattern"):
        if config.get(k):
            raise LoraError(f"adapter_config.json: {k} {sorted(config[k])[:8]} is not supported (one rank / alpha per adapter)")
    if config.get("use_dora"):
        raise LoraError("adapter_config.json: use_dora = true (DoRA) is not supported")


def _split_key(key):
    for suf, kind in _SUFFIXES:
        if key.endswith("." + suf):
            return key[:-len(suf) - 1], kind
    return None, None


def _wan_module(mod):
    """original Wan-repo module path (prefix removed) -> diffusers path, or None"""
    m = re.fullmatch(r"blocks\.(\d+)\.(.+)", mod)
    if m:
        sub = _WAN_BLOCK.get(m.group(2))
        return None if sub is None else f"blocks.{m.group(1)}.{sub}"
    return _WAN_TOP.get(mod)


def parse_adapter(sd, params, prefix="transformer", config=None, wan_layout=True):
    """State dict -> (factors, diffs): factors = [(parameter name, A, B, alpha / r)], diffs = [(parameter name, delta)].
    `params`: the model's {name: parameter} (shapes checked here).  Raises LoraError naming every key it cannot place."""
    _check_config(config)
    dora = [k for k in sd if "lora_magnitude_vector" in k]
    if dora:
        raise LoraError(f"DoRA adapters are not supported: {dora[:5]}")
    groups, unknown = {}, []
    for key, t in sd.items():
        k = key
        for p in ("base_model.model.", (prefix + ".") if prefix else None, "diffusion_model.", "model.diffusion_model."):
            if p and k.startswith(p):
                k = k[len(p):]
        mod, kind = _split_key(k)
        if mod is None:
            unknown.append(key)
            continue
        target = mod
        if not _has_module(params, mod) and wan_layout:
            target = _wan_module(mod) or mod
        groups.setdefault(target, {})[kind] = (key, t)
    if unknown:
        raise LoraError(f"unknown LoRA keys (not lora_A / lora_B / lora_down / lora_up / alpha / diff / diff_b): {unknown[:8]}")
    conv = [v[next(iter(v))][0] for m, v in groups.items() if m.startswith(_CONV_TARGETS)]
    if conv:
        raise LoraError(f"LoRA on a convolution is not supported: {conv[:8]}")
    missing = [g[next(iter(g))][0] for m, g in groups.items() if not _has_module(params, m)]
    if missing:
        raise LoraError(f"LoRA keys whose target this model does not have: {missing[:8]}")
    r_cfg = config.get("r") if config else None
    a_cfg = config.get("lora_alpha") if config else None
    rslora = bool(config.get("use_rslora")) if config else False
    factors, diffs, bad = [], [], []
    for mod, g in sorted(groups.items()):
        if ("A" in g) != ("B" in g):
            bad.append(f"{(g.get('A') or g.get('B'))[0]}: its {'lora_B / lora_up' if 'A' in g else 'lora_A / lora_down'} is missing")
            continue
        if "A" in g:
            w = params.get(mod + ".weight")
            (ka, a), (kb, b) = g["A"], g["B"]
            a, b = a.reshape(a.shape[0], -1) if a.dim() > 2 else a, b.reshape(b.shape[0], -1) if b.dim() > 2 else b
            if w is None or w.dim() != 2:
                bad.append(f"{ka}: {mod} is not a linear layer")
                continue
            r = a.shape[0]
            if a.dim() != 2 or b.dim() != 2 or a.shape[1] != w.shape[1] or b.shape != (w.shape[0], r):
                bad.append(f"{ka} {tuple(a.shape)} / {kb} {tuple(b.shape)} do not fit {mod}.weight {tuple(w.shape)}")
                continue
            if r_cfg is not None and r_cfg != r:
                bad.append(f"{ka}: rank {r} but adapter_config.json says r = {r_cfg}")
                continue
            if "alpha" in g:
                alpha = float(g["alpha"][1].reshape(-1)[0])
            elif a_cfg is not None:
                alpha = float(a_cfg)
            else:
                alpha = None
            scale = 1.0 if alpha is None else (alpha / math.sqrt(r) if rslora else alpha / r)
            factors.append((mod + ".weight", a.contiguous(), b.contiguous(), scale))
        elif "alpha" in g and not ("diff" in g or "diff_b" in g):
            bad.append(f"{g['alpha'][0]}: an alpha without factors")
        for kind, pname in (("diff", mod + ".weight"), ("diff_b", mod + ".bias")):
            if kind in g:
                key, d = g[kind]
                p = params.get(pname)
                if p is None or tuple(d.shape) != tuple(p.shape):
                    bad.append(f"{key} {tuple(d.shape)} does not fit {pname} {None if p is None else tuple(p.shape)}")
                    continue
                diffs.append((pname, d.contiguous()))
    if bad:
        raise LoraError("LoRA keys that cannot be applied: " + "; ".join(bad[:8]))
    return factors, diffs


def _has_module(params, mod):
    return (mod + ".weight") in params or (mod + ".bias") in params


# ---------------------------------------------------------------------------------------------- model mixin
class LoraModelMixin:
    """PeftAdapterMixin's names on this package's transformers, adapters MERGED into the weights (module docstring)."""

    def _lora_state(self):
        st = self.__dict__.get("_lora")
        if st is None:
            st = self.__dict__["_lora"] = {"adapters": {}, "active": [], "weights": {}, "enabled": True, "call_scale": 1.0,
                                           "fused": None, "merged": None, "bases": {}, "busy": 0, "dev": {},
                                           "serial": 0}
        return st

    def _lora_mutable(self, what):
        if self._lora_state()["busy"]:
            raise RuntimeError(f"{what}: LoRA state cannot change while a denoise loop runs (its captured step graph holds "
                               f"the current weights); change it before or after the pipeline call")

    # ---- PeftAdapterMixin surface ----
    def load_lora_adapter(self, state_dict_or_path, adapter_name=None, prefix="transformer", weight_name=None, **kwargs):
        self._lora_mutable("load_lora_adapter")
        st = self._lora_state()
        sd, config = read_adapter(state_dict_or_path, weight_name)
        factors, diffs = parse_adapter(sd, dict(self.named_parameters()), prefix=prefix, config=config,
                                       wan_layout=getattr(self, "_lora_wan_layout", False))
        if not factors and not diffs:
            raise LoraError(f"no LoRA weights for this model in the adapter (prefix={prefix!r})")
        if adapter_name is None:
            i = 0
            while f"default_{i}" in st["adapters"]:
                i += 1
            adapter_name = f"default_{i}"
        if adapter_name in st["adapters"]:
            raise ValueError(f"adapter name {adapter_name!r} is already in use")
        st["serial"] += 1                   # the merge key names this load, not just the name (a re-used name re-merges)
        st["adapters"][adapter_name] = {"factors": factors, "diffs": diffs, "id": st["serial"]}
        st["active"].append(adapter_name)
        st["weights"][adapter_name] = 1.0
        return adapter_name

    def set_adapters(self, adapter_names, weights=None):
        self._lora_mutable("set_adapters")
        st = self._lora_state()
        names = [adapter_names] if isinstance(adapter_names, str) else list(adapter_names)
        unknown = [n for n in names if n not in st["adapters"]]
        if unknown:
            raise ValueError(f"unknown adapters {unknown}; loaded: {sorted(st['adapters'])}")
        if weights is None:
            weights = [1.0] * len(names)
        elif not isinstance(weights, (list, tuple)):
            weights = [weights] * len(names)
        if len(weights) != len(names):
            raise ValueError(f"{len(names)} adapter names but {len(weights)} weights")
        st["active"] = names
        st["weights"].update({n: (1.0 if w is None else float(w)) for n, w in zip(names, weights)})

    def active_adapters(self):
        return list(self._lora_state()["active"])

    def get_list_adapters(self):
        return sorted(self._lora_state()["adapters"])

    def disable_lora(self):
        self._lora_mutable("disable_lora")
        self._lora_state()["enabled"] = False

    def enable_lora(self):
        self._lora_mutable("enable_lora")
        self._lora_state()["enabled"] = True

    def delete_adapters(self, adapter_names):
        self._lora_mutable("delete_adapters")
        st = self._lora_state()
        for n in ([adapter_names] if isinstance(adapter_names, str) else list(adapter_names)):
            if n not in st["adapters"]:
                raise ValueError(f"unknown adapter {n!r}")
            del st["adapters"][n]
            st["weights"].pop(n, None)
            st["active"] = [a for a in st["active"] if a != n]
            if st["fused"] and n in st["fused"][1]:
                st["fused"] = (st["fused"][0], [a for a in st["fused"][1] if a != n])
        st["dev"].clear()
        self._lora_sync()

    def unload_lora(self):
        """Drop every adapter and restore the base parameters (bit-exact) and their buffers."""
        self._lora_mutable("unload_lora")
        st = self._lora_state()
        st["adapters"].clear()
        st["active"], st["weights"], st["fused"] = [], {}, None
        st["dev"].clear()
        self._lora_sync()
        if st["merged"] is None:
            for name in list(st["bases"]):
                mod, attr = self._lora_owner(name)
                delattr(mod, attr)
            st["bases"].clear()

    def fuse_lora(self, lora_scale=1.0, adapter_names=None):
        """Merge now and pin `lora_scale` for these adapters (default: the active ones): later call scales leave them alone."""
        self._lora_mutable("fuse_lora")
        st = self._lora_state()
        names = list(st["active"]) if adapter_names is None else \
            ([adapter_names] if isinstance(adapter_names, str) else list(adapter_names))
        unknown = [n for n in names if n not in st["adapters"]]
        if unknown:
            raise ValueError(f"unknown adapters {unknown}")
        st["fused"] = (float(lora_scale), names)
        self._lora_sync()

    def unfuse_lora(self):
        self._lora_mutable("unfuse_lora")
        self._lora_state()["fused"] = None

    # ---- merge ----
    def _lora_plan(self):
        """{parameter name: [(A, B, scale)] + diffs} for the current state, and its hashable key"""
        st = self._lora_state()
        if not st["enabled"]:
            return {}, ()
        fused = st["fused"]
        plan, key = {}, []
        for n in st["active"]:
            if fused and n in fused[1]:
                s = fused[0] * st["weights"][n]
            elif fused:
                continue                    # fused_lora(adapter_names=...) pins the listed adapters; the others are off
            else:
                s = st["call_scale"] * st["weights"][n]
            ad = st["adapters"][n]
            key.append((ad["id"], s))
            for pname, a, b, alpha_r in ad["factors"]:
                plan.setdefault(pname, []).append(("f", n, a, b, s * alpha_r))
            for pname, d in ad["diffs"]:
                plan.setdefault(pname, []).append(("d", n, d, None, s))
        return plan, tuple(key)

    def _lora_owner(self, pname):
        mod_name, _, attr = pname.rpartition(".")
        return self.get_submodule(mod_name) if mod_name else self, "_lora_base_" + attr

    def _lora_on_device(self, t, p, cache_key):
        st = self._lora_state()
        k = (cache_key, p.device, p.dtype)
        v = st["dev"].get(k)
        if v is None:
            v = st["dev"][k] = t.to(device=p.device, dtype=p.dtype).contiguous()
        return v

    def _lora_apply(self, scale):
        """the call-time scale of a forward (attention_kwargs["scale"], as diffusers' scale_lora_layers): merge if it changes
        what is merged.  Cheap when no adapter was ever loaded."""
        st = self.__dict__.get("_lora")
        if st is None or (not st["adapters"] and st["merged"] is None):
            return
        st["call_scale"] = 1.0 if scale is None else float(scale)
        self._lora_sync()

    def _lora_sync(self):
        """Bring the parameters to the current plan (fino_lora_merge from the base copies).  A no-op when they already are,
        or while they are not on the GPU (the next forward on the device merges)."""
        from . import ops
        st = self._lora_state()
        plan, key = self._lora_plan()
        if key == (st["merged"] or ()):
            return False
        params = dict(self.named_parameters())
        if not all(p.is_cuda for p in params.values()):
            if key == () and st["bases"]:
                with torch.no_grad():            # restoring on the host is a copy, no arithmetic
                    for pname in st["bases"]:
                        mod, attr = self._lora_owner(pname)
                        params[pname].data.copy_(getattr(mod, attr))
                st["merged"] = None
                self.reset_caches()
            return False
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("a LoRA scale / adapter change reached a forward while the stream is capturing a graph: "
                               "apply it before the capture (the pipelines do so before their denoise loop)")
        with torch.no_grad():
            for pname in sorted(set(plan) | set(st["bases"])):
                p = params[pname]
                mod, attr = self._lora_owner(pname)
                base = getattr(mod, attr, None)
                if base is None:
                    base = p.detach().clone()
                    mod.register_buffer(attr, base, persistent=False)
                    st["bases"][pname] = True
                w2 = p.data if p.dim() == 2 else p.data.view(1, -1)
                b2 = base if base.dim() == 2 else base.view(1, -1)
                terms = []
                for kind, n, x, y, s in plan.get(pname, []):
                    if kind == "f":
                        terms.append((self._lora_on_device(x, p, (n, pname, "A")), self._lora_on_device(y, p, (n, pname, "B")), s))
                    else:                        # a dense delta: one rank-1 term, B = 1 (the fp32 sum happens in the kernel)
                        a = self._lora_on_device(x.reshape(1, -1), p, (n, pname, "d"))
                        terms.append((a, torch.ones(w2.shape[0], 1, dtype=p.dtype, device=p.device), s))
                if len(terms) > ops.LORA_MAX_ADAPTERS:
                    raise LoraError(f"{pname}: {len(terms)} adapter terms at once (at most {ops.LORA_MAX_ADAPTERS})")
                ops.lora_merge_(b2, terms, out=w2)
        st["merged"] = key if key else None
        self.reset_caches()
        return True

    @contextlib.contextmanager
    def _lora_hold(self, scale):
        """the pipelines' denoise loop: apply the call scale once, then refuse any LoRA change until the loop ends"""
        self._lora_apply(scale)
        st = self._lora_state()
        st["busy"] += 1
        try:
            yield
        finally:
            st["busy"] -= 1


# ---------------------------------------------------------------------------------------------- pipeline mixin
def lora_denoise_loop(fn):
    """Decorator of a pipeline's `denoise`: the LoRA call scale (attention_kwargs["scale"]) is merged before the loop, and
    LoRA state changes during it (a `callback_on_step_end` included) raise RuntimeError."""
    sig = inspect.signature(fn)

    @functools.wraps(fn)
    def run(self, *args, **kwargs):
        tr = getattr(self, "transformer", None)
        if not isinstance(tr, LoraModelMixin):
            return fn(self, *args, **kwargs)
        ak = sig.bind(self, *args, **kwargs).arguments.get("attention_kwargs") or {}
        with tr._lora_hold(ak.get("scale")):
            return fn(self, *args, **kwargs)
    return run


class LoraPipelineMixin:
    """The diffusers LoRA loader names on this package's pipelines (WanLoraLoaderMixin / CogVideoXLoraLoaderMixin): local
    folders, files or state dicts only; the adapter goes to `self.transformer` (module docstring)."""
    transformer_name = "transformer"

    @classmethod
    def lora_state_dict(cls, pretrained_model_name_or_path_or_dict, weight_name=None, **hub_kwargs):
        from .loading import _HUB_KWARGS
        unknown = sorted(set(hub_kwargs) - set(_HUB_KWARGS))
        if unknown:
            raise TypeError(f"lora_state_dict: unexpected keyword arguments {unknown}")
        return read_adapter(pretrained_model_name_or_path_or_dict, weight_name)[0]

    def load_lora_weights(self, pretrained_model_name_or_path_or_dict, adapter_name=None, weight_name=None, **hub_kwargs):
        from .loading import _HUB_KWARGS
        unknown = sorted(set(hub_kwargs) - set(_HUB_KWARGS))
        if unknown:
            raise TypeError(f"load_lora_weights: unexpected keyword arguments {unknown}")
        return self.transformer.load_lora_adapter(pretrained_model_name_or_path_or_dict, adapter_name=adapter_name,
                                                  prefix=self.transformer_name, weight_name=weight_name)

    def set_adapters(self, adapter_names, adapter_weights=None):
        self.transformer.set_adapters(adapter_names, adapter_weights)

    def get_active_adapters(self):
        return self.transformer.active_adapters()

    def get_list_adapters(self):
        return {self.transformer_name: self.transformer.get_list_adapters()}

    def delete_adapters(self, adapter_names):
        self.transformer.delete_adapters(adapter_names)

    def disable_lora(self):
        self.transformer.disable_lora()

    def enable_lora(self):
        self.transformer.enable_lora()

    def unload_lora_weights(self):
        self.transformer.unload_lora()

    def fuse_lora(self, lora_scale=1.0, adapter_names=None, **kwargs):
        self.transformer.fuse_lora(lora_scale, adapter_names)

    def unfuse_lora(self, **kwargs):
        self.transformer.unfuse_lora()
