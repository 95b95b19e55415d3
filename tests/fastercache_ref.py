"""FasterCache restated for the tests: the radial low-pass by torch.fft (fp64 and fp32), the three decision / weight functions
re-derived from the rule (not imported from frameino_amd.step_cache), CPU stand-ins for ops.fastercache_delta / _apply, and a
driver that runs the unconditional-branch rule over a model callable."""
import numpy as np
import torch


# ---------------------------------------------------------------- the low-pass
def lowpass_mask(h, w):
    """the kept bins of the CENTRED spectrum: (xx - W//2)^2 + (yy - H//2)^2 <= r^2, r = min(H, W) // 5"""
    r = min(h, w) // 5
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    return ((xx - w // 2) ** 2 + (yy - h // 2) ** 2) <= r * r


def lowpass(x, dtype=torch.float64):
    """LP of every [H, W] plane of x: ifft2(ifftshift(fftshift(fft2(x)) * mask)).real, computed in `dtype` (fp64 / fp32)"""
    h, w = x.shape[-2:]
    xf = torch.fft.fftshift(torch.fft.fft2(x.to(dtype)), dim=(-2, -1))
    xf = xf * lowpass_mask(h, w).to(x.device)
    return torch.fft.ifft2(torch.fft.ifftshift(xf, dim=(-2, -1))).real


def bin_count(h, w):
    return int(lowpass_mask(h, w).sum())


def delta_ref(u, c, dtype=torch.float64):
    """(D, DL) with D = float(u) - float(c) (one fp32 subtraction) and DL = LP(D) computed in `dtype`"""
    d = u.float() - c.float()
    return d, lowpass(d, dtype)


def delta_cpu(u, c):
    """CPU stand-in of ops.fastercache_delta: (DL, DH) fp32 with the fp32 torch.fft low-pass"""
    d, dl = delta_ref(u, c, torch.float32)
    dl = dl.float()
    return dl, d - dl


def apply_ref(c, d_low, d_high, a_low, a_high):
    """T((float(c) + aL * DL) + aH * DH): every operation one fp32 operation (torch's fp32 tensor ops do not contract)"""
    al = torch.tensor(float(a_low), dtype=torch.float32, device=c.device)
    ah = torch.tensor(float(a_high), dtype=torch.float32, device=c.device)
    t0 = d_low.reshape(c.shape) * al
    t1 = d_high.reshape(c.shape) * ah
    return ((c.float() + t0) + t1).to(c.dtype)


def f32(x):
    return float(np.float32(x))


# ---------------------------------------------------------------- the rule, re-derived
def _inside(t, rng):
    return rng[0] < t < rng[1]


def uncond_skips(i, t, has_delta, cfg):
    n = cfg.unconditional_batch_skip_range
    if n is None or cfg.is_guidance_distilled or not has_delta or i <= 0:
        return False
    return _inside(t, cfg.unconditional_batch_timestep_skip_range) and i % n != 0


def weights(t, a_low, a_high, cfg, model=None):
    if cfg.low_frequency_weight_callback is not None:
        wl = cfg.low_frequency_weight_callback(model)
    else:
        wl = cfg.alpha_low_frequency if _inside(t, cfg.low_frequency_weight_update_timestep_range) else 1.0
    if cfg.high_frequency_weight_callback is not None:
        wh = cfg.high_frequency_weight_callback(model)
    else:
        wh = cfg.alpha_high_frequency if _inside(t, cfg.high_frequency_weight_update_timestep_range) else 1.0
    return f32(np.float32(a_low) * np.float32(wl)), f32(np.float32(a_high) * np.float32(wh))


def attention_computes(i, t, n_planes, ran_prev, cfg):
    n = cfg.spatial_attention_block_skip_range
    if n is None or n_planes == 0 or not ran_prev:
        return True
    return (not _inside(t, cfg.spatial_attention_timestep_skip_range)) or i % n == 0


def uncond_pattern(timesteps, cfg):
    """[stack_ran of the "uncond" context] over a call's steps, from fresh state"""
    out, has = [], False
    for i, t in enumerate(timesteps):
        skip = uncond_skips(i, float(t), has, cfg)
        out.append(not skip)
        has = has or not skip
    return out


def drive(model, inputs, timesteps, cfg, delta=delta_cpu, apply=apply_ref):
    """The unconditional-branch rule over `model(context, x) -> prediction [C, F, H, W]`: per step (cond, uncond) as the
    cached model must return them, plus the log rows (context, i, t, stack_ran)."""
    outs, log = [], []
    dl = dh = None
    al = ah = f32(1.0)
    for i, (x, t) in enumerate(zip(inputs, timesteps)):
        t = float(t)
        c = model("cond", x)
        log.append(("cond", i, t, True))
        if uncond_skips(i, t, dl is not None, cfg):
            al, ah = weights(t, al, ah, cfg)
            u = apply(c, dl, dh, al, ah)
            log.append(("uncond", i, t, False))
        else:
            u = model("uncond", x)
            dl, dh = delta(u, c)
            al = ah = f32(1.0)
            log.append(("uncond", i, t, True))
        outs.append((c, u))
    return outs, log


# ---------------------------------------------------------------- the self-attention part on the oracle's pieces
def attention_ref(sd, cfg, config):
    """`ref(context, hidden_states, timestep, text)`: the Wan DiT forward recomposed from oracle.wan_dit pieces (as
    tests/taylorseer_ref.py does) with every block's attn1 output computed or extrapolated by the rule of `config`; attn2
    always computes.  `.log` holds (context, i, t, stack_ran, attention_computed)."""
    from tests.taylorseer_ref import TaylorSeerRef, _embed, _head, update_ref

    class FasterCacheAttentionRef(TaylorSeerRef):
        def _hooked(self, st, key, compute, k, run):
            if key.endswith(".attn2"):
                return run()
            f = st["factors"].get(key, [])
            if compute:
                y = run()
                st["factors"][key], _ = update_ref(y, f, len(f), 1, 1, y.dtype)      # f_0 = y_1, f_1 = T(y_1 - y_0)
                return y
            cb = self.config.attention_weight_callback
            w = f32(0.5 if cb is None else cb(None))
            p = f[0].float()
            if len(f) > 1:
                p = p + f[1].float() * torch.full_like(p, w)
            return p                                   # fp32: the consumer rounds once, as the kernel's epilogue does

        def __call__(self, context, hidden_states, timestep, txt):
            st = self.state.setdefault(context, {"s": 0, "n": 0, "ran_prev": False, "factors": {}})
            i, t = st["s"], float(self.config.current_timestep_callback())
            compute = attention_computes(i, t, st["n"], st["ran_prev"], self.config)
            self.log.append((context, i, t, True, compute))
            st["s"], st["ran_prev"] = i + 1, True
            if compute:
                st["n"] = min(st["n"] + 1, 2)
            x, temb, tproj, txt, rot, geo = _embed(self.sd, self.cfg, hidden_states, timestep, txt)
            for li in range(self.cfg["num_layers"]):
                x = self._block(st, compute, 1, f"blocks.{li}", x, txt, tproj, rot)
            return _head(self.sd, self.cfg, x, temb, geo)

    return FasterCacheAttentionRef(sd, cfg, config)
