"""fp64 reference of the guiders (frameino_amd/guiders.py), in TENSOR form -- the published operations on the two predictions
of one sample, not the (A, B) form the kernels use:

    CFG-Zero*          the optimal scale by flattened dot products, `s u + g (c - s u)`; zeros on the first steps
    APG                clip `c - u` to the norm threshold, project on c, recombine `u + g (orth + eta par)`
    guidance rescale   `torch.std` of the conditional and of the combined prediction over the sample

the tables of configs and degenerate inputs the test files share, and a host stand-in for the guided kernels
(`HostGuidedOps`): the loop's own transformer predictions, combined here in fp64, then the sampler's linear step from the
coefficient row in fp64.
"""
import torch

from frameino_amd.guiders import (APG, ZERO_STAR, AdaptiveProjectedGuidanceConfig, CFGZeroStarConfig,
                                  GuidanceRescaleConfig)

# the guiders the CPU and the kernel tests run: each alone, each with the rescale, APG with the clip binding and with eta alone
CONFIGS = {
    "rescale": GuidanceRescaleConfig(guidance_rescale=0.7),
    "zero_star": CFGZeroStarConfig(zero_init_steps=1),
    "zero_star+rescale": CFGZeroStarConfig(zero_init_steps=1, guidance_rescale=0.5),
    "apg_clipping": AdaptiveProjectedGuidanceConfig(norm_threshold=15.0, eta=0.0),
    "apg_eta": AdaptiveProjectedGuidanceConfig(norm_threshold=0.0, eta=0.3),
    "apg+rescale": AdaptiveProjectedGuidanceConfig(norm_threshold=15.0, eta=0.5, guidance_rescale=0.7),
}


def combine(config, c, u, g, step=0):
    """v for one sample; c, u of any shape (the n elements the step updates), computed in fp64"""
    c, u, g = c.double(), u.double(), float(g)
    if config.kind == ZERO_STAR:
        if step < config.zero_init_steps:
            return torch.zeros_like(c)
        cf, uf = c.flatten(), u.flatten()
        s = torch.dot(cf, uf) / (torch.dot(uf, uf) + 1e-8)
        v = s * u + g * (c - s * u)
    elif config.kind == APG:
        diff = c - u
        if config.norm_threshold > 0:
            norm = torch.linalg.vector_norm(diff)
            if norm > 0:
                diff = diff * torch.clamp(config.norm_threshold / norm, max=1.0)
        cc = (c * c).sum()
        par = ((diff * c).sum() / cc) * c if cc > 0 else torch.zeros_like(c)
        orth = diff - par
        v = u + g * (orth + config.eta * par)
    else:
        v = u + g * (c - u)
    phi = float(config.guidance_rescale)
    if phi > 0:
        f = 1.0
        if c.numel() >= 2:
            std_c, std_v = torch.std(c), torch.std(v)
            if std_v > 0:
                f = std_c / std_v
        v = v * (phi * f + 1.0 - phi)
    return v


def moments(c, u):
    """(Sc, Su, Scc, Suu, Scu) in fp64 as Python floats"""
    c, u = c.double().flatten(), u.double().flatten()
    return tuple(float(x) for x in (c.sum(), u.sum(), torch.dot(c, c), torch.dot(u, u), torch.dot(c, u)))


def family(n, seed, device="cpu"):
    """the input family of the tests: c ~ N(0.1, 1), u = 0.8 c + 0.6 z (correlated: no variance is ill-conditioned)"""
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(n, generator=g, dtype=torch.float64) + 0.1
    u = 0.8 * c + 0.6 * torch.randn(n, generator=g, dtype=torch.float64)
    return c.to(device), u.to(device)


# the degenerate inputs of tests/test_guiders_cpu.py (what every guider makes of them) and tests/test_guiders_kernels_gpu.py
def degenerate_cases():
    c, u = family(64, seed=3)
    z = torch.zeros(64, dtype=torch.float64)
    return {"u=0": (c, z), "c=0": (z, u), "c==u": (c, c.clone()),
            "constants": (torch.full((64,), 0.5, dtype=torch.float64), torch.full((64,), 0.25, dtype=torch.float64)),
            "n=1": (c[:1], u[:1])}


class HostGuidedOps:
    """`ops` with the guider's launches replaced by this file's fp64 host arithmetic; everything else goes to the real module.
    The step index is counted here, from the calls -- not read from the loop's zero-init flag."""

    def __init__(self, real, config):
        self._real, self._config, self._step, self._v = real, config, 0, None

    def __getattr__(self, name):
        return getattr(self._real, name)

    # -- Wan: preds [C, Ft, H, W], the first gen_frames frames are the sample
    def guider_coefs(self, cond_pred, uncond_pred, gen_frames, args, g_dev, zero_dev, workspace, ab):
        self._v = combine(self._config, cond_pred[:, :gen_frames], uncond_pred[:, :gen_frames], g_dev.item(), self._step)
        self._step += 1

    def guided_euler_step_(self, lat, cond_pred, uncond_pred, ab, dt_dev, round_out=True):
        lat.copy_(lat.double() + dt_dev.double() * self._v)

    def guided_unipc_step_(self, x, last, m0, m1, cond_pred, uncond_pred, coef_dev, ab):
        k = coef_dev.double().tolist()
        x64, a0 = x.double(), m0.double()
        mt = x64 - k[1] * self._v
        xc = k[3] * last.double() + k[4] * a0 + k[5] * m1.double() + k[6] * mt if k[2] != 0 else x64
        x.copy_(k[7] * xc + k[8] * mt + k[9] * a0)
        last.copy_(xc)
        m1.copy_(a0)
        m0.copy_(mt)

    # -- CogVideoX: pred [2, Ft, C, H, W] (uncond, cond), the first n_lat elements of each are the sample
    def guider_coefs_rows(self, pred, n_lat, args, g_dev, zero_dev, workspace, ab):
        p = pred.reshape(2, -1)[:, :n_lat]
        self._v = combine(self._config, p[1], p[0], g_dev.item(), self._step)
        self._step += 1

    def guided_vpred_step_(self, lat, pred, coef_dev, ab):
        sa, sb, ca, cb = coef_dev.double().tolist()[:4]
        x = lat.double().flatten()
        x0 = sa * x - sb * self._v
        lat.copy_((ca * x + cb * x0).reshape(lat.shape))

    def guided_dpm_step_(self, lat, pred, x0_old, noise, coef_dev, ab):
        sa, sb, m1, m2, m3, m4, mn, _, use_old = coef_dev.double().tolist()[:9]
        x = lat.double().flatten()
        x0 = sa * x - sb * self._v
        d = m3 * x0 - m4 * x0_old.double().flatten() if use_old != 0 else x0
        lat.copy_((m1 * x - m2 * d + mn * noise.double().flatten()).reshape(lat.shape))
        x0_old.copy_(x0.reshape(x0_old.shape))
