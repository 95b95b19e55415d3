"""Guiders: how the sampler loops combine the conditional and the unconditional prediction.

Plain classifier-free guidance is `u + g (c - u)`.  Three published refinements are offered here, as diffusers ships them
(`diffusers.guiders`), on both FrameINO pipelines:

    CFGZeroStarConfig                CFG-Zero* (Fan et al. 2025): the unconditional branch rescaled by the optimal scalar
                                     s = <c, u> / (<u, u> + 1e-8), `s u + g (c - s u)`, and a zero prediction on the first
                                     `zero_init_steps` steps
    AdaptiveProjectedGuidanceConfig  APG (Sadat et al. 2024): `c - u` clipped to the norm `norm_threshold`, split into its
                                     projection on c and the remainder, `u + g (orth + eta par)`
    GuidanceRescaleConfig            guidance rescale (Lin et al. 2024) on plain CFG: the combined prediction rescaled towards the
                                     standard deviation of c, `phi f + 1 - phi` with f = std(c) / std(v); `guidance_rescale=`
                                     adds the same to the other two

Every one of them is `v = A c + B u` with two scalars that depend on five global moments of (c, u) over one sample -- exactly the
elements the step kernel updates -- so a guided step is `fino_guider_coefs` (two small launches, csrc/fino_guidance.hip: moments
in fp64, {A, B} written to device memory) and the `fino_guided_*_step` sibling of the loop's fused step kernel.  Nothing is read
on the host: the guided step replays from the captured hipGraph like the plain one.  `coefficients()` below is the same
formulas on the host in fp64; the kernel mirrors it term by term.

    pipe.set_guider(CFGZeroStarConfig(zero_init_steps=1))
    pipe.set_guider(AdaptiveProjectedGuidanceConfig(norm_threshold=15.0, eta=0.0, guidance_rescale=0.5))
    pipe.disable_guider()

A guider applies when the call guides at all (guidance_scale > 1 and a negative prompt); without one, or with guidance off, the
loop issues exactly the calls it issued before.  It sits after the model, so it composes with the step caches, the attention
variants and the MX linears.  Not built: guidance intervals (`start` / `stop`), APG momentum (a running-difference buffer),
`use_original_formulation`, and a parallel plan (a rank may hold one CFG branch only).  What a guider does to the videos is not
measured in this repository: no claim about quality is made.
"""
import math
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional

RESCALE, ZERO_STAR, APG = 0, 1, 2            # FINO_GUIDER_* (include/frameino_hip.h)


def _check_rescale(phi):
    if not isinstance(phi, (int, float)) or isinstance(phi, bool) or not (0.0 <= float(phi) <= 1.0):
        raise ValueError(f"`guidance_rescale` must be a number in [0, 1], got {phi!r}")


@dataclass(frozen=True)
class CFGZeroStarConfig:
    zero_init_steps: int = 1
    guidance_rescale: float = 0.0
    kind = ZERO_STAR

    def __post_init__(self):
        if not isinstance(self.zero_init_steps, int) or isinstance(self.zero_init_steps, bool) or self.zero_init_steps < 0:
            raise ValueError(f"`zero_init_steps` must be an integer >= 0, got {self.zero_init_steps!r}")
        _check_rescale(self.guidance_rescale)


@dataclass(frozen=True)
class AdaptiveProjectedGuidanceConfig:
    norm_threshold: float = 15.0
    eta: float = 1.0
    momentum: Optional[float] = None
    guidance_rescale: float = 0.0
    kind = APG

    def __post_init__(self):
        for name in ("norm_threshold", "eta"):
            v = getattr(self, name)
            if not isinstance(v, (int, float)) or isinstance(v, bool) or not math.isfinite(v):
                raise ValueError(f"`{name}` must be a finite number, got {v!r}")
        if self.momentum is not None and (not isinstance(self.momentum, (int, float)) or isinstance(self.momentum, bool)):
            raise ValueError(f"`momentum` must be None or a number, got {self.momentum!r}")
        _check_rescale(self.guidance_rescale)


@dataclass(frozen=True)
class GuidanceRescaleConfig:
    guidance_rescale: float = 0.7
    kind = RESCALE

    def __post_init__(self):
        _check_rescale(self.guidance_rescale)


GUIDER_CONFIGS = (CFGZeroStarConfig, AdaptiveProjectedGuidanceConfig, GuidanceRescaleConfig)


def coefficients(config, moments, n, g, step=0):
    """(A, B) of `v = A c + B u` in fp64 (Python floats).  `moments` = (Sc, Su, Scc, Suu, Scu) over the n elements of one sample,
    `g` the step's guidance scale, `step` the index of the step in the loop.  csrc/fino_guidance.hip::guider_formulas is this
    text on the device."""
    Sc, Su, Scc, Suu, Scu = (float(m) for m in moments)
    n, g = float(n), float(g)
    if config.kind == ZERO_STAR:
        if step < config.zero_init_steps:
            return 0.0, 0.0
        s = Scu / (Suu + 1e-8)
        a0, b0 = g, (1.0 - g) * s
    elif config.kind == APG:
        dd = Scc - 2.0 * Scu + Suu
        s = 1.0
        if config.norm_threshold > 0.0 and dd > 0.0:            # (dd is a sum of squares: below zero only by rounding)
            s = min(1.0, config.norm_threshold / math.sqrt(dd))
        p = s * (Scc - Scu) / Scc if Scc > 0.0 else 0.0
        a0, b0 = g * (s + (config.eta - 1.0) * p), 1.0 - g * s
    else:
        a0, b0 = g, 1.0 - g
    m = 1.0
    phi = float(config.guidance_rescale)
    if phi > 0.0:
        f = 1.0
        if n >= 2.0:
            var_c = max((Scc - Sc * Sc / n) / (n - 1.0), 0.0)    # (a variance: below zero only by rounding)
            var_u = max((Suu - Su * Su / n) / (n - 1.0), 0.0)
            cov = (Scu - Sc * Su / n) / (n - 1.0)
            var_p = a0 * a0 * var_c + b0 * b0 * var_u + 2.0 * a0 * b0 * cov
            if var_p > 0.0:
                f = math.sqrt(var_c / var_p)
        m = phi * f + 1.0 - phi
    return m * a0, m * b0


def kernel_args(config):
    """(kind, norm_threshold, eta, guidance_rescale) of fino_guider_coefs"""
    return (config.kind, float(getattr(config, "norm_threshold", 0.0)), float(getattr(config, "eta", 1.0)),
            float(config.guidance_rescale))


class GuiderPipelineMixin:
    """`set_guider(config)` / `disable_guider()` / `guider` on a pipeline, and the loop-state helpers both loops share."""

    _guider = None

    @property
    def guider(self):
        return self._guider

    def set_guider(self, config):
        if not isinstance(config, GUIDER_CONFIGS):
            raise TypeError(f"set_guider takes one of {', '.join(c.__name__ for c in GUIDER_CONFIGS)}, got "
                            f"{type(config).__name__}")
        self._guider = config
        return self

    def disable_guider(self):
        self._guider = None
        return self

    def _guider_check(self):
        """the limits of a guider, checked before any launch.  -> the config or None"""
        cfg = self._guider
        if cfg is None:
            return None
        if getattr(cfg, "momentum", None) is not None:
            raise NotImplementedError("adaptive projected guidance with `momentum`: the running difference of the predictions "
                                      "needs a buffer across steps, which is not built; use momentum=None")
        if getattr(self, "parallel", None) is not None or getattr(self.transformer, "parallel", None) is not None:
            raise NotImplementedError("a guider runs on one GPU: it needs both CFG branches of a sample in one place, and under a "
                                      "parallel plan a rank may hold one branch only")
        return cfg

    @staticmethod
    def _guider_state(ops, cfg, n, g_dev, num_steps, device):
        """The guider's part of the loop state, allocated once (a captured step replays these buffers): the workspace of the
        moments, {A, B}, the guidance scale's device slot `g_dev` (one float, refreshed by whoever owns it) and the zero-init
        flag with its per-step values (a device copy per step, like the coefficient rows)."""
        import torch
        gs = SimpleNamespace(config=cfg, args=kernel_args(cfg), g=g_dev)
        gs.workspace = torch.empty(ops.guider_workspace_bytes(n), dtype=torch.uint8, device=device)
        gs.ab = torch.zeros(2, dtype=torch.float32, device=device)
        gs.zero = gs.zero_steps = None
        if cfg.kind == ZERO_STAR:
            gs.zero = torch.zeros(1, dtype=torch.float32, device=device)
            gs.zero_steps = torch.tensor([1.0 if i < cfg.zero_init_steps else 0.0 for i in range(num_steps)],
                                         dtype=torch.float32, device=device)
        return gs

    @staticmethod
    def _guider_begin_step(gs, i):
        """before step i: the zero-init flag from the step index (device-to-device: no host sync)"""
        if gs is not None and gs.zero is not None:
            gs.zero.copy_(gs.zero_steps[i:i + 1])


# ---- the examples' flags (examples/run_wan_frameino.py, examples/run_cogvideox_frameino.py) ----------------------------------
def add_guider_arguments(ap):
    ap.add_argument("--cfg-zero-star", type=int, nargs="?", const=1, default=None, metavar="K",
                    help="CFG-Zero* guidance (quality on real checkpoints unmeasured): the unconditional prediction rescaled by "
                         "its optimal scalar, and a zero prediction on the first K steps (default 1)")
    ap.add_argument("--apg", type=float, default=None, metavar="R",
                    help="adaptive projected guidance (quality on real checkpoints unmeasured): the guidance direction clipped to "
                         "the norm R, e.g. 15 (0: no clip), its part along the conditional prediction weighted by --apg-eta")
    ap.add_argument("--apg-eta", type=float, default=1.0, metavar="E", help="with --apg: weight of the parallel part (default 1)")
    ap.add_argument("--guidance-rescale", type=float, default=None, metavar="PHI",
                    help="guidance rescale (quality on real checkpoints unmeasured): the guided prediction rescaled towards the "
                         "standard deviation of the conditional one, PHI in [0, 1], e.g. 0.7; alone (on plain CFG) or with "
                         "--cfg-zero-star / --apg")


def guider_from_arguments(ap, a):
    """the config the flags ask for, or None; argparse errors for combinations that make no sense"""
    if a.cfg_zero_star is not None and a.apg is not None:
        ap.error("--cfg-zero-star and --apg: one guider at a time")
    if a.apg is None and a.apg_eta != 1.0:
        ap.error("--apg-eta needs --apg")
    phi = 0.0 if a.guidance_rescale is None else a.guidance_rescale
    try:
        if a.cfg_zero_star is not None:
            return CFGZeroStarConfig(zero_init_steps=a.cfg_zero_star, guidance_rescale=phi)
        if a.apg is not None:
            return AdaptiveProjectedGuidanceConfig(norm_threshold=a.apg, eta=a.apg_eta, guidance_rescale=phi)
        if a.guidance_rescale is not None:
            return GuidanceRescaleConfig(guidance_rescale=phi)
    except ValueError as ex:
        ap.error(str(ex))
    return None
