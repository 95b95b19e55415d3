"""Restatement of MagCache (frameino_amd/step_cache.py) for the tests: the rule in exact `fractions.Fraction` arithmetic, written
independently of `magcache_decide`; the calibration quantity in fp64 torch; and a Wan DiT forward composed from oracle.wan_dit
pieces (built like `FirstBlockCacheRef` in tests/step_cache_ref.py, whose embedding and head it imports) that runs the whole
block stack or re-uses its residual.  oracle/ itself is not changed."""
from fractions import Fraction

import torch

from oracle import wan_dit as W
from tests.step_cache_ref import _embed, _head


def retention(retention_ratio, n):
    """R = floor(retention_ratio * N + 1/2), exactly"""
    return (Fraction(retention_ratio) * n + Fraction(1, 2)).__floor__()


def rule_trace(forwards, ratios, n, threshold=0.06, max_skip_steps=3, retention_ratio=0.2, calibrate=False):
    """[(s, computed, acc_err, acc_steps)] of `forwards` consecutive forwards of one context, the accumulators as they stand
    after the decision (Fractions).  The context starts over when its counter reaches n."""
    thr, keep = Fraction(threshold), retention(retention_ratio, n)
    out, s = [], 0
    ratio, steps, err, residual = Fraction(1), 0, Fraction(0), False
    for _ in range(forwards):
        if calibrate or s < keep:
            compute = True
        else:
            ratio *= Fraction(ratios[s]) if s < len(ratios) else 1
            steps += 1
            err += abs(1 - ratio)
            compute = not (residual and err <= thr and steps <= max_skip_steps)
            if compute:
                ratio, steps, err = Fraction(1), 0, Fraction(0)
        residual = residual or compute
        out.append((s, compute, err, steps))
        s += 1
        if s == n:
            s, ratio, steps, err, residual = 0, Fraction(1), 0, Fraction(0), False
    return out


def decision_margins(forwards, ratios, n, threshold=0.06, max_skip_steps=3, retention_ratio=0.2):
    """|acc_err - threshold| of every forward that compared the two (Fractions): the test's condition on its own inputs"""
    thr, keep = Fraction(threshold), retention(retention_ratio, n)
    out, s = [], 0
    ratio, steps, err, residual = Fraction(1), 0, Fraction(0), False
    for _ in range(forwards):
        compute = True
        if s >= keep:
            ratio *= Fraction(ratios[s]) if s < len(ratios) else 1
            steps += 1
            err += abs(1 - ratio)
            out.append(abs(err - thr))
            compute = not (residual and err <= thr and steps <= max_skip_steps)
            if compute:
                ratio, steps, err = Fraction(1), 0, Fraction(0)
        residual = True
        s += 1
        if s == n:
            s, ratio, steps, err, residual = 0, Fraction(1), 0, Fraction(0), False
    return out


def calibration(r_new, r_prev):
    """(mean ratio, mean cos_dist) over the rows of two residuals [rows, D] in their storage dtype: the norms and the dot
    product over the feature axis of the values as stored, here in fp64"""
    a, p = r_new.double(), r_prev.double()
    na, npv = a.norm(dim=-1), p.norm(dim=-1)
    ratio = na / (npv + 1e-8)
    cos = 1.0 - (a * p).sum(-1) / torch.clamp(na * npv, min=1e-8)
    return float(ratio.mean()), float(cos.mean())


def mean_norm_ratio(r_new, r_prev):
    """what a kernel that averaged the norms instead of the ratios would report"""
    return float(r_new.double().norm(dim=-1).mean() / (r_prev.double().norm(dim=-1).mean() + 1e-8))


class MagCacheRef:
    """`ref(context, hidden_states, timestep, text)`: one forward with MagCache under `context`, the decisions from
    `rule_trace`'s arithmetic.  `log` holds (context, s, computed) per forward; `residuals[context]` the stored residual."""

    def __init__(self, sd, cfg, ratios, n, **rule):
        self.sd, self.cfg, self.ratios, self.n, self.rule = sd, cfg, ratios, n, rule
        self.count, self.residuals, self.log = {}, {}, []

    def stack(self, h0, txt, tproj, rot):
        x = h0
        for i in range(self.cfg["num_layers"]):
            x = W.wan_block(self.sd, f"blocks.{i}", self.cfg, x, txt, tproj, rot)
        return x

    def uncached(self, hidden_states, timestep, txt):
        h0, temb, tproj, txt, rot, geo = _embed(self.sd, self.cfg, hidden_states, timestep, txt)
        return _head(self.sd, self.cfg, self.stack(h0, txt, tproj, rot), temb, geo)

    def __call__(self, context, hidden_states, timestep, txt):
        h0, temb, tproj, txt, rot, geo = _embed(self.sd, self.cfg, hidden_states, timestep, txt)
        done = self.count.get(context, 0)
        ratios = self.ratios[context] if isinstance(self.ratios, dict) else self.ratios
        s, compute, _, _ = rule_trace(done + 1, ratios, self.n, **self.rule)[-1]
        self.count[context] = done + 1
        self.log.append((context, s, compute))
        if compute:
            x = self.stack(h0, txt, tproj, rot)
            self.residuals[context] = x - h0
        else:
            x = h0 + self.residuals[context]
        return _head(self.sd, self.cfg, x, temb, geo)
