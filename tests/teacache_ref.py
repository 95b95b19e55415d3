"""Restatement of TeaCache (frameino_amd/step_cache.py) for the tests: the rule in exact `fractions.Fraction` arithmetic, written
independently of `teacache_decide`; the probe's quantities in fp64 torch; and a Wan DiT forward composed from oracle.wan_dit
pieces (built like `MagCacheRef` in tests/magcache_ref.py, with the embedding and head of tests/step_cache_ref.py) that measures
block 0's modulated input, decides, and runs the whole block stack or re-uses its residual.  oracle/ itself is not changed."""
import math
from fractions import Fraction

import torch

from oracle import wan_dit as W
from tests.step_cache_ref import _embed, _head


def poly(coefficients, d):
    """P(d), coefficients highest power first, exactly"""
    return sum(Fraction(c) * Fraction(d) ** (len(coefficients) - 1 - i) for i, c in enumerate(coefficients))


def _usable(d):
    return d is not None and math.isfinite(d)


def rule_trace(ds, n, coefficients, rel_l1_thresh=0.2, ret_steps=1, cutoff_steps=None, max_skip_steps=None, calibrate=False,
               margins=None):
    """[(s, computed, acc, measured)] of len(ds) consecutive forwards of one context, `ds[i]` the distance forward i measured
    (ignored where the rule computes unconditionally -- `measured` False --; NaN / inf: no skip), acc as it stands after the
    decision (a Fraction).  The context starts over when its counter reaches n.  `margins`: a list that receives
    (acc, threshold) of every forward that compared them."""
    thr = Fraction(rel_l1_thresh)
    cut = n - 1 if cutoff_steps is None else cutoff_steps
    out, s, acc, row, ready = [], 0, Fraction(0), 0, False
    for d in ds:
        measured = not (calibrate or not ready or s < ret_steps or s >= cut)
        if not measured or not _usable(d):
            compute, acc, row = True, Fraction(0), 0
        else:
            acc += poly(coefficients, d)
            if margins is not None:
                margins.append((acc, thr))
            if acc < thr and (max_skip_steps is None or row < max_skip_steps):
                compute, row = False, row + 1
            else:
                compute, acc, row = True, Fraction(0), 0
        ready = True
        out.append((s, compute, acc, measured))
        s += 1
        if s == n:
            s, acc, row, ready = 0, Fraction(0), 0, False
    return out


def modulated(x, shift, scale, sel=None, eps=1e-6):
    """block 0's norm1 modulation of the rows x [rows, D] in the dtype of x: T(LN(x) * (1 + scale[sel]) + shift[sel]), the
    statistics and the arithmetic in fp32 (oracle.wan_dit.wan_block's line)"""
    if sel is not None:
        shift, scale = shift[sel.long()], scale[sel.long()]
    return (W.fp32_layer_norm(x.float(), None, None, eps) * (1 + scale.float()) + shift.float()).to(x.dtype)


def sums(m, p):
    """(sum |m - p|, sum |p|) over two planes in their storage dtype, here in fp64"""
    return float((m.double() - p.double()).abs().sum()), float(p.double().abs().sum())


def rel_l1(m, p):
    a, q = sums(m, p)
    return a / q


class TeaCacheRef:
    """`ref(context, hidden_states, timestep, text)`: one forward with TeaCache under `context`.  `log` holds
    (context, s, computed, d, acc) per forward -- d None where the rule compares nothing --, `margins` (acc, threshold) of every
    comparison, `residuals[context]` the stored residual."""

    def __init__(self, sd, cfg, coefficients, n, **rule):
        self.sd, self.cfg, self.coefficients, self.n, self.rule = sd, cfg, coefficients, n, rule
        self.ds, self.planes, self.residuals, self.log, self.margins = {}, {}, {}, [], []

    def stack(self, h0, txt, tproj, rot):
        x = h0
        for i in range(self.cfg["num_layers"]):
            x = W.wan_block(self.sd, f"blocks.{i}", self.cfg, x, txt, tproj, rot)
        return x

    def uncached(self, hidden_states, timestep, txt):
        h0, temb, tproj, txt, rot, geo = _embed(self.sd, self.cfg, hidden_states, timestep, txt)
        return _head(self.sd, self.cfg, self.stack(h0, txt, tproj, rot), temb, geo)

    def probe(self, h0, tproj):
        """block 0's modulated input [B, L, D] (oracle.wan_dit.wan_block :334)"""
        table = self.sd["blocks.0.scale_shift_table"]
        if tproj.ndim == 4:
            mods = (table.unsqueeze(0) + tproj.float()).chunk(6, dim=2)
            shift, scale = mods[0].squeeze(2), mods[1].squeeze(2)
        else:
            shift, scale = (table + tproj.float()).chunk(6, dim=1)[:2]
        return (W.fp32_layer_norm(h0.float(), None, None, self.cfg["eps"]) * (1 + scale) + shift).type_as(h0)

    def __call__(self, context, hidden_states, timestep, txt):
        h0, temb, tproj, txt, rot, geo = _embed(self.sd, self.cfg, hidden_states, timestep, txt)
        m = self.probe(h0, tproj)
        ds = self.ds.setdefault(context, [])
        if len(ds) % self.n == 0:                   # the context starts over: no plane
            self.planes.pop(context, None)
        prev = self.planes.get(context)
        d = None if prev is None else rel_l1(m, prev)
        self.planes[context] = m
        ds.append(d)
        coef = self.coefficients[context] if isinstance(self.coefficients, dict) else self.coefficients
        mine = []
        s, compute, acc, measured = rule_trace(ds, self.n, coef, margins=mine, **self.rule)[-1]
        if measured and mine and _usable(d):        # (the trace replays the context: this forward's comparison is the last)
            self.margins.append(mine[-1])
        self.log.append((context, s, compute, d if measured else None, acc))
        if compute:
            x = self.stack(h0, txt, tproj, rot)
            self.residuals[context] = x - h0
        else:
            x = h0 + self.residuals[context]
        return _head(self.sd, self.cfg, x, temb, geo)
