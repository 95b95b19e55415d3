"""Calibration of the dynamic block-sparse self-attention: per (layer, head) the smallest cdf threshold
whose sparse output stays within a relative L1 error of the dense output, measured on the user's own weights and inputs.

    config, report = calibrate_sparse_attention(model, run, l1_bound=0.05, base=SparseAttentionConfig(window_frames=1))
    model.enable_sparse_attention(config)

While `run()` executes -- any callable that performs forwards of `model`: a direct call, `lambda: pipe(..., num_inference_steps=4)`
-- every self-attention call of a layer outside `base.skip_layers` computes the dense output o_d (the forward continues with it: a
calibration run IS a dense run, bit for bit) and, per grid value g, the sparse output o_g: the plan with cdf = g, `base`'s forced
tiles and `base`'s similarity gate, then the tile walk.  sum |o_g - o_d| and sum |o_d| are accumulated per (layer, head, g) in fp32
on the device over all rows, batch elements and calls.  Offline work: the reductions are plain torch, none of it runs in an
ordinary forward, and the pipeline's loop runs eagerly meanwhile (`window_attention_runs_eagerly`).

err = sum |o_g - o_d| / sum |o_d|.  The threshold of (layer, head) is the smallest g such that g and every larger grid value
have err <= l1_bound; none: 1.0, that head stays dense.

Random weights say nothing about what a real checkpoint's heads look like; this tool is how someone with the checkpoint finds out."""
import dataclasses
import json

import torch

from .window_attention import Q_BLOCK, SparseAttentionConfig


def choose_thresholds(err, grid, l1_bound):
    """err [..., len(grid)] (grid ascending) -> per leading index the smallest g such that g and every larger grid value have
    err <= l1_bound, else 1.0.  A NaN error (sum |o_d| = 0) counts as a miss."""
    err = torch.as_tensor(err, dtype=torch.float64)
    flat = err.reshape(-1, len(grid))
    out = []
    for row in flat.tolist():
        pick = 1.0
        for g, e in zip(reversed(grid), reversed(row)):
            if not e <= l1_bound:
                break
            pick = float(g)
        out.append(pick)
    return torch.tensor(out, dtype=torch.float64).reshape(err.shape[:-1])


def _popcount(mask):
    """int32 [...] -> int64 [...]: set bits per word"""
    w = mask.view(torch.int32).to(torch.int64) & 0xffffffff
    return ((w.unsqueeze(-1) >> torch.arange(32, device=mask.device)) & 1).sum(-1)


class _Calibration:
    """the running sums; `attend` stands in for the tile route of `SelfAttentionOptionsMixin._attend_tiles`"""

    def __init__(self, grid, similarity):
        self.grid, self.similarity = grid, similarity
        self.diff, self.ref, self.kept, self.total, self.calls = {}, {}, {}, {}, {}

    def attend(self, model, ops, q, k, v, heads, tiles, **kw):
        out = ops.attention(q, k, v, heads, **kw)                        # the dense call, as a dense forward makes it
        b, lq, hd = q.shape
        li, dh = tiles.layer, hd // heads
        dev = q.device
        if li not in self.diff:
            self.diff[li] = torch.zeros(len(self.grid), heads, dtype=torch.float32, device=dev)
            self.ref[li] = torch.zeros(heads, dtype=torch.float32, device=dev)
            self.kept[li] = torch.zeros(len(self.grid), heads, dtype=torch.int64, device=dev)
            self.total[li], self.calls[li] = 0, 0
        o_d = out.float().reshape(b, lq, heads, dh)
        self.ref[li] += o_d.abs().sum((0, 1, 3))
        gate = {} if self.similarity is None else {"similarity_threshold": self.similarity}
        for gi, g in enumerate(self.grid):
            mask = ops.attention_tile_plan(q, k, heads, g, keep_ranges=tiles.keep, scale=kw.get("scale"), **gate)
            o_g = ops.attention_tiles(q, k, v, heads, mask, scale=kw.get("scale"))
            self.diff[li][gi] += (o_g.float().reshape(b, lq, heads, dh) - o_d).abs().sum((0, 1, 3))
            self.kept[li][gi] += _popcount(mask).sum((0, 2, 3))
        self.total[li] += b * -(-lq // Q_BLOCK) * -(-k.shape[1] // 64)
        self.calls[li] += 1
        return out


def calibrate_sparse_attention(model, run, *, l1_bound, grid=(0.5, 0.6, 0.7, 0.8, 0.9, 0.95), base=None):
    """-> (SparseAttentionConfig, report).  The config is `base` (default: SparseAttentionConfig()) with `head_thresholds` filled
    for every layer outside `base.skip_layers` that made a sparse-eligible self-attention call during `run()`.  report: {"grid",
    "l1_bound", "error": {layer: [heads][len(grid)]}, "density": {layer: [heads][len(grid)]} (kept share of the (q-block, key
    tile) entries, from popcounts of the masks), "thresholds": {layer: [heads]}, "calls": {layer: n}}.  The model's sparse
    attention setting is put back afterwards.
    Thresholds are calibrated in bf16 / fp16 and loaded: with fp8 attention on (`enable_fp8_attention`) this raises
    NotImplementedError before anything is launched -- the dense reference and the tile walks here are the bf16 / fp16 ones, and
    the masks are predicted from the bf16 / fp16 q and k whatever the operands of the walk."""
    base = SparseAttentionConfig() if base is None else base
    if not isinstance(base, SparseAttentionConfig):
        raise TypeError(f"base: a SparseAttentionConfig is needed, got {type(base)}")
    grid = tuple(float(g) for g in grid)
    if not grid or any(not 0 < g < 1 for g in grid) or any(a >= b for a, b in zip(grid, grid[1:])):
        raise ValueError(f"grid = {grid}: ascending thresholds in (0, 1) are needed")
    if isinstance(l1_bound, bool) or not isinstance(l1_bound, (int, float)) or not l1_bound > 0:
        raise ValueError(f"l1_bound = {l1_bound!r}: a number > 0 is needed")
    if getattr(model, "_sparse_calib", None) is not None:
        raise RuntimeError("a calibration of this model is already running")
    if getattr(model, "fp8_attention", False):
        raise NotImplementedError("calibrate_sparse_attention with fp8 attention: thresholds are calibrated in bf16 / fp16 and "
                                  "loaded; enable_fp8_attention(False) first, calibrate, then switch fp8 attention back on")
    before = model._sparse
    state = _Calibration(grid, base.similarity_threshold)
    # the model's own host path builds the forced tiles, skips `skip_layers` and hands every other call to `state.attend`
    model.enable_sparse_attention(dataclasses.replace(base, cdf_threshold=grid[0], head_thresholds=None, keep_masks=False))
    model._sparse_calib = state
    try:
        run()
    finally:
        model._sparse_calib = None
        model.disable_sparse_attention()
        if before is not None:
            model.enable_sparse_attention(before)
    report = _report(state, l1_bound)
    return dataclasses.replace(base, head_thresholds={li: tuple(t) for li, t in report["thresholds"].items()}), report


def _report(state, l1_bound):
    grid = state.grid
    error, density, thresholds = {}, {}, {}
    for li in sorted(state.diff):
        err = (state.diff[li].double() / state.ref[li].double()).t().cpu()               # [heads][grid]
        error[li] = err.tolist()
        density[li] = (state.kept[li].double() / state.total[li]).t().cpu().tolist()
        thresholds[li] = choose_thresholds(err, grid, l1_bound).tolist()
    return {"grid": list(grid), "l1_bound": float(l1_bound), "error": error, "density": density, "thresholds": thresholds,
            "calls": dict(state.calls)}


_FIELDS = ("cdf_threshold", "window_frames", "sink_frames", "skip_layers", "similarity_threshold", "head_thresholds")


def save_sparse_thresholds(path, config):
    """the config (without `keep_masks`) as plain JSON; layers become string keys"""
    d = {f: getattr(config, f) for f in _FIELDS}
    d["head_thresholds"] = None if d["head_thresholds"] is None else {str(li): list(r) for li, r in d["head_thresholds"].items()}
    d["sink_frames"], d["skip_layers"] = list(d["sink_frames"]), list(d["skip_layers"])
    with open(path, "w") as f:
        json.dump({"format": "frameino_amd.sparse_thresholds", "version": 1, **d}, f, indent=1)


def load_sparse_thresholds(path):
    """-> the SparseAttentionConfig `save_sparse_thresholds` wrote"""
    with open(path) as f:
        d = json.load(f)
    if d.get("format") != "frameino_amd.sparse_thresholds":
        raise ValueError(f"{path}: not a file of save_sparse_thresholds")
    ht = d.get("head_thresholds")
    return SparseAttentionConfig(cdf_threshold=d["cdf_threshold"], window_frames=d["window_frames"],
                                 sink_frames=tuple(d["sink_frames"]), skip_layers=tuple(d["skip_layers"]),
                                 similarity_threshold=d.get("similarity_threshold"),
                                 head_thresholds=None if ht is None else {int(li): tuple(r) for li, r in ht.items()})
