"""Sliding-window self-attention over latent frames (opt-in, approximate).

Every query attends its own latent frame +- `window_frames` neighbours plus a few "sink" frames that every query always sees
(the conditioning first frame, the identity-reference frames appended at the end).  Tokens are frame-major, so for one 256-row
q-block "window + sinks" is at most three contiguous key ranges: the table `frame_window_ranges` builds is what
`ops.attention_ranges` (fino_attn_fwd_ranges) and `ops.attention_fp8_ranges` (fino_attn_fwd_fp8_ranges) walk -- per q-block up
to three [begin, end) ranges of 64-key tiles.

Both backbones use it.  The Wan DiT's sequence is the frames alone; the CogVideoX DiT's joint sequence is
[text | frame 0 | ... | frame F - 1 (| ID frame)], which `prefix_rows` describes: the text rows are keys every query sees and
queries that see every key.

The granularity is the kernel's: a q-block's window is the union over its rows (a block that straddles two frames sees both
frames' windows) and frame boundaries are rounded OUTWARD to key tiles, so a query may see up to 63 keys of a frame just outside
its window on either side, never fewer keys than the definition says.  `block_mask` expands a table to the boolean mask of
exactly what the kernel computes.  The tables are pure Python + CPU torch: nothing in them touches a GPU.

`SelfAttentionOptionsMixin` is the host side both DiTs inherit: the fp8 and window switches with their state, the per-forward
window decision and the one dispatch among the four `ops` self-attention front ends; `window_attention_runs_eagerly` is the rule
both pipelines apply.

Dynamic block-sparse self-attention (opt-in, approximate) lives here too: `SparseAttentionConfig`, the
mixin's `enable_sparse_attention` and the `tiles=` route of `_attend` -- a device-side predictor (`ops.attention_tile_plan`) picks
the key tiles per (batch element, head, q-block) right before each call, `ops.attention_tiles` walks them; the window tables
above are its always-kept tiles.  Wired on the Wan DiT only.  Its two safeguards are fields of the same
config: `similarity_threshold` (blocks whose tokens do not resemble each other are never predicted from) and `head_thresholds`
(one cdf threshold per layer and head; frameino_amd/sparse_calibration.py measures them on the user's own weights)."""
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Any, Callable, Mapping, Optional, Sequence, Tuple

import torch

Q_BLOCK = 256        # query rows per q-block (kQBlock of csrc/fino_attention_common.h)
KEY_TILE = 64        # keys per tile (kKV)
MAX_RANGES = 3


def _sink_frames(frames, sink_frames):
    out = []
    for s in sink_frames:
        s = int(s)
        f = s + frames if s < 0 else s
        if not 0 <= f < frames:
            raise ValueError(f"sink frame {s} is outside the {frames} latent frame(s)")
        out.append(f)
    return sorted(set(out))


def frame_window_ranges(frames, tokens_per_frame, window_frames, sink_frames=(0,), q_rows=None, prefix_rows=0):
    """-> CPU int32 [nqb, 3, 2]: per q-block of the query rows `q_rows` = (s0, s1) (default: all L = frames x tokens_per_frame
    rows; q-blocks are counted from s0) up to three ascending, disjoint [begin, end) ranges of key tiles, unused entries (0, 0).
    For q-block rows [r0, r1): f0 = r0 // tpf, f1 = (r1 - 1) // tpf; the window is frames [max(0, f0 - w), min(F, f1 + w + 1)),
    every sink frame s (negatives count from the end) is [s, s + 1); a frame interval [a, b) becomes the tiles
    [a tpf // 64, min(ntall, ceil(b tpf / 64))); intervals that overlap or touch are merged.  ValueError if more than three
    ranges remain (sinks in the middle of the clip).
    prefix_rows = p > 0: p rows (the text of a joint sequence) sit in front of frame 0, L = p + F tpf.  A q-block with any row < p is
    dense, [0, ntall).  Any other has f0 = (r0 - p) // tpf, f1 = (r1 - 1 - p) // tpf and sees the ROW intervals [0, p) (the prefix),
    [p + max(0, f0 - w) tpf, p + min(F, f1 + w + 1) tpf) (the window) and [p + s tpf, p + (s + 1) tpf) per sink frame s, each
    rounded outward to tiles, merged as above."""
    frames, tpf, w = int(frames), int(tokens_per_frame), int(window_frames)
    if frames < 1 or tpf < 1:
        raise ValueError(f"frames = {frames}, tokens_per_frame = {tpf}: both must be >= 1")
    if w < 0:
        raise ValueError(f"window_frames = {w}: must be >= 0")
    p = int(prefix_rows)
    if p < 0:
        raise ValueError(f"prefix_rows = {p}: must be >= 0")
    L = p + frames * tpf
    ntall = -(-L // KEY_TILE)
    s0, s1 = (0, L) if q_rows is None else (int(q_rows[0]), int(q_rows[1]))
    if not 0 <= s0 < s1 <= L:
        raise ValueError(f"q_rows = ({s0}, {s1}) is not a non-empty range of the {L} token rows")
    sinks = _sink_frames(frames, sink_frames)
    nqb = -(-(s1 - s0) // Q_BLOCK)
    table = torch.zeros((nqb, MAX_RANGES, 2), dtype=torch.int32)
    for i in range(nqb):
        r0 = s0 + Q_BLOCK * i
        r1 = min(r0 + Q_BLOCK, s1)
        if r0 < p:
            table[i, 0, 1] = ntall
            continue
        f0, f1 = (r0 - p) // tpf, (r1 - 1 - p) // tpf
        spans = [(max(0, f0 - w), min(frames, f1 + w + 1))] + [(s, s + 1) for s in sinks]
        rows = [(p + a * tpf, p + b * tpf) for a, b in spans] + ([(0, p)] if p else [])
        tiles = sorted((a // KEY_TILE, min(ntall, -(-b // KEY_TILE))) for a, b in rows)
        merged = [list(tiles[0])]
        for a, b in tiles[1:]:
            if a <= merged[-1][1]:
                merged[-1][1] = max(merged[-1][1], b)
            else:
                merged.append([a, b])
        if len(merged) > MAX_RANGES:
            raise ValueError(f"q-block {i} (rows [{r0}, {r1})) needs {len(merged)} key ranges {merged}; the kernel walks at most "
                             f"{MAX_RANGES}: put the sink frames at the ends of the clip")
        for j, (a, b) in enumerate(merged):
            table[i, j, 0], table[i, j, 1] = a, b
    return table


def ranges_density(table, lk):
    """fraction of the (q-block, key tile) pairs the table walks"""
    ntall = -(-int(lk) // KEY_TILE)
    t = table.clamp(0, ntall).long()
    return float((t[:, :, 1] - t[:, :, 0]).clamp_min(0).sum()) / (table.shape[0] * ntall)


def ranges_cover_all(table, lk):
    """every q-block walks every key tile: the dense attention"""
    ntall = -(-int(lk) // KEY_TILE)
    return bool(((table[:, 0, 0] <= 0) & (table[:, 0, 1] >= ntall)).all())


def block_mask(table, lq, lk, prefix_rows=0):
    """the boolean [lq, lk] mask of what `ops.attention_ranges` computes under `table` (query rows counted from the table's
    first q-block).  `prefix_rows` is the one the table was built with: the table already carries the prefix (as a key range and
    as dense q-blocks), so it changes nothing here beyond the check that the prefix fits into the keys."""
    if not 0 <= int(prefix_rows) <= int(lk):
        raise ValueError(f"prefix_rows = {prefix_rows} is outside the {lk} key rows")
    mask = torch.zeros((int(lq), int(lk)), dtype=torch.bool)
    for i, blk in enumerate(table.tolist()):
        for a, b in blk:
            mask[Q_BLOCK * i:Q_BLOCK * (i + 1), KEY_TILE * max(a, 0):KEY_TILE * max(b, 0)] = True
    return mask


@dataclass
class WindowAttentionConfig:
    """`WanTransformer3DModel.enable_window_attention(config)` and `CogVideoXTransformer3DModel.enable_window_attention(config)`:
    one class serves both models (the CogVideoX model adds its text rows as `prefix_rows` when it builds the table).

    window_frames: every query sees its own latent frame +- this many neighbours.
    sink_frames: latent frames every query sees (negatives count from the end); `forward(id_frames=n)` adds the trailing n.
    skip_layers: blocks whose self-attention stays dense.
    timestep_range = (lo, hi): windows apply only while lo < t < hi, t read from `current_timestep_callback` once per forward
    (`lambda: pipe.current_timestep`); None: always.  With a range the pipeline's loop runs eagerly."""
    window_frames: int = 2
    sink_frames: Tuple[int, ...] = (0,)
    skip_layers: Tuple[int, ...] = ()
    timestep_range: Optional[Tuple[float, float]] = None
    current_timestep_callback: Optional[Callable[[], Any]] = None

    def __post_init__(self):
        if isinstance(self.window_frames, bool) or not isinstance(self.window_frames, int) or self.window_frames < 0:
            raise ValueError(f"window_frames = {self.window_frames!r}: a non-negative int is needed")
        try:
            self.sink_frames = tuple(int(s) for s in self.sink_frames)
            self.skip_layers = tuple(int(s) for s in self.skip_layers)
        except TypeError as e:
            raise ValueError(f"sink_frames / skip_layers must be sequences of ints: {e}") from None
        if any(s < 0 for s in self.skip_layers):
            raise ValueError(f"skip_layers = {self.skip_layers}: block indices are >= 0")
        if self.timestep_range is not None:
            try:
                lo, hi = (float(x) for x in self.timestep_range)
            except (TypeError, ValueError):
                raise ValueError(f"timestep_range = {self.timestep_range!r}: (lo, hi) is needed") from None
            if not lo < hi:
                raise ValueError(f"timestep_range = ({lo}, {hi}): lo < hi is needed")
            self.timestep_range = (lo, hi)
            if self.current_timestep_callback is None:
                raise ValueError("timestep_range needs `current_timestep_callback`: it returns the denoising loop's current "
                                 "timestep (`lambda: pipe.current_timestep`)")

    def key(self):
        """what a range table depends on"""
        return (self.window_frames, self.sink_frames)


def window_attention_runs_eagerly(transformer, use_hip_graph):
    """The pipelines' rule, checked before any work.  -> whether the denoising loop must run eagerly: with a timestep range the
    host decides per step whether the windows apply.  Off, or without a range (the table is a static device tensor), the step
    captures as it is."""
    if getattr(transformer, "is_sparse_calibrating", False):
        # a calibration run (frameino_amd/sparse_calibration.py) accumulates per-call statistics on the host's schedule
        if use_hip_graph is True:
            raise RuntimeError("use_hip_graph=True while the sparse attention is being calibrated: every self-attention call "
                               "runs the dense and the sparse kernels and adds to running sums, which one captured step "
                               "replayed cannot contain (the loop runs eagerly; use_hip_graph=None or False)")
        return True
    if not getattr(transformer, "window_attention_is_timestep_gated", False):
        return False
    if use_hip_graph is True:
        raise RuntimeError("use_hip_graph=True with window attention under a timestep range: whether a step's self-attention "
                           "is windowed changes from step to step on the host's schedule, which one captured step cannot "
                           "contain (the loop runs eagerly; use_hip_graph=None or False)")
    return True


@dataclass
class SparseAttentionConfig:
    """`WanTransformer3DModel.enable_sparse_attention(config)`: dynamic block-sparse self-attention.

    cdf_threshold: per (batch element, head, q-block) the kept key tiles carry at least this share of the softmax mass that
    the pooled predictor sees (`ops.attention_tile_plan`); >= 1: dense.
    window_frames, sink_frames: the tiles that are ALWAYS kept -- `frame_window_ranges(frames, tpf, window_frames, sinks)`, the
    own latent frame(s) +- window_frames neighbours and the sink frames (negatives count from the end; `forward(id_frames=n)`
    adds the trailing n).
    skip_layers: blocks whose self-attention stays dense.
    keep_masks: copy every layer's mask into `model.sparse_attention_masks[layer]` (tests, `sparse_attention_density()`).
    similarity_threshold: theta in (0, 1], or None (off).  A mean-pooled block predicts its tokens only
    when they resemble each other: a q-block whose mean pairwise cosine is below theta attends everything, such a key tile is
    always kept and takes no part in the predicted softmax.
    head_thresholds: layer -> one cdf threshold per head (each in (0, inf), >= 1: that head is dense), or None.  A layer that is
    not named uses `cdf_threshold`; a layer whose heads are all >= 1 takes the dense call.
    `frameino_amd.sparse_calibration.calibrate_sparse_attention` returns a config with this table filled."""
    cdf_threshold: float = 0.9
    window_frames: int = 0
    sink_frames: Tuple[int, ...] = (0,)
    skip_layers: Tuple[int, ...] = ()
    keep_masks: bool = False
    similarity_threshold: Optional[float] = None
    head_thresholds: Optional[Mapping[int, Sequence[float]]] = None

    def __post_init__(self):
        t = self.cdf_threshold
        if isinstance(t, bool) or not isinstance(t, (int, float)) or not (t > 0) or t == float("inf"):
            raise ValueError(f"cdf_threshold = {t!r}: a number in (0, inf) is needed (>= 1: dense)")
        self.cdf_threshold = float(t)
        if isinstance(self.window_frames, bool) or not isinstance(self.window_frames, int) or self.window_frames < 0:
            raise ValueError(f"window_frames = {self.window_frames!r}: a non-negative int is needed")
        try:
            self.sink_frames = tuple(int(s) for s in self.sink_frames)
            self.skip_layers = tuple(int(s) for s in self.skip_layers)
        except TypeError as e:
            raise ValueError(f"sink_frames / skip_layers must be sequences of ints: {e}") from None
        if any(s < 0 for s in self.skip_layers):
            raise ValueError(f"skip_layers = {self.skip_layers}: block indices are >= 0")
        self.keep_masks = bool(self.keep_masks)
        th = self.similarity_threshold
        if th is not None:
            if isinstance(th, bool) or not isinstance(th, (int, float)) or not 0 < th <= 1:
                raise ValueError(f"similarity_threshold = {th!r}: a number in (0, 1] is needed (None: off)")
            self.similarity_threshold = float(th)
        if self.head_thresholds is not None:
            if not isinstance(self.head_thresholds, Mapping):
                raise ValueError(f"head_thresholds = {self.head_thresholds!r}: a mapping layer -> thresholds per head is needed")
            table = {}
            for li, row in self.head_thresholds.items():
                if isinstance(li, bool) or not isinstance(li, int) or li < 0:
                    raise ValueError(f"head_thresholds: layer {li!r}: block indices are ints >= 0")
                try:
                    row = tuple(row)
                except TypeError:
                    raise ValueError(f"head_thresholds[{li}] = {row!r}: one threshold per head is needed") from None
                for t in row:
                    if isinstance(t, bool) or not isinstance(t, (int, float)) or not (t > 0) or t == float("inf"):
                        raise ValueError(f"head_thresholds[{li}]: {t!r}: numbers in (0, inf) are needed (>= 1: dense)")
                if not row:
                    raise ValueError(f"head_thresholds[{li}] is empty: one threshold per head is needed")
                table[li] = tuple(float(t) for t in row)
            self.head_thresholds = table

    def key(self):
        """what a forced-tile table depends on"""
        return (self.window_frames, self.sink_frames)

    def check_model(self, num_layers, num_heads):
        """what can be checked only against a model: the layers exist, every `head_thresholds` row has one entry per head"""
        if any(li >= num_layers for li in self.skip_layers):
            raise ValueError(f"skip_layers = {self.skip_layers}: this model has {num_layers} blocks")
        for li, row in (self.head_thresholds or {}).items():
            if li >= num_layers:
                raise ValueError(f"head_thresholds names layer {li}: this model has {num_layers} blocks")
            if len(row) != num_heads:
                raise ValueError(f"head_thresholds[{li}] has {len(row)} entries: this model has {num_heads} heads")


def tile_mask_words(lk):
    """uint32 words per q-block row of a tile mask over lk keys"""
    return (-(-int(lk) // KEY_TILE) + 31) // 32


def pack_tile_mask(keep):
    """bool [..., ntall] -> int32 [..., ceil(ntall / 32)]: bit t & 31 of word t >> 5 is tile t (the layout of `ops.attention_tiles`)"""
    keep = torch.as_tensor(keep, dtype=torch.bool)
    nt = keep.shape[-1]
    words = (nt + 31) // 32
    pad = torch.zeros(keep.shape[:-1] + (words * 32,), dtype=torch.int64)
    pad[..., :nt] = keep
    w = (pad.view(keep.shape[:-1] + (words, 32)) << torch.arange(32, dtype=torch.int64)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def unpack_tile_mask(mask, lk):
    """int32 / uint32 [..., words] -> bool [..., ceil(lk / 64)] (bits at or beyond the last tile dropped)"""
    ntall = -(-int(lk) // KEY_TILE)
    w = mask.detach().cpu().view(torch.int32).to(torch.int64) & 0xffffffff
    bits = (w.unsqueeze(-1) >> torch.arange(32, dtype=torch.int64)) & 1
    return bits.reshape(w.shape[:-1] + (-1,))[..., :ntall].bool()


class SelfAttentionOptionsMixin:
    """The self-attention switches of a DiT -- fp8 operands (`enable_fp8_attention`) and the sliding window over frames
    (`enable_window_attention`) -- with their state, and `_attend`, the one place that picks among `ops.attention`,
    `ops.attention_ranges`, `ops.attention_fp8` and `ops.attention_fp8_ranges`.  The model calls `_init_self_attention_options()`
    from its constructor, names the dict that holds its positional tables in `_window_table_cache` (the range tables are dropped
    with them), says in `_window_refusals(fp8, default_procs, shard=None)` what it does not combine with the windows, calls
    `_window_begin` once per forward and keeps its kernel front end in `self.ops`.  The sparse attention
    (`enable_sparse_attention`, `_sparse_begin` once per forward, `_attend(tiles=)`) is a fifth route beside the four."""
    _window_table_cache = None    # name of the model's dict of positional tables: `_window_begin` caches the range tables there
    _fp8_window_walk = False      # whether the model has an fp8 range walk at all; without one fp8 is refused while windows are on

    def _init_self_attention_options(self):
        self.fp8_attention = False        # see enable_fp8_attention
        self.fp8_p_mode = None
        self.fp8_smooth_k = False
        self.fp8_smooth_v = False
        self.fp8_smooth_q = False
        self._window = None               # WindowAttentionConfig or None: see enable_window_attention
        self._window_forwards = 0
        self.window_attention_log = []    # (forward index, timestep or None, windowed) since enable_window_attention
        self._sparse = None               # SparseAttentionConfig or None: see enable_sparse_attention
        self.sparse_attention_masks = {}  # layer -> that layer's last tile mask (device), with `keep_masks`
        self._sparse_mask_keys = {}       # layer -> the key count of that mask
        self._sparse_sims = {}            # layer -> (sim_q | sim_k of the last call (device), (b, heads, nqb, ntall)), gate + `keep_masks`
        self._sparse_calib = None         # a running calibration (frameino_amd/sparse_calibration.py), else None

    def _smooth_q_refusals(self, smooth_q, window, sparse):
        """smooth Q exists on the dense fp8 call alone: not on the fp8 range walk (window attention), not on the fp8 tile walk
        (sparse attention)"""
        if not smooth_q:
            return
        for on, what, walk in ((window, "window attention (enable_window_attention)", "fp8 range walk (fino_attn_fwd_fp8_ranges)"),
                               (sparse, "sparse attention (enable_sparse_attention)", "fp8 tile walk (fino_attn_fwd_fp8_tiles)")):
            if on:
                raise NotImplementedError(f"fp8 attention with smooth_q and {what}: the {walk} has no smooth Q; switch one of "
                                          f"them off first (enable_fp8_attention(smooth_q=False))")

    def enable_fp8_attention(self, enabled=True, p_mode=None, smooth_k=False, smooth_v=False, smooth_q=False):
        """The self-attention with fp8 (e4m3) matrix operands -- q, k, v and P on the block-scaled fp8 MFMA, softmax and
        accumulation fp32 (`ops.attention_fp8`; the model's class docstring says where it applies).  Opt-in, no reference counterpart.
        p_mode: "exp2" | "ramp" -- how a softmax weight becomes its e4m3 byte (ops.FP8_P_*; None = ops.FP8_P_DEFAULT).
        smooth_k: subtract the per-(batch element, head, channel) mean of K over the keys before K is quantised
        (fino_attn_fwd_fp8_smooth): invisible to the softmax, and a channel offset that all keys share (a to_k bias, norm_k
        weights, low-frequency RoPE channels) stops taking the mantissa bits.  Off by default.
        smooth_v: subtract the per-(batch element, head, channel) mean of V over the keys before V is quantised and add it back
        to the normalised output in fp32 (fino_attn_fwd_fp8_smoothed): exact, the softmax weights sum to one, and an offset that
        all keys of a channel share (attn1.to_v.bias, a DC component of the modulated input: V has no norm and no RoPE) stops
        taking the mantissa bits.  Off by default.
        smooth_q: subtract from every block of 256 consecutive query rows its per-(batch element, head, channel) mean before q is
        quantised and add qbar . k_key back to the logits in fp32 (fino_attn_fwd_fp8_smooth_q): exact, and an
        offset that neighbouring query rows share (norm_q weights, low-frequency RoPE channels) stops taking the mantissa bits.
        The dense call only: refused with window attention and with sparse attention, in either order.  The token-sharded forward
        keeps its bf16 attention.  Off by default."""
        if enabled:
            self._smooth_q_refusals(smooth_q, self._window is not None, self._sparse is not None)
        if enabled and getattr(self, "_step_cache_policy", None) is not None:
            self._cache_refusals(fp8=True)           # (a step cache that keeps K / V in the model dtype says so, once)
        if enabled and self._sparse is not None:
            self._sparse_refusals(True, self._default_processors(), getattr(self, "parallel", None))
        if enabled and self._window is not None and not self._fp8_window_walk:
            # (such a model's hook refuses fp8 whatever else holds; one with an fp8 walk decides per head_dim, in its forward)
            self._window_refusals(True, self._default_processors(), getattr(self, "parallel", None))
        self.fp8_attention = bool(enabled)
        self.fp8_p_mode = p_mode
        self.fp8_smooth_k = bool(smooth_k)
        self.fp8_smooth_v = bool(smooth_v)
        self.fp8_smooth_q = bool(smooth_q)
        return self

    def enable_window_attention(self, config):
        """Opt-in, approximate: in every block not in `config.skip_layers` a query attends its own latent frame +-
        `config.window_frames` neighbours plus the sink frames (`config.sink_frames`, and the trailing `forward(id_frames=n)`
        frames) instead of every token -- `ops.attention_ranges` (with fp8 attention, where the model has that walk,
        `ops.attention_fp8_ranges`) over a per-q-block table of key-tile ranges (the module docstring has the exact definition and
        the kernel's granularity; DESIGN.md sections 6f, 6g).  A window that covers the whole clip takes the dense call, bit for
        bit.  In a joint sequence (CogVideoX: the text rows in front of frame 0, `prefix_rows`) only the video queries are windowed: the
        prefix rows are keys every query sees and queries that see every key.  What the model does not combine with it (its class docstring) is refused here where it can be seen, else by the
        forward before anything is launched.  No reference counterpart."""
        if not isinstance(config, WindowAttentionConfig):
            raise TypeError(f"enable_window_attention takes a WindowAttentionConfig, got {type(config)}")
        if any(li >= self.config.num_layers for li in config.skip_layers):
            raise ValueError(f"skip_layers = {config.skip_layers}: this model has {self.config.num_layers} blocks")
        if self._sparse is not None:
            raise NotImplementedError("window attention (enable_window_attention) with sparse attention "
                                      "(enable_sparse_attention): switch one of them off first; the sparse attention's "
                                      "`window_frames` keeps a window of frames always")
        self._smooth_q_refusals(self.fp8_attention and self.fp8_smooth_q, True, False)
        self._window_refusals(self.fp8_attention, self._default_processors(), getattr(self, "parallel", None))
        self._window = config
        self._window_forwards = 0
        self.window_attention_log = []
        return self

    def disable_window_attention(self):
        self._window = None
        return self

    @property
    def is_window_attention_enabled(self):
        return self._window is not None

    @property
    def window_attention_is_timestep_gated(self):
        """on, and under a `timestep_range`: whether a forward is windowed is then decided on the host, forward by forward"""
        return self._window is not None and self._window.timestep_range is not None

    def _window_begin(self, frames, tokens_per_frame, prefix_rows, id_frames, dev):
        """This forward's window state, decided before anything is launched: None (off, or outside the timestep range), else
        `.table(q_rows)` -> the device range table of those query rows of the sequence [prefix_rows | frames], or None when it
        covers every key tile (the dense call) -- and `.skip`, the blocks that stay dense.  Reads the timestep callback ONCE and
        appends to `window_attention_log`."""
        cfg = self._window
        if cfg is None:
            return None
        id_frames = int(id_frames or 0)
        if not 0 <= id_frames < frames:
            raise ValueError(f"id_frames = {id_frames} of {frames} latent frames")
        t, on = None, True
        if cfg.timestep_range is not None:
            t = float(cfg.current_timestep_callback())
            on = cfg.timestep_range[0] < t < cfg.timestep_range[1]
        self.window_attention_log.append((self._window_forwards, t, on))
        self._window_forwards += 1
        if not on:
            return None
        sinks = tuple(cfg.sink_frames) + tuple(range(frames - id_frames, frames))
        L = prefix_rows + frames * tokens_per_frame
        cache = getattr(self, self._window_table_cache)
        # tests and tools read the keys by position (id_frames, q_rows), per model: a sequence without a prefix keeps the key
        # it has always had, without the component
        prefix = (prefix_rows,) if prefix_rows else ()

        def table(q_rows):
            key = ("window", frames, tokens_per_frame) + prefix + (cfg.key(), id_frames, tuple(q_rows), str(dev))
            if key not in cache:
                tab = frame_window_ranges(frames, tokens_per_frame, cfg.window_frames, sinks, q_rows, prefix_rows)
                cache[key] = None if ranges_cover_all(tab, L) else tab.to(dev)
            return cache[key]

        return SimpleNamespace(table=table, skip=frozenset(cfg.skip_layers))

    @staticmethod
    def _window_ranges(win, li, q_rows):
        """the range table of block li's self-attention over the query rows `q_rows`, or None (dense)"""
        return None if win is None or li in win.skip else win.table(q_rows)

    # ------------------------------------------------------------------ dynamic block-sparse attention
    def _sparse_refusals(self, fp8, default_procs, shard=None):
        what = "sparse attention (enable_sparse_attention)"
        if self._window is not None:
            raise NotImplementedError(f"{what} with window attention (enable_window_attention): switch one of them off first; "
                                      f"`SparseAttentionConfig.window_frames` keeps a window of frames always")
        if fp8 and self.config.attention_head_dim != 128:
            raise NotImplementedError(f"{what} with fp8 attention at head_dim {self.config.attention_head_dim}: the fp8 tile walk "
                                      f"(fino_attn_fwd_fp8_tiles) exists for head_dim 128 only; switch one of them off first "
                                      f"(disable_sparse_attention() / enable_fp8_attention(False))")
        self._cache_refusals(sparse=True)        # (a step cache that does not run beside it: the model's one statement)
        if shard is not None and getattr(shard, "active", True):
            raise NotImplementedError(f"{what} with a token-sharded plan: it runs on one GPU")
        if not default_procs:
            raise NotImplementedError(f"{what} with a user-installed attention processor: the tile masks are applied by the "
                                      f"built-in attention path only")

    def enable_sparse_attention(self, config):
        """Opt-in, approximate: in every block not in `config.skip_layers` each (batch element, head, 256-row q-block) attends
        only the 64-key tiles that a device-side predictor picks right before the call, from that call's q and k
        (`ops.attention_tile_plan`: mean-pooled q-blocks and key tiles, the smallest set of tiles by descending predicted
        softmax mass that reaches `config.cdf_threshold`), plus the always-kept tiles of `frame_window_ranges(frames, tpf,
        config.window_frames, sinks)` -- `ops.attention_tiles` over the mask (with fp8 attention, head_dim 128:
        `ops.attention_fp8_tiles` over the same mask, predicted from the bf16 / fp16 q and k).  `cdf_threshold >= 1`, or forced tiles that cover
        everything, take the dense call, bit for bit.  No timestep gate and no host read: the step captures as it is.  What does
        not combine with it (window attention, fp8 attention at a head_dim other than 128, Pyramid Attention Broadcast, a
        token-sharded plan, a user-installed processor) is refused here where it can be seen, else by the forward before anything is launched.  No
        reference counterpart; quality on real checkpoints is unmeasured.
        `config.similarity_threshold` and `config.head_thresholds` (both off by default): blocks whose tokens do
        not resemble each other are never predicted from, and every (layer, head) gets its own threshold -- a head at >= 1 keeps
        every tile, a layer whose heads are all >= 1 takes the dense call.  `head_thresholds` is checked against this model here."""
        if not isinstance(config, SparseAttentionConfig):
            raise TypeError(f"enable_sparse_attention takes a SparseAttentionConfig, got {type(config)}")
        config.check_model(self.config.num_layers, self.config.num_attention_heads)
        self._smooth_q_refusals(self.fp8_attention and self.fp8_smooth_q, False, True)
        self._sparse_refusals(self.fp8_attention, self._default_processors(), getattr(self, "parallel", None))
        self._sparse = config
        self.sparse_attention_masks, self._sparse_mask_keys, self._sparse_sims = {}, {}, {}
        return self

    def disable_sparse_attention(self):
        self._sparse = None
        self.sparse_attention_masks, self._sparse_mask_keys, self._sparse_sims = {}, {}, {}
        return self

    @property
    def is_sparse_calibrating(self):
        """inside `calibrate_sparse_attention`: every self-attention call runs dense and sparse and adds to running sums"""
        return getattr(self, "_sparse_calib", None) is not None

    @property
    def is_sparse_attention_enabled(self):
        return self._sparse is not None

    def sparse_attention_density(self):
        """layer -> fraction of the (batch element, head, q-block, key tile) entries the last forward kept (needs `keep_masks`;
        a host read)"""
        return {li: float(unpack_tile_mask(m, self._sparse_mask_keys[li]).float().mean())
                for li, m in sorted(self.sparse_attention_masks.items())}

    def sparse_attention_similarity(self):
        """layer -> (mean sim_q, mean sim_k, share of q-blocks under theta, share of key tiles under theta) of the last forward's
        last call of that layer (needs `similarity_threshold` and `keep_masks`; a host read)"""
        theta = getattr(self._sparse, "similarity_threshold", None) if self._sparse is not None else None
        out = {}
        for li, (sims, (b, heads, nqb, nt)) in sorted(self._sparse_sims.items()):
            s = sims.detach().float().cpu()
            sq, sk = s[:b * heads * nqb], s[b * heads * nqb:]
            out[li] = (float(sq.mean()), float(sk.mean()), float((sq < theta).float().mean()), float((sk < theta).float().mean()))
        return out

    def _sparse_begin(self, frames, tokens_per_frame, id_frames, dev, ws, batch, heads, head_dim):
        """This forward's sparse state, decided before anything is launched: None (off, or `cdf_threshold >= 1` without
        `head_thresholds`: dense), else `.keep(q_rows)` -> the device table of the always-kept tiles of those query rows, or None
        when it covers every key tile (the dense call); `.skip`; and the mask buffer and plan workspace, kept on the model
        workspace `ws` (allocated once per workspace: a captured step replays them).  With `head_thresholds`: `.cdf_heads(layer)`
        -> that layer's device table [heads] (None: the scalar) and `.dense`, the layers whose thresholds are all >= 1; with
        `similarity_threshold`: `.similarity`, and the workspace holds the similarities too."""
        cfg = self._sparse
        head_thr = getattr(cfg, "head_thresholds", None) or None
        theta = getattr(cfg, "similarity_threshold", None)
        if cfg is None or (cfg.cdf_threshold >= 1.0 and head_thr is None):
            return None
        id_frames = int(id_frames or 0)
        if not 0 <= id_frames < frames:
            raise ValueError(f"id_frames = {id_frames} of {frames} latent frames")
        sinks = tuple(cfg.sink_frames) + tuple(range(frames - id_frames, frames))
        L = frames * tokens_per_frame
        cache = getattr(self, self._window_table_cache)

        def keep(q_rows):
            key = ("sparse", frames, tokens_per_frame, cfg.key(), id_frames, tuple(q_rows), str(dev))
            if key not in cache:
                tab = frame_window_ranges(frames, tokens_per_frame, cfg.window_frames, sinks, q_rows)
                cache[key] = None if ranges_cover_all(tab, L) else tab.to(dev)
            return cache[key]

        words, nqb = tile_mask_words(L), -(-L // Q_BLOCK)
        need_mask = batch * heads * nqb * words
        plan_bytes = self.ops.attention_tile_plan_bytes if theta is None else self.ops.attention_tile_plan_gated_bytes
        need_plan = plan_bytes(batch, heads, L, L, head_dim) // 4
        if getattr(ws, "sparse_mask", None) is None or ws.sparse_mask.numel() < need_mask:
            ws.sparse_mask = torch.zeros(need_mask, dtype=torch.int32, device=dev)
        if getattr(ws, "sparse_plan", None) is None or ws.sparse_plan.numel() < need_plan:
            ws.sparse_plan = torch.empty(need_plan, dtype=torch.float32, device=dev)
        sp = SimpleNamespace(keep=keep, skip=frozenset(cfg.skip_layers), cdf=cfg.cdf_threshold, words=words, lk=L,
                             mask=ws.sparse_mask, workspace=ws.sparse_plan, keep_masks=cfg.keep_masks)
        if theta is not None:
            sp.similarity = theta
        if head_thr is not None:
            for li, row in head_thr.items():
                if len(row) != heads:
                    raise ValueError(f"head_thresholds[{li}] has {len(row)} entries: this forward has {heads} heads")
            named_dense = {li for li, row in head_thr.items() if min(row) >= 1.0}
            sp.dense = frozenset(named_dense if cfg.cdf_threshold < 1.0 else
                                 named_dense | (set(range(self.config.num_layers)) - set(head_thr)))

            def cdf_heads(li):
                row = head_thr.get(li)
                if row is None:
                    return None
                key = ("sparse_cdf", li, row, str(dev))
                if key not in cache:
                    cache[key] = torch.tensor(row, dtype=torch.float32).to(dev)
                return cache[key]

            sp.cdf_heads = cdf_heads
        return sp

    @staticmethod
    def _sparse_tiles(sp, li, q_rows):
        """what `_attend(tiles=)` takes for block li's self-attention over the query rows `q_rows`, or None (dense)"""
        if sp is None or li in sp.skip or li in getattr(sp, "dense", ()):
            return None
        table = sp.keep(q_rows)
        if table is None:
            return None
        tiles = SimpleNamespace(sp=sp, layer=li, keep=table)
        if getattr(sp, "cdf_heads", None) is not None:
            tiles.cdf_heads = sp.cdf_heads(li)
        return tiles

    def _attend_tiles(self, ops, q, k, v, heads, tiles, fp8=False, **kw):
        """the plan on this call's q and k, then the tile walk over its mask -- `fp8`: the fp8 walk with the model's fp8 options"""
        if getattr(self, "_sparse_calib", None) is not None:
            if fp8:          # (switched on inside the calibration's run(): calibrate_sparse_attention has refused any other)
                raise NotImplementedError("calibrate_sparse_attention with fp8 attention: thresholds are calibrated in "
                                          "bf16 / fp16 and loaded; enable_fp8_attention(False) first")
            return self._sparse_calib.attend(self, ops, q, k, v, heads, tiles, **kw)
        sp = tiles.sp
        b, nqb = q.shape[0], -(-q.shape[1] // Q_BLOCK)
        mask = sp.mask[:b * heads * nqb * sp.words].view(b, heads, nqb, sp.words)
        gate = {}                         # the safeguards of section 6k, named only when they are in use
        if getattr(tiles, "cdf_heads", None) is not None:
            gate["cdf_heads"] = tiles.cdf_heads
        theta = getattr(sp, "similarity", None)
        if theta is not None:
            gate["similarity_threshold"] = theta
        ops.attention_tile_plan(q, k, heads, sp.cdf, keep_ranges=tiles.keep, scale=kw.get("scale"), out=mask,
                                workspace=sp.workspace, **gate)
        if sp.keep_masks and theta is not None:
            # the similarities sit in the workspace behind the pooled means (ops.attention_tile_plan)
            nt = -(-k.shape[1] // KEY_TILE)
            n, at = b * heads * (nqb + nt), b * heads * (nqb + nt) * (q.shape[2] // heads)
            old = self._sparse_sims.get(tiles.layer)
            sims = old[0] if old is not None and old[0].numel() == n else torch.empty(n, dtype=torch.float32,
                                                                                     device=sp.workspace.device)
            sims.copy_(sp.workspace[at:at + n])
            self._sparse_sims[tiles.layer] = (sims, (b, heads, nqb, nt))
        if sp.keep_masks:
            old = self.sparse_attention_masks.get(tiles.layer)
            if old is None or old.shape != mask.shape:
                old = self.sparse_attention_masks[tiles.layer] = torch.empty_like(mask)
            old.copy_(mask)
            self._sparse_mask_keys[tiles.layer] = k.shape[1]
        if fp8:
            return ops.attention_fp8_tiles(q, k, v, heads, mask, p_mode=self.fp8_p_mode, smooth_k=self.fp8_smooth_k,
                                           smooth_v=self.fp8_smooth_v, **kw)
        return ops.attention_tiles(q, k, v, heads, mask, **kw)

    def _attend(self, ops, q, k, v, heads, *, fp8, ranges=None, tiles=None, **kw):
        """one self-attention call: dense or over `ranges`, bf16 / fp16 or -- `fp8` -- with the model's fp8 options; `kw`: out=,
        scale=.  `tiles` (`_sparse_tiles`): the dynamic tile walk instead (with `fp8`: head_dim 128 only, `_sparse_refusals`)."""
        if fp8 and self.fp8_smooth_q:
            # (the enable_* calls have refused these; a walk reached some other way is refused before it launches)
            self._smooth_q_refusals(True, ranges is not None, tiles is not None)
        if tiles is not None:
            return self._attend_tiles(ops, q, k, v, heads, tiles, fp8=fp8, **kw)
        if fp8:
            kw.update(p_mode=self.fp8_p_mode, smooth_k=self.fp8_smooth_k, smooth_v=self.fp8_smooth_v)
            if self.fp8_smooth_q:
                kw.update(smooth_q=True)             # the dense route alone (ranges is None here)
        if ranges is None:
            return (ops.attention_fp8 if fp8 else ops.attention)(q, k, v, heads, **kw)
        return (ops.attention_fp8_ranges if fp8 else ops.attention_ranges)(q, k, v, heads, ranges, **kw)
