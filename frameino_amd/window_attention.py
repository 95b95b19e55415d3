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
exactly what the kernel computes.  Pure Python + CPU torch: nothing here touches a GPU."""
from dataclasses import dataclass
from typing import Any, Callable, Optional, Tuple

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
