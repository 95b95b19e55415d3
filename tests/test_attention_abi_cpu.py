"""Error contract of the attention entry points, on the CPU: every forward entry point plus fino_attn_partial and fino_attn_merge
is called with bad arguments and must answer with the recorded return code and message (validation runs before any launch,
tests/test_lib_abi.py).  The expected (rc, message behind the "name:" prefix) were recorded from the library before the host
paths of the three attention translation units were folded into shared helpers; the prefix itself is free to name the real
entry point."""
import ctypes
import os
import re

import pytest

from frameino_amd import _lib

PTR = 4096                       # a non-null, 16-byte aligned "device pointer": no case gets as far as a launch
ARG, UNSUPPORTED = -1, -3
BF16_ENTRIES = ("fino_attn_fwd", "fino_attn_fwd_ws", "fino_attn_fwd_ranges", "fino_attn_fwd_tiles", "fino_attn_fwd_tail")
FP8_ENTRIES = ("fino_attn_fwd_fp8", "fino_attn_fwd_fp8_smooth", "fino_attn_fwd_fp8_smoothed", "fino_attn_fwd_fp8_ranges",
               "fino_attn_fwd_fp8_tiles")
_LK_B = (ctypes.c_int * 4)(100, 100, 100, 100)            # fino_attn_fwd_tail reads these two on the host
_MULT = (ctypes.c_float * 4)(2.0, 2.0, 2.0, 2.0)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _defaults(entry):
    """a call that would pass validation; the cases below break it"""
    d = dict(q=PTR, k=PTR, v=PTR, o=PTR, batch=1, heads=2, lq=256, lk=128, head_dim=128, scale=0.125, dtype=0, stream=0)
    for t in "qkvo":
        d.update({t + "_bs": 65536, t + "_rs": 256, t + "_hs": 128})
    d.update(ws=0, ws_bytes=0, ranges=PTR, mask=PTR, mask_bs=0, mask_hs=0, words=1, lk_b=_LK_B, tail_mult=_MULT,
             p_mode=0, kv_ws=PTR, kv_ws_bytes=1 << 40, smooth=0, part0=PTR, part1=0, part2=0)
    if entry == "fino_attn_fwd_fp8_ranges":
        d["head_dim"] = 64
    if entry == "fino_attn_partial":
        d.update(ws=PTR, ws_bytes=1 << 40)
    return d


def _args(entry, d):
    f = ctypes.c_float(d["scale"])
    shape = [d["batch"], d["heads"], d["lq"], d["lk"], d["head_dim"]]
    if entry == "fino_attn_merge":
        return [d["o"], d["batch"], d["heads"], d["lq"], d["head_dim"], d["o_bs"], d["o_rs"], d["o_hs"], d["part0"], d["part1"],
                d["part2"], d["dtype"], d["stream"]]
    if entry == "fino_attn_partial":
        return [d["q"], d["k"], d["v"]] + shape + [d[t + s] for t in "qkv" for s in ("_bs", "_rs", "_hs")] + \
               [f, d["dtype"], d["ws"], d["ws_bytes"], d["stream"]]
    if entry in BF16_ENTRIES:
        lead = [d["q"], d["k"], d["v"], d["o"]] + shape + [d[t + s] for t in "qkvo" for s in ("_bs", "_rs", "_hs")] + [f, d["dtype"]]
        tail = {"fino_attn_fwd": [], "fino_attn_fwd_ws": [d["ws"], d["ws_bytes"]], "fino_attn_fwd_ranges": [d["ranges"]],
                "fino_attn_fwd_tiles": [d["mask"], d["mask_bs"], d["mask_hs"], d["words"]],
                "fino_attn_fwd_tail": [d["lk_b"], d["tail_mult"]]}[entry]
        return lead + tail + [d["stream"]]
    lead = [d["q"], d["k"], d["v"], d["o"]] + shape + [d[t + s] for t in "qkvo" for s in ("_bs", "_rs")] + \
           [f, d["dtype"], d["p_mode"], d["kv_ws"], d["kv_ws_bytes"]]
    return lead + {"fino_attn_fwd_fp8": [d["stream"]], "fino_attn_fwd_fp8_smooth": [d["stream"]],
                   "fino_attn_fwd_fp8_smoothed": [d["stream"], d["smooth"]],
                   "fino_attn_fwd_fp8_ranges": [d["smooth"], d["ranges"], d["stream"]],
                   "fino_attn_fwd_fp8_tiles": [d["smooth"], d["mask"], d["mask_bs"], d["mask_hs"], d["words"], d["stream"]]}[entry]


def _call(lib, entry, changes):
    d = _defaults(entry)
    assert set(changes) <= set(d), changes
    d.update(changes)
    args = [ctypes.cast(a, ctypes.c_void_p) if isinstance(a, ctypes.Array) else a for a in _args(entry, d)]
    rc = getattr(lib, entry)(*args)
    return rc, re.sub(r"^[a-z0-9_]+: ", "", lib.fino_last_error().decode())


ALIGN = "pointers and strides must be 16-byte aligned"
SCALE = "scale must be > 0 (or FINO_ATTN_SCALE_FOLDED)"
HD_BF16 = "head_dim 96 not in {64,128}"
HD_FP8 = "head_dim 96 not in {64, 128}"
RANGE64 = "head_dim 128: the range walk exists for head_dim 64 only"
TILE128 = "head_dim 64: the fp8 tile walk exists for head_dim 128 only"
TAIL = "needs head_dim 128, batch <= 4, lk > 64 (got head_dim %d, batch %d, lk %d)"

# (entry point, what is wrong with the call, rc, message behind the prefix)
CASES = []
for _e in BF16_ENTRIES[:4]:
    CASES += [
        (_e, dict(head_dim=96), UNSUPPORTED, HD_BF16),
        (_e, dict(dtype=7), ARG, "dtype 7"),
        (_e, dict(k=0), ARG, "null pointer"),
        (_e, dict(o=0), ARG, "null pointer"),
        (_e, dict(batch=0), ARG, "bad shape B=0 H=2 Lq=256 Lk=128"),
        (_e, dict(lk=0), ARG, "bad shape B=1 H=2 Lq=256 Lk=0") if _e != "fino_attn_fwd_tiles" else
        (_e, dict(lk=0), UNSUPPORTED, "Lk=0 is more than 1024 key tiles"),
        (_e, dict(lq=(1 << 31) - 256), ARG, "sequence too long"),
        (_e, dict(v=PTR + 8), ARG, ALIGN),
        (_e, dict(k_rs=260), ARG, ALIGN),
        (_e, dict(o_hs=4), ARG, ALIGN),
        (_e, dict(q_bs=12), ARG, ALIGN),
        (_e, dict(scale=0.0), ARG, SCALE),
        (_e, dict(scale=-0.5), ARG, SCALE),
        (_e, dict(lk=1 << 20, k_rs=2048), UNSUPPORTED, "Lk=1048576 keys x row stride 2048 exceed the 2 GiB one (batch, head) K/V slice "
                                                       "may span") if _e != "fino_attn_fwd_tiles" else
        (_e, dict(lk=1 << 20, k_rs=2048), UNSUPPORTED, "Lk=1048576 is more than 1024 key tiles"),
        # two faults at once: the order of the checks
        (_e, dict(dtype=7, head_dim=96), ARG, "dtype 7"),
        (_e, dict(q=0, head_dim=96), ARG, "null pointer"),
        (_e, dict(head_dim=96, q_rs=4), UNSUPPORTED, HD_BF16),
        (_e, dict(k=PTR + 2, scale=0.0), ARG, ALIGN),
    ]
CASES += [
    ("fino_attn_fwd_ws", dict(ws=24, ws_bytes=1024), ARG, "workspace must be 16-byte aligned"),
    ("fino_attn_fwd_ws", dict(ws=24, ws_bytes=1024, scale=0.0), ARG, SCALE),
    ("fino_attn_fwd_ranges", dict(ranges=0), ARG, "null ranges table"),
    ("fino_attn_fwd_ranges", dict(ranges=PTR + 2), ARG, "the ranges table must be 4-byte aligned"),
    ("fino_attn_fwd_ranges", dict(ranges=0, dtype=7), ARG, "null ranges table"),
    ("fino_attn_fwd_tiles", dict(mask=0), ARG, "null mask"),
    ("fino_attn_fwd_tiles", dict(mask=PTR + 1), ARG, "the mask must be 4-byte aligned"),
    ("fino_attn_fwd_tiles", dict(lk=64 * 33), ARG, "1 mask words per q-block do not hold 33 key tiles"),
    ("fino_attn_fwd_tiles", dict(words=0), ARG, "0 mask words per q-block do not hold 2 key tiles"),
    ("fino_attn_fwd_tiles", dict(lk=64 * 1024 + 1, words=64), UNSUPPORTED, "Lk=65537 is more than 1024 key tiles"),
    ("fino_attn_fwd_tiles", dict(mask_hs=-1), ARG, "negative mask stride"),
    ("fino_attn_fwd_tiles", dict(mask=0, dtype=7), ARG, "null mask"),
    ("fino_attn_fwd_tiles", dict(words=0, head_dim=96), ARG, "0 mask words per q-block do not hold 2 key tiles"),
    # the tail form: its own shape rule, then the shared operand checks
    ("fino_attn_fwd_tail", dict(dtype=7), ARG, "dtype 7"),
    ("fino_attn_fwd_tail", dict(v=0), ARG, "null pointer"),
    ("fino_attn_fwd_tail", dict(lk_b=0), ARG, "null pointer"),
    ("fino_attn_fwd_tail", dict(tail_mult=0), ARG, "null pointer"),
    ("fino_attn_fwd_tail", dict(head_dim=96), UNSUPPORTED, TAIL % (96, 1, 128)),
    ("fino_attn_fwd_tail", dict(head_dim=64), UNSUPPORTED, TAIL % (64, 1, 128)),
    ("fino_attn_fwd_tail", dict(batch=5), UNSUPPORTED, TAIL % (128, 5, 128)),
    ("fino_attn_fwd_tail", dict(lk=64), UNSUPPORTED, TAIL % (128, 1, 64)),
    ("fino_attn_fwd_tail", dict(lk=40), UNSUPPORTED, TAIL % (128, 1, 40)),
    ("fino_attn_fwd_tail", dict(q=PTR + 4), ARG, ALIGN),
    ("fino_attn_fwd_tail", dict(v_rs=12), ARG, ALIGN),
    ("fino_attn_fwd_tail", dict(scale=0.0), ARG, "scale"),
    ("fino_attn_fwd_tail", dict(lk=1 << 19, k_rs=4096), UNSUPPORTED, "an operand spans more than 2 GiB"),
    ("fino_attn_fwd_tail", dict(lk=96), ARG, "lk_b[0] = 100 (of 96), tail_mult 2"),
    ("fino_attn_fwd_tail", dict(batch=5, q=0), ARG, "null pointer"),
    ("fino_attn_fwd_tail", dict(batch=5, q_rs=4), UNSUPPORTED, TAIL % (128, 5, 128)),
    ("fino_attn_fwd_tail", dict(q_rs=4, scale=0.0), ARG, ALIGN),
    # partials and their merge
    ("fino_attn_partial", dict(head_dim=96), UNSUPPORTED, "head_dim 96"),
    ("fino_attn_partial", dict(dtype=7), ARG, "dtype 7"),
    ("fino_attn_partial", dict(ws=0), ARG, "workspace of 270336 bytes needed"),
    ("fino_attn_partial", dict(ws_bytes=270335), ARG, "workspace of 270336 bytes needed"),
    ("fino_attn_partial", dict(head_dim=64, ws_bytes=1000), ARG, "workspace of 139264 bytes needed"),
    ("fino_attn_partial", dict(q=0), ARG, "null pointer"),
    ("fino_attn_partial", dict(k=PTR + 8), ARG, ALIGN),
    ("fino_attn_partial", dict(v_hs=4), ARG, ALIGN),
    ("fino_attn_partial", dict(scale=0.0), ARG, SCALE),
    ("fino_attn_partial", dict(ws=PTR + 8), ARG, "workspace must be 16-byte aligned"),
    ("fino_attn_partial", dict(ws_bytes=0, q=0), ARG, "workspace of 270336 bytes needed"),
    ("fino_attn_partial", dict(dtype=7, ws_bytes=0), ARG, "dtype 7"),
    ("fino_attn_merge", dict(dtype=7), ARG, "dtype 7"),
    ("fino_attn_merge", dict(o=0), ARG, "bad arguments"),
    ("fino_attn_merge", dict(part0=0), ARG, "bad arguments"),
    ("fino_attn_merge", dict(head_dim=96), ARG, "bad arguments"),
    ("fino_attn_merge", dict(lq=0), ARG, "bad arguments"),
    ("fino_attn_merge", dict(o=PTR + 8), ARG, "output must be 16-byte aligned"),
    ("fino_attn_merge", dict(o_rs=4), ARG, "output must be 16-byte aligned"),
    ("fino_attn_merge", dict(part2=PTR), ARG, "part2 without part1"),
    ("fino_attn_merge", dict(dtype=7, o=0), ARG, "dtype 7"),
]
for _e in FP8_ENTRIES:
    _hd = 64 if _e == "fino_attn_fwd_fp8_ranges" else 128
    # fino_attn_fp8_kv_bytes(1, 2, 128, head_dim); fino_attn_fwd_fp8_smooth adds the key mean and its partials
    _need = 69275648 if _e == "fino_attn_fwd_fp8_smooth" else {64: 33792, 128: 69273600}[_hd]
    CASES += [
        (_e, dict(head_dim=96), UNSUPPORTED, HD_FP8) if _e != "fino_attn_fwd_fp8_tiles" else
        (_e, dict(head_dim=96), UNSUPPORTED, "head_dim 96: the fp8 tile walk exists for head_dim 128 only"),
        (_e, dict(dtype=7), ARG, "dtype 7"),
        (_e, dict(p_mode=2), ARG, "p_mode 2"),
        (_e, dict(q=0), ARG, "null pointer"),
        (_e, dict(kv_ws=0), ARG, "null pointer"),
        (_e, dict(heads=0), ARG, "bad shape"),
        (_e, dict(o=PTR + 8), ARG, ALIGN),
        (_e, dict(kv_ws=PTR + 8), ARG, ALIGN),
        (_e, dict(v_rs=4), ARG, ALIGN),
        (_e, dict(q_bs=12), ARG, ALIGN),
        (_e, dict(scale=0.0), ARG, "scale"),
        (_e, dict(kv_ws_bytes=1000), ARG, "workspace 1000 B < %d B" % _need),
        (_e, dict(dtype=7, p_mode=2), ARG, "p_mode 2"),
        (_e, dict(dtype=7, q=0), ARG, "dtype 7"),
        (_e, dict(q=0, batch=0), ARG, "null pointer"),
        (_e, dict(v_rs=4, scale=0.0), ARG, ALIGN),
        (_e, dict(scale=0.0, kv_ws_bytes=1000), ARG, "scale"),
    ]
CASES += [
    ("fino_attn_fwd_fp8_smoothed", dict(smooth=4), ARG, "smooth flags 4 not in 0 .. 3"),
    ("fino_attn_fwd_fp8_smoothed", dict(smooth=-1, p_mode=2), ARG, "smooth flags -1 not in 0 .. 3"),
    ("fino_attn_fwd_fp8_smoothed", dict(smooth=3, kv_ws_bytes=1000), ARG, "workspace 1000 B < 69277696 B"),
    ("fino_attn_fwd_fp8_ranges", dict(head_dim=128), UNSUPPORTED, RANGE64),
    ("fino_attn_fwd_fp8_ranges", dict(ranges=0), ARG, "null ranges table"),
    ("fino_attn_fwd_fp8_ranges", dict(ranges=PTR + 2), ARG, "the ranges table must be 4-byte aligned"),
    ("fino_attn_fwd_fp8_ranges", dict(ranges=0, head_dim=128), ARG, "null ranges table"),
    ("fino_attn_fwd_fp8_ranges", dict(head_dim=128, q=0), UNSUPPORTED, RANGE64),
    ("fino_attn_fwd_fp8_tiles", dict(head_dim=64), UNSUPPORTED, TILE128),
    ("fino_attn_fwd_fp8_tiles", dict(mask=0), ARG, "null mask"),
    ("fino_attn_fwd_fp8_tiles", dict(mask=PTR + 2), ARG, "the mask must be 4-byte aligned"),
    ("fino_attn_fwd_fp8_tiles", dict(lk=64 * 33), ARG, "1 mask words per q-block do not hold 33 key tiles"),
    ("fino_attn_fwd_fp8_tiles", dict(lk=64 * 1024 + 1, words=64), UNSUPPORTED, "Lk=65537 is more than 1024 key tiles"),
    ("fino_attn_fwd_fp8_tiles", dict(mask_bs=-8), ARG, "negative mask stride"),
    ("fino_attn_fwd_fp8_tiles", dict(smooth=4), ARG, "smooth flags 4 not in 0 .. 3"),
    ("fino_attn_fwd_fp8_tiles", dict(head_dim=64, mask=0), UNSUPPORTED, TILE128),
    ("fino_attn_fwd_fp8_tiles", dict(mask=0, dtype=7), ARG, "null mask"),
    ("fino_attn_fwd_fp8_tiles", dict(words=0, q=0), ARG, "0 mask words per q-block do not hold 2 key tiles"),
]


@pytest.mark.parametrize("entry,changes,rc,message", CASES,
                         ids=["%s-%s" % (c[0], "+".join("%s=%s" % (k, getattr(v, "_length_", v)) for k, v in c[1].items()))
                              for c in CASES])
def test_bad_arguments_keep_their_return_code_and_message(lib, entry, changes, rc, message):
    got_rc, got = _call(lib, entry, changes)
    assert (got_rc, got) == (rc, message)


def test_every_entry_point_of_the_table_is_covered():
    assert {c[0] for c in CASES} == set(BF16_ENTRIES) | set(FP8_ENTRIES) | {"fino_attn_partial", "fino_attn_merge"}


def test_supported_predicates_share_one_shape_rule(lib):
    """the four *_supported() answers, on shapes at the edges of the rule they share"""
    big_q, big_k = (1 << 31) - 256, (1 << 31) - 64
    shapes = [(1, 1, 1, 1), (0, 1, 8, 8), (1, 0, 8, 8), (1, 1, 0, 8), (1, 1, 8, 0), (2, 3, big_q - 1, 64), (2, 3, big_q, 64),
              (2, 3, 64, big_k - 1), (2, 3, 64, big_k), (1, 1, 256, 65536), (1, 1, 256, 65537)]
    for b, h, lq, lk in shapes:
        ok = b > 0 and h > 0 and 0 < lq < big_q and 0 < lk < big_k
        few = (lk + 63) // 64 <= 1024
        for hd in (64, 128, 96):
            got = (lib.fino_attn_ranges_supported(b, h, lq, lk, hd), lib.fino_attn_tiles_supported(b, h, lq, lk, hd),
                   lib.fino_attn_fp8_ranges_supported(b, h, lq, lk, hd), lib.fino_attn_fp8_tiles_supported(b, h, lq, lk, hd))
            want = (int(ok and hd in (64, 128)), int(ok and hd in (64, 128) and few), int(ok and hd == 64),
                    int(ok and hd == 128 and few))
            assert got == want, (b, h, lq, lk, hd)
