"""Error contract of the GEMM family, on the CPU: every entry point of fino_gemm.hip, fino_gemm_fp8.hip and fino_gemm_fp6.hip is
called with arguments that break each of its checks in turn and must answer with the recorded return code and message
(validation runs before any launch, tests/test_lib_abi.py).  The expected (rc, message) were recorded from the library before
the host halves of the three translation units were folded into shared dispatchers and one parameter fill.  Among the cases are
the ones refused AFTER validation but before a launch (the fp32 epilogues with a ragged K, fino_conv3d_split with
c_out_pad % 32 != 0, the reciprocal range of the K-blocked A) and M = 0, which returns FINO_OK without a launch."""
import ctypes
import os

import pytest

from frameino_amd import _lib

PTR = 4096                       # a non-null, 16-byte aligned "device pointer": no case gets as far as a launch
OK, ARG, UNSUPPORTED = 0, -1, -3

_GEMM = ["a", "w", "bias", "c", "m", "n", "k", "lda", "ldw", "ldc", "epilogue", "r", "ldr", "gate", "mod_stride", "sel", "dtype"]
_CONV_GEO = ["t_out", "h_out", "w_out", "c_out_pad", "kt", "kh", "kw", "st", "sh", "sw", "pt", "ph", "pw", "up", "epilogue", "r",
             "zero_page"]
_MX = ["a", "sa", "w", "sw", "bias", "c", "m", "n", "k", "ldc", "epilogue", "r", "ldr", "gate", "mod_stride", "sel", "dtype"]
_QUANT = ["a", "c", "cs", "rows", "cols", "ldx", "dtype"]
ORDER = {
    "fino_gemm": _GEMM + ["stream"],
    "fino_gemm_split_n": _GEMM + ["c2", "ldc2", "n_split", "tile_m", "stream"],
    "fino_gemm_keep": _GEMM + ["keep", "ldk", "tile_m", "stream"],
    "fino_gemm_blocked_a": ["a", "w", "bias", "c", "m", "n", "k", "a_block_k", "a_block_stride", "a_groups", "a_group_stride", "lda",
                            "ldw", "ldc", "r", "ldr", "gate", "mod_stride", "sel", "dtype", "tile_m", "stream"],
    "fino_conv3d": ["a", "w", "bias", "c", "t_in", "h_in", "w_in", "c_in_pad"] + _CONV_GEO + ["dtype", "stream"],
    "fino_conv3d_split": ["a", "w", "bias", "c", "t_in", "h_in", "w_in", "c_in_pad", "planes"] + _CONV_GEO + ["stream"],
    "fino_skinny_linear": ["a", "w", "bias", "c", "m", "n", "k", "dtype", "silu", "stream"],
    "fino_gemm_mxfp8": _MX + ["stream"],
    "fino_gemm_mxfp8_keep": _MX + ["keep", "ldk", "stream"],
    "fino_gemm_mxfp8_q": ["a", "sa", "w", "sw", "bias", "c", "cs", "m", "n", "k", "epilogue", "dtype", "stream"],
    "fino_gemm_mxfp6": _MX + ["stream"],
    "fino_gemm_mxfp6_keep": _MX + ["keep", "ldk", "stream"],
    "fino_quantize_mxfp8": _QUANT + ["stream"],
    "fino_quantize_mxfp6": _QUANT + ["stream"],
    "fino_quantize_mxfp6_rot": _QUANT + ["mode", "stream"],
}
KEEPS = ("fino_gemm_keep", "fino_gemm_mxfp8_keep", "fino_gemm_mxfp6_keep")
MXS = ("fino_gemm_mxfp8", "fino_gemm_mxfp8_keep", "fino_gemm_mxfp6", "fino_gemm_mxfp6_keep")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _defaults(entry):
    """a call that would pass validation (and launch); every case below breaks it or makes it empty"""
    d = dict(a=PTR, w=PTR, bias=0, c=PTR, m=256, n=256, k=128, lda=128, ldw=128, ldc=256, epilogue=0, r=0, ldr=0, gate=0,
             mod_stride=0, sel=0, dtype=0, stream=0, c2=0, ldc2=0, n_split=0, tile_m=0, keep=PTR, ldk=256, sa=PTR, sw=PTR, cs=PTR,
             rows=16, cols=128, ldx=128, mode=1, silu=0)
    if entry in KEEPS:
        d.update(epilogue=2, r=PTR, ldr=256)
    if entry == "fino_gemm_blocked_a":
        d.update(r=PTR, ldr=256, gate=PTR, a_block_k=64, a_block_stride=64 * 256, a_groups=1, a_group_stride=0, lda=64)
    if entry.startswith("fino_conv3d"):
        d.update(t_in=4, h_in=4, w_in=4, c_in_pad=64, t_out=4, h_out=4, w_out=4, c_out_pad=64, kt=3, kh=3, kw=3, st=1, sh=1, sw=1,
                 pt=1, ph=1, pw=1, up=0, zero_page=PTR, planes=2)
    if entry == "fino_skinny_linear":
        d.update(m=2, n=8, k=8, dtype=-1)
    return d


def _call(lib, entry, changes):
    d = _defaults(entry)
    assert changes and set(changes) <= set(d), changes
    d.update(changes)
    rc =getattr(lib, entry)(*[d[name] for name in ORDER[entry]])
    return rc, lib.fino_last_error().decode() if rc else None


SPLIT = ("fino_gemm_split_n: needs c2, 0 < n_split < N a multiple of 256, ldc2 >= N - n_split, K % 64 == 0, no residual "
         "epilogue")
SPLIT_OK = dict(n=512, ldc=512, c2=PTR, ldc2=256, n_split=256)
LD = "fino_gemm: leading dimensions must be multiples of 8 and cover the row"
F32_ARGS = "fino_gemm: the fp32-output epilogues take one output, the planned tiling and a 16-byte aligned fp32 bias"
F32_ROUTE = "fino_gemm: the fp32-output epilogues need K % 64 == 0, 16-byte aligned operands and operands < 2 GiB"
KEEP = "%s: needs a 16-byte aligned keep buffer with ldk >= N a multiple of 8"
KEEP_EPI = "%s: epilogue %d (the residual epilogues 2, 3 and 4 keep y)"
GATED = dict(epilogue=3, r=PTR, ldr=256, gate=PTR)
BA = "fino_gemm_blocked_a: "
CONV_SPAN = ("fino_conv3d_split: a 256-row tile's input span (81920 bytes) exceeds the 2 GiB the gather offsets cover, or "
             "c_out_pad % 32 != 0 -- run the layer in chunks of fewer frames")

# (entry point, what is wrong with the call, rc, message)
CASES = []
for _e in ("fino_gemm", "fino_gemm_split_n", "fino_gemm_keep"):
    _who = "fino_gemm_keep" if _e == "fino_gemm_keep" else "fino_gemm"
    CASES += [
        (_e, dict(dtype=7), ARG, _who + ": dtype 7"),
        (_e, dict(a=0), ARG, "fino_gemm: null pointer"),
        (_e, dict(w=0), ARG, "fino_gemm: null pointer"),
        (_e, dict(c=0), ARG, "fino_gemm: null pointer"),
        (_e, dict(m=-1), ARG, "fino_gemm: bad shape M=-1 N=256 K=128"),
        (_e, dict(n=0), ARG, "fino_gemm: bad shape M=256 N=0 K=128"),
        (_e, dict(k=0), ARG, "fino_gemm: bad shape M=256 N=256 K=0"),
        (_e, dict(n=12), ARG, "fino_gemm: N=12 and K=128 must be multiples of 8"),
        (_e, dict(k=12), ARG, "fino_gemm: N=256 and K=12 must be multiples of 8"),
        (_e, dict(lda=100), ARG, LD),
        (_e, dict(lda=64), ARG, LD),
        (_e, dict(ldw=120), ARG, LD),
        (_e, dict(ldc=128), ARG, LD),
        (_e, dict(a=PTR + 8), ARG, "fino_gemm: A/W/C must be 16-byte aligned"),
        (_e, dict(c=PTR + 2), ARG, "fino_gemm: A/W/C must be 16-byte aligned"),
        (_e, dict(m=0), OK, None),
        # two faults at once: the order of the checks
        (_e, dict(dtype=7, a=0), ARG, _who + ": dtype 7"),
        (_e, dict(a=0, n=12), ARG, "fino_gemm: null pointer"),
        (_e, dict(m=-1, lda=100), ARG, "fino_gemm: bad shape M=-1 N=256 K=128"),
        (_e, dict(k=12, a=PTR + 8), ARG, "fino_gemm: N=256 and K=12 must be multiples of 8"),
        (_e, dict(lda=100, w=PTR + 4), ARG, LD),
        (_e, dict(m=0, a=PTR + 8), ARG, "fino_gemm: A/W/C must be 16-byte aligned"),
    ]
for _e in ("fino_gemm", "fino_gemm_split_n"):
    CASES += [
        (_e, dict(epilogue=7), ARG, "fino_gemm: epilogue 7"),
        (_e, dict(epilogue=-1), ARG, "fino_gemm: epilogue -1"),
        (_e, dict(epilogue=2), ARG, "fino_gemm: residual operand"),
        (_e, dict(epilogue=2, r=PTR, ldr=128), ARG, "fino_gemm: residual operand"),
        (_e, dict(epilogue=4, r=PTR + 8, ldr=256), ARG, "fino_gemm: residual operand"),
        (_e, dict(epilogue=6), ARG, "fino_gemm: residual operand"),
        (_e, dict(GATED, gate=0), ARG, "fino_gemm: gate operand"),
        (_e, dict(GATED, mod_stride=2), ARG, "fino_gemm: gate operand"),
        (_e, dict(GATED, epilogue=4, gate=PTR + 4), ARG, "fino_gemm: gate operand"),
        (_e, dict(GATED, m=0), OK, None),
        (_e, dict(epilogue=5, bias=PTR + 4), ARG, F32_ARGS),
        (_e, dict(epilogue=5, m=0), OK, None),
        # refused behind the validation, in front of the launch
        (_e, dict(epilogue=5, k=72, lda=72, ldw=72), UNSUPPORTED, F32_ROUTE),
        (_e, dict(epilogue=6, r=PTR, ldr=256, k=8, lda=8, ldw=8), UNSUPPORTED, F32_ROUTE),
        (_e, dict(epilogue=5, m=1 << 24), UNSUPPORTED, F32_ROUTE),
        (_e, dict(epilogue=5, n=1 << 24, ldc=1 << 24), UNSUPPORTED, F32_ROUTE),
        (_e, dict(epilogue=7, r=PTR + 8), ARG, "fino_gemm: epilogue 7"),
        (_e, dict(epilogue=3, gate=0), ARG, "fino_gemm: residual operand"),
    ]
for _e in ("fino_gemm_split_n", "fino_gemm_keep"):
    CASES += [
        (_e, dict(tile_m=1), ARG, "fino_gemm: tile_m=1 (0 = planned, 2 .. 8)"),
        (_e, dict(tile_m=9), ARG, "fino_gemm: tile_m=9 (0 = planned, 2 .. 8)"),
        (_e, dict(tile_m=-2, a=0), ARG, "fino_gemm: tile_m=-2 (0 = planned, 2 .. 8)"),
        (_e, dict(tile_m=5, m=0), OK, None),
    ]
CASES += [
    ("fino_gemm_split_n", dict(c2=PTR), ARG, SPLIT),
    ("fino_gemm_split_n", dict(n_split=256, n=512, ldc=512), ARG, SPLIT),
    ("fino_gemm_split_n", dict(SPLIT_OK, n_split=100), ARG, SPLIT),
    ("fino_gemm_split_n", dict(SPLIT_OK, n_split=512), ARG, SPLIT),
    ("fino_gemm_split_n", dict(SPLIT_OK, ldc2=8), ARG, SPLIT),
    ("fino_gemm_split_n", dict(SPLIT_OK, ldc2=260), ARG, SPLIT),
    ("fino_gemm_split_n", dict(SPLIT_OK, c2=PTR + 8), ARG, SPLIT),
    ("fino_gemm_split_n", dict(SPLIT_OK, k=72, lda=72, ldw=72), ARG, SPLIT),
    ("fino_gemm_split_n", dict(SPLIT_OK, epilogue=2, r=PTR, ldr=512), ARG, SPLIT),
    ("fino_gemm_split_n", dict(SPLIT_OK, epilogue=5), ARG, SPLIT),
    ("fino_gemm_split_n", dict(SPLIT_OK, ldc=128), ARG, "fino_gemm_split_n: ldc must cover the first n_split columns"),
    ("fino_gemm_split_n", dict(SPLIT_OK, ldc=256, m=0), OK, None),         # ldc covers n_split, not N
    ("fino_gemm_split_n", dict(SPLIT_OK, a=0), ARG, "fino_gemm: null pointer"),
    ("fino_gemm_split_n", dict(SPLIT_OK, tile_m=1, n_split=100), ARG, "fino_gemm: tile_m=1 (0 = planned, 2 .. 8)"),
    ("fino_gemm_split_n", dict(SPLIT_OK, dtype=7, n_split=100), ARG, "fino_gemm: dtype 7"),
    ("fino_gemm_split_n", dict(epilogue=5, tile_m=8), ARG, F32_ARGS),
    ("fino_gemm_keep", dict(epilogue=0), ARG, KEEP_EPI % ("fino_gemm_keep", 0)),
    ("fino_gemm_keep", dict(epilogue=1), ARG, KEEP_EPI % ("fino_gemm_keep", 1)),
    ("fino_gemm_keep", dict(epilogue=5), ARG, KEEP_EPI % ("fino_gemm_keep", 5)),
    ("fino_gemm_keep", dict(keep=0), ARG, KEEP % "fino_gemm_keep"),
    ("fino_gemm_keep", dict(keep=PTR + 8), ARG, KEEP % "fino_gemm_keep"),
    ("fino_gemm_keep", dict(ldk=100), ARG, KEEP % "fino_gemm_keep"),
    ("fino_gemm_keep", dict(ldk=128), ARG, KEEP % "fino_gemm_keep"),
    ("fino_gemm_keep", dict(r=0), ARG, "fino_gemm: residual operand"),
    ("fino_gemm_keep", dict(epilogue=3), ARG, "fino_gemm: gate operand"),
    ("fino_gemm_keep", dict(epilogue=4, gate=PTR, mod_stride=6), ARG, "fino_gemm: gate operand"),
    ("fino_gemm_keep", dict(epilogue=0, dtype=7), ARG, "fino_gemm_keep: dtype 7"),
    ("fino_gemm_keep", dict(epilogue=0, keep=0), ARG, KEEP_EPI % ("fino_gemm_keep", 0)),
    ("fino_gemm_keep", dict(keep=0, tile_m=1), ARG, KEEP % "fino_gemm_keep"),
    ("fino_gemm_keep", dict(keep=0, a=0), ARG, KEEP % "fino_gemm_keep"),
    # the K-blocked A
    ("fino_gemm_blocked_a", dict(dtype=7), ARG, BA + "dtype 7"),
    ("fino_gemm_blocked_a", dict(tile_m=1), ARG, BA + "tile_m=1 (0 = planned, 2 .. 8)"),
    ("fino_gemm_blocked_a", dict(a=0), ARG, BA + "null pointer"),
    ("fino_gemm_blocked_a", dict(r=0), ARG, BA + "null pointer"),
    ("fino_gemm_blocked_a", dict(gate=0), ARG, BA + "null pointer"),
    ("fino_gemm_blocked_a", dict(m=-1), ARG, BA + "bad shape"),
    ("fino_gemm_blocked_a", dict(n=12), ARG, BA + "bad shape"),
    ("fino_gemm_blocked_a", dict(a_block_k=0), ARG, BA + "a_block_k=0 must be a multiple of 64 dividing K=128"),
    ("fino_gemm_blocked_a", dict(a_block_k=96, lda=96), ARG, BA + "a_block_k=96 must be a multiple of 64 dividing K=128"),
    ("fino_gemm_blocked_a", dict(k=192, a_block_k=128, lda=128, ldw=192), ARG,
     BA + "a_block_k=128 must be a multiple of 64 dividing K=192"),
    ("fino_gemm_blocked_a", dict(k=64 * 257, a_block_k=64 * 257, lda=64 * 257, ldw=64 * 257), ARG,
     BA + "a_block_k=16448 must be a multiple of 64 dividing K=16448"),
    ("fino_gemm_blocked_a", dict(k=64 * 4097, ldw=64 * 4097), ARG, BA + "a_block_k=64 must be a multiple of 64 dividing K=262208"),
    ("fino_gemm_blocked_a", dict(lda=32), ARG, BA + "leading dimensions"),
    ("fino_gemm_blocked_a", dict(a_block_stride=4), ARG, BA + "leading dimensions"),
    ("fino_gemm_blocked_a", dict(ldw=64), ARG, BA + "leading dimensions"),
    ("fino_gemm_blocked_a", dict(ldc=128), ARG, BA + "leading dimensions"),
    ("fino_gemm_blocked_a", dict(ldr=100), ARG, BA + "leading dimensions"),
    ("fino_gemm_blocked_a", dict(mod_stride=2), ARG, BA + "leading dimensions"),
    ("fino_gemm_blocked_a", dict(w=PTR + 8), ARG, BA + "16-byte alignment required"),
    ("fino_gemm_blocked_a", dict(gate=PTR + 4), ARG, BA + "16-byte alignment required"),
    ("fino_gemm_blocked_a", dict(a_groups=0), ARG, BA + "a_groups=0 must divide the 2 K blocks"),
    ("fino_gemm_blocked_a", dict(a_groups=3), ARG, BA + "a_groups=3 must divide the 2 K blocks"),
    ("fino_gemm_blocked_a", dict(a_groups=17), ARG, BA + "a_groups=17 must divide the 2 K blocks"),
    ("fino_gemm_blocked_a", dict(a_groups=2, a_group_stride=4), ARG, BA + "a_groups=2 must divide the 2 K blocks"),
    ("fino_gemm_blocked_a", dict(a_block_stride=1 << 30), ARG, BA + "operands must span < 2 GiB"),
    ("fino_gemm_blocked_a", dict(a_groups=2, a_group_stride=1 << 30), ARG, BA + "operands must span < 2 GiB"),
    ("fino_gemm_blocked_a", dict(n=1 << 23, ldc=1 << 23, ldr=1 << 23), ARG, BA + "operands must span < 2 GiB"),
    ("fino_gemm_blocked_a", dict(m=0), OK, None),
    ("fino_gemm_blocked_a", dict(m=0, a_block_stride=1 << 30), ARG, BA + "operands must span < 2 GiB"),
    # behind the validation, in front of the launch: 255 K-tiles per block, 510 K-tiles
    ("fino_gemm_blocked_a", dict(k=32640, a_block_k=16320, lda=16320, ldw=32640, a_block_stride=16320 * 256), UNSUPPORTED,
     BA + "a_block_k=16320 / a_groups=1 with K=32640 is beyond the exact range of the kernel's reciprocal index arithmetic"),
    ("fino_gemm_blocked_a", dict(dtype=7, tile_m=1), ARG, BA + "dtype 7"),
    ("fino_gemm_blocked_a", dict(tile_m=9, a=0), ARG, BA + "tile_m=9 (0 = planned, 2 .. 8)"),
    ("fino_gemm_blocked_a", dict(r=0, n=12), ARG, BA + "null pointer"),
    ("fino_gemm_blocked_a", dict(n=12, a_block_k=0), ARG, BA + "bad shape"),
    ("fino_gemm_blocked_a", dict(lda=32, w=PTR + 8), ARG, BA + "leading dimensions"),
    ("fino_gemm_blocked_a", dict(w=PTR + 8, a_groups=3), ARG, BA + "16-byte alignment required"),
]
for _e in ("fino_conv3d", "fino_conv3d_split"):
    CASES += [
        (_e, dict(a=0), ARG, "fino_conv3d: null pointer"),
        (_e, dict(zero_page=0), ARG, "fino_conv3d: null pointer"),
        (_e, dict(c_in_pad=32), ARG, "fino_conv3d: c_in_pad=32 must be a multiple of 64 (pad channels with zeros)"),
        (_e, dict(c_in_pad=0), ARG, "fino_conv3d: c_in_pad=0 must be a multiple of 64 (pad channels with zeros)"),
        (_e, dict(c_out_pad=12), ARG, "fino_conv3d: c_out_pad=12 % 8 != 0"),
        (_e, dict(t_in=0), ARG, "fino_conv3d: bad geometry"),
        (_e, dict(w_out=0), ARG, "fino_conv3d: bad geometry"),
        (_e, dict(kh=0), ARG, "fino_conv3d: bad geometry"),
        (_e, dict(st=0), ARG, "fino_conv3d: bad geometry"),
        (_e, dict(pw=-1), ARG, "fino_conv3d: bad geometry"),
        (_e, dict(epilogue=1), ARG, "fino_conv3d: epilogue 1 (NONE or RESIDUAL with r)"),
        (_e, dict(epilogue=2), ARG, "fino_conv3d: epilogue 2 (NONE or RESIDUAL with r)"),
        (_e, dict(a=PTR + 8), ARG, "fino_conv3d: 16-byte alignment required"),
        (_e, dict(epilogue=2, r=PTR + 8), ARG, "fino_conv3d: 16-byte alignment required"),
        (_e, dict(zero_page=PTR + 2), ARG, "fino_conv3d: 16-byte alignment required"),
        (_e, dict(c=0, c_in_pad=32), ARG, "fino_conv3d: null pointer"),
        (_e, dict(c_in_pad=32, c_out_pad=12), ARG, "fino_conv3d: c_in_pad=32 must be a multiple of 64 (pad channels with zeros)"),
        (_e, dict(c_out_pad=12, kt=0), ARG, "fino_conv3d: c_out_pad=12 % 8 != 0"),
        (_e, dict(kt=0, epilogue=1), ARG, "fino_conv3d: bad geometry"),
        (_e, dict(epilogue=1, w=PTR + 8), ARG, "fino_conv3d: epilogue 1 (NONE or RESIDUAL with r)"),
    ]
CASES += [
    ("fino_conv3d", dict(dtype=7), ARG, "fino_conv3d: dtype 7"),
    ("fino_conv3d", dict(dtype=2, a=0), ARG, "fino_conv3d: dtype 2"),
    ("fino_conv3d_split", dict(planes=1), ARG, "fino_conv3d_split: planes = 1 (2: hi | lo, 3: hi | mid | lo)"),
    ("fino_conv3d_split", dict(planes=4, a=0), ARG, "fino_conv3d_split: planes = 4 (2: hi | lo, 3: hi | mid | lo)"),
    ("fino_conv3d_split", dict(bias=PTR + 4), ARG, "fino_conv3d_split: bias must be 16-byte aligned"),
    ("fino_conv3d_split", dict(bias=PTR + 4, a=PTR + 8), ARG, "fino_conv3d: 16-byte alignment required"),
    # behind the validation, in front of the launch
    ("fino_conv3d_split", dict(c_out_pad=72), UNSUPPORTED, CONV_SPAN),
    ("fino_conv3d_split", dict(c_out_pad=72, planes=3, epilogue=2, r=PTR), UNSUPPORTED, CONV_SPAN.replace("81920", "122880")),
    ("fino_skinny_linear", dict(a=0), ARG, "fino_skinny_linear: null pointer"),
    ("fino_skinny_linear", dict(w=0), ARG, "fino_skinny_linear: null pointer"),
    ("fino_skinny_linear", dict(c=0), ARG, "fino_skinny_linear: null pointer"),
    ("fino_skinny_linear", dict(m=0), ARG, "fino_skinny_linear: need 1 <= M <= 16 (M=0)"),
    ("fino_skinny_linear", dict(m=17), ARG, "fino_skinny_linear: need 1 <= M <= 16 (M=17)"),
    ("fino_skinny_linear", dict(n=0), ARG, "fino_skinny_linear: need 1 <= M <= 16 (M=2)"),
    ("fino_skinny_linear", dict(k=0), ARG, "fino_skinny_linear: need 1 <= M <= 16 (M=2)"),
    ("fino_skinny_linear", dict(dtype=2), ARG, "fino_skinny_linear: w_dtype 2"),
    ("fino_skinny_linear", dict(dtype=-2), ARG, "fino_skinny_linear: w_dtype -2"),
    ("fino_skinny_linear", dict(a=0, m=17), ARG, "fino_skinny_linear: null pointer"),
    ("fino_skinny_linear", dict(m=17, dtype=2), ARG, "fino_skinny_linear: need 1 <= M <= 16 (M=17)"),
]
for _e in MXS + ("fino_gemm_mxfp8_q",):
    CASES += [
        (_e, dict(dtype=7), ARG, _e + ": dtype 7"),
        (_e, dict(a=0), ARG, _e + ": null pointer"),
        (_e, dict(sa=0), ARG, _e + ": null pointer"),
        (_e, dict(w=0), ARG, _e + ": null pointer"),
        (_e, dict(sw=0), ARG, _e + ": null pointer"),
        (_e, dict(c=0), ARG, _e + ": null pointer"),
        (_e, dict(k=64), ARG, _e + ": K=64 must be a multiple of 128, N=256 of 8"),
        (_e, dict(k=0), ARG, _e + ": K=0 must be a multiple of 128, N=256 of 8"),
        (_e, dict(n=12), ARG, _e + ": K=128 must be a multiple of 128, N=12 of 8"),
        (_e, dict(m=-1), ARG, _e + ": K=128 must be a multiple of 128, N=256 of 8"),
        (_e, dict(a=PTR + 8), ARG, _e + ": alignment / leading dimension"),
        (_e, dict(sw=PTR + 4), ARG, _e + ": alignment / leading dimension"),
        (_e, dict(epilogue=5), ARG, _e + ": epilogue 5"),
        (_e, dict(epilogue=-1), ARG, _e + ": epilogue -1"),
        (_e, dict(m=1 << 24), UNSUPPORTED, _e + ": operand > 2 GiB"),
        (_e, dict(n=1 << 24, ldc=1 << 24, ldk=1 << 24, ldr=1 << 24), UNSUPPORTED, _e + ": operand > 2 GiB"),
        (_e, dict(m=0), OK, None),
        (_e, dict(dtype=7, a=0), ARG, _e + ": dtype 7"),
        (_e, dict(a=0, k=64), ARG, _e + ": null pointer"),
        (_e, dict(k=64, a=PTR + 8), ARG, _e + ": K=64 must be a multiple of 128, N=256 of 8"),
        (_e, dict(a=PTR + 8, epilogue=-1), ARG, _e + ": alignment / leading dimension"),
    ]
for _e in MXS:
    CASES += [
        (_e, dict(ldc=100), ARG, _e + ": alignment / leading dimension"),
        (_e, dict(ldc=128), ARG, _e + ": alignment / leading dimension"),
        (_e, dict(c=PTR + 8), ARG, _e + ": alignment / leading dimension"),
        (_e, dict(epilogue=2, r=0), ARG, _e + ": residual operand"),
        (_e, dict(epilogue=2, r=PTR, ldr=128), ARG, _e + ": residual operand"),
        (_e, dict(epilogue=4, r=PTR + 8, ldr=256), ARG, _e + ": residual operand"),
        (_e, dict(GATED, gate=0), ARG, _e + ": gate operand"),
        (_e, dict(GATED, mod_stride=2), ARG, _e + ": gate operand"),
        (_e, dict(GATED, epilogue=4, gate=PTR + 4), ARG, _e + ": gate operand"),
        (_e, dict(GATED, m=0), OK, None),
        (_e, dict(epilogue=3, r=0, gate=0), ARG, _e + ": residual operand"),
    ]
for _e in ("fino_gemm_mxfp8_keep", "fino_gemm_mxfp6_keep"):
    CASES += [
        (_e, dict(epilogue=0), ARG, KEEP_EPI % (_e, 0)),
        (_e, dict(epilogue=1), ARG, KEEP_EPI % (_e, 1)),
        (_e, dict(keep=0), ARG, KEEP % _e),
        (_e, dict(keep=PTR + 8), ARG, KEEP % _e),
        (_e, dict(ldk=100), ARG, KEEP % _e),
        (_e, dict(ldk=128), ARG, KEEP % _e),
        (_e, dict(epilogue=0, keep=0), ARG, KEEP_EPI % (_e, 0)),
        (_e, dict(keep=0, m=1 << 24), ARG, KEEP % _e),
        (_e, dict(keep=0, m=0), ARG, KEEP % _e),
        (_e, dict(epilogue=0, r=0, a=0), ARG, _e + ": null pointer"),
    ]
CASES += [
    ("fino_gemm_mxfp8_q", dict(cs=0), ARG, "fino_gemm_mxfp8_q: null pointer"),
    ("fino_gemm_mxfp8_q", dict(n=264), ARG, "fino_gemm_mxfp8_q: K=128 and N=264 must be multiples of 128"),
    ("fino_gemm_mxfp8_q", dict(epilogue=2), ARG, "fino_gemm_mxfp8_q: residual operand"),      # (it has no residual to give)
    ("fino_gemm_mxfp8_q", dict(c=PTR + 4), ARG, "fino_gemm_mxfp8_q: alignment"),
    ("fino_gemm_mxfp8_q", dict(c=PTR + 8, epilogue=1, m=0), OK, None),                        # 8-byte aligned is enough
    ("fino_gemm_mxfp8_q", dict(cs=0, n=264), ARG, "fino_gemm_mxfp8_q: null pointer"),
    ("fino_gemm_mxfp8_q", dict(n=264, c=PTR + 4), ARG, "fino_gemm_mxfp8_q: K=128 and N=264 must be multiples of 128"),
    ("fino_gemm_mxfp8_q", dict(c=PTR + 4, m=1 << 24), ARG, "fino_gemm_mxfp8_q: alignment"),
]
for _e in ("fino_quantize_mxfp8", "fino_quantize_mxfp6", "fino_quantize_mxfp6_rot"):
    _shape = _e + ": cols must be a multiple of 128 (rows=%d cols=%d)"
    CASES += [
        (_e, dict(dtype=7), ARG, _e + ": dtype 7"),
        (_e, dict(a=0), ARG, _e + ": null pointer"),
        (_e, dict(c=0), ARG, _e + ": null pointer"),
        (_e, dict(cs=0), ARG, _e + ": null pointer"),
        (_e, dict(rows=0), ARG, _shape % (0, 128)),
        (_e, dict(cols=64, ldx=64), ARG, _shape % (16, 64)),
        (_e, dict(cols=0), ARG, _shape % (16, 0)),
        (_e, dict(ldx=64), ARG, _shape % (16, 128)),
        (_e, dict(ldx=132), ARG, _shape % (16, 128)),
        (_e, dict(a=PTR + 8), ARG, _e + ": alignment"),
        (_e, dict(c=PTR + 4), ARG, _e + ": alignment"),
        (_e, dict(dtype=7, a=0), ARG, _e + ": dtype 7"),
        (_e, dict(a=0, rows=0), ARG, _e + ": null pointer"),
        (_e, dict(rows=0, a=PTR + 8), ARG, _shape % (0, 128)),
    ]
CASES += [
    ("fino_quantize_mxfp6", dict(c=PTR + 8), ARG, "fino_quantize_mxfp6: alignment"),          # e2m3 fragments: 16 bytes
    ("fino_quantize_mxfp6_rot", dict(c=PTR + 8, mode=2), ARG, "fino_quantize_mxfp6_rot: alignment"),
    ("fino_quantize_mxfp6_rot", dict(mode=0), ARG, "fino_quantize_mxfp6_rot: mode 0 (FINO_MX_ROT_ACT = 1 | FINO_MX_ROT_WEIGHT = 2)"),
    ("fino_quantize_mxfp6_rot", dict(mode=3, dtype=7), ARG,
     "fino_quantize_mxfp6_rot: mode 3 (FINO_MX_ROT_ACT = 1 | FINO_MX_ROT_WEIGHT = 2)"),
    ("fino_quantize_mxfp6_rot", dict(mode=2, dtype=7), ARG, "fino_quantize_mxfp6_rot: dtype 7"),
    ("fino_quantize_mxfp6_rot", dict(mode=2, rows=-1), ARG, "fino_quantize_mxfp6_rot: cols must be a multiple of 128 (rows=-1 cols=128)"),
]


def _case_id(c):
    return "%s-%s" % (c[0], "+".join("%s=%s" % kv for kv in c[1].items()))


@pytest.mark.parametrize("entry,changes,rc,message", CASES, ids=[_case_id(c) for c in CASES])
def test_bad_arguments_keep_their_return_code_and_message(lib, entry, changes, rc, message):
    assert rc != OK or changes.get("m") == 0          # what returns FINO_OK here is an empty GEMM: nothing is launched
    assert _call(lib, entry, changes) == (rc, message)


def test_every_entry_point_of_the_family_is_covered():
    assert {c[0] for c in CASES} == set(ORDER)
    assert len({_case_id(c) for c in CASES}) == len(CASES)


def test_plan_rejects_empty_shapes(lib):
    """fino_gemm_plan validates without a message: the code alone, and the last error stays what it was"""
    lib.fino_gemm(0, PTR, 0, PTR, 256, 256, 128, 128, 128, 256, 0, 0, 0, 0, 0, 0, 0, 0)
    for m, n in ((0, 256), (-5, 256), (256, 0), (0, 0)):
        rows, rest = ctypes.c_int64(-7), ctypes.c_int(-7)
        assert lib.fino_gemm_plan(m, n, ctypes.byref(rows), ctypes.byref(rest)) == ARG
        assert (rows.value, rest.value) == (-7, -7)
    assert lib.fino_last_error().decode() == "fino_gemm: null pointer"
