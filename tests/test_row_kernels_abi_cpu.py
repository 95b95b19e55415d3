"""Error contract of the row, sampler, step-cache, token, guider, LoRA, condition and VAE entry points, on the CPU: the 58
`extern "C"` functions of fino_elementwise.hip, fino_step_cache.hip, fino_vae.hip, fino_guidance.hip, fino_token_select.hip,
fino_vae_cog.hip, fino_conditions.hip and fino_lora.hip are called with arguments that break each of their checks in turn, and
must answer with the recorded return code and message (validation runs before any launch, tests/test_lib_abi.py).  Two faults
at once pin the order in which an entry point reports; an empty input returns FINO_OK without a launch.  No case reaches a
launch: a library on a machine without a GPU answers every one of them.

The expected (rc, message) are tests/golden/row_kernels_abi.json.  They were RECORDED, from the library of the commit before
these translation units took their host halves from fino_host.h, and are not written from reading the code:

    make -C frameino_amd/csrc variant NAME=parent          # in a checkout of that commit
    FINO_LIB_PATH=<that checkout>/frameino_amd/lib/libframeino_parent.so python tools/record_row_kernels_abi.py

The four entry points without an error channel (the workspace sizes, fino_fastercache_supported) are recorded by value.

The test passes against both libraries, the recorded one and the one built from this tree (1229 cases each).  Checks that no
argument list can make fail on their own, and that therefore have no case: `parts`, "a segment asks for RoPE without tables" and
"segments need dim % 8 == 0" of the RMSNorm family (the entry points build the segments themselves), the `dim % 8` term of
fino_qkv_rmsnorm_rope_rows' head_dim check (the rows / dim check in front of it has refused), the LDS bound of
fino_fastercache_delta (every supported plane fits) and "n too large" of fino_lora_merge (at most 2048 segments are asked for)."""
import ctypes
import json
import os
import re

import pytest

from frameino_amd import _lib

PTR = 4096                       # a non-null, 16-byte aligned "device pointer": no case gets as far as a launch
OK, ARG, UNSUPPORTED = 0, -1, -3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "row_kernels_abi.json")
B31, B40 = 1 << 31, 1 << 40
NAN = float("nan")


def _argument_names():
    """entry point -> the argument names of its prototype in include/frameino_hip.h"""
    text = open(_lib.HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return {m.group(1): [re.findall(r"\w+", a)[-1] for a in m.group(2).split(",")]
            for m in re.finditer(r"\b(fino_\w+)\s*\(([^)]*)\)\s*;", text) if m.group(2).strip() not in ("", "void")}


ORDER = _argument_names()

_ROW = dict(rows=8, dim=64, ldx=64, ldy=64, ldo=64, mod_stride=64)
_RMS = dict(rows=8, dim=64, ldx=64, head_dim=32)
_HEADNORM = dict(batch=1, rows=8, heads=2, head_dim=64, ldx=128, batch_stride=1024, rope_row0=0)
_FRAMES = dict(channels=4, gen_frames=2, total_frames=3, height=4, width=4, round_out=0)
_FLAT = dict(n_lat=64, batch_stride=64, has_uncond=1)
_VEC = dict(rows=8, dim=64, lda=64, ldb=64, ldo=64, ldx=64, ldy=64, mod_stride=64, subtract=1)
_MOVE = dict(ld_src=64, n=16, k=4, row_bytes=64, ld_dst=64)
_SEG = dict(seg_h0=PTR, seg_h1=PTR, seg_p=PTR, seg_r=PTR, seg_h1_copy=PTR, seg_rows=8, seg_ld_h0=64, seg_ld_h1=64, seg_ld_p=64,
            seg_ld_r=64, seg_ld_h1_copy=64)
# what a call that would pass validation (and launch) gives for everything that is not a pointer or a float; pointers default
# to PTR, floats to 1.0, the stream to NULL.  Every case below breaks such a call or makes it empty.
DEFAULTS = {
    "fino_adaln_modulate": _ROW, "fino_layernorm": _ROW, "fino_layernorm_zero": _ROW,
    "fino_gated_residual": _ROW, "fino_gated_residual_staged": _ROW,
    "fino_ln_mxfp8": dict(mode=2, rows=8, dim=128, ldx=128, mod_stride=128),
    "fino_row_rrms": dict(rows=8, dim=64, ldx=64),
    "fino_rmsnorm_rope": _RMS, "fino_rmsnorm_rope_scaled": _RMS, "fino_rmsnorm_rope_scatter": _RMS,
    "fino_qkv_rmsnorm_rope": dict(_RMS, ldx=192),
    "fino_qkv_rmsnorm_rope_rows": dict(_RMS, ldx=192, n=16, ld_cache=64),
    "fino_headnorm_rope": _HEADNORM, "fino_headnorm_rope_scaled": _HEADNORM,
    "fino_patchify": dict(channels=4, frames=2, height=4, width=4, pt=1, ph=2, pw=2, lda=16),
    "fino_unpatchify": dict(cout=4, frames=2, height=4, width=4, pt=1, ph=2, pw=2, ldy=16),
    "fino_wan_model_input": dict(channels=4, gen_frames=2, id_frames=1, height=4, width=4),
    "fino_cfg_vpred_step": _FLAT, "fino_cfg_dpm_step": _FLAT, "fino_guided_vpred_step": _FLAT, "fino_guided_dpm_step": _FLAT,
    "fino_cfg_unipc_step": _FRAMES, "fino_cfg_euler_step": _FRAMES, "fino_guided_unipc_step": _FRAMES,
    "fino_guided_euler_step": _FRAMES,
    "fino_step_cache_probe": dict(_SEG, segs="auto", nseg=1, dim=64),
    "fino_step_cache_residual": _VEC, "fino_pab_broadcast": _VEC,
    "fino_magcache_workspace_bytes": dict(rows=8),
    "fino_magcache_calibrate": dict(ld_out=64, ld_in=64, ld_prev=64, ld_new=64, rows=8, dim=64, workspace_bytes=1 << 20),
    "fino_taylor_update": dict(ldy=64, plane_stride=512, ldf=64, rows=8, dim=64, n_old=1, n_new=2, delta=1, fdtype=0),
    "fino_taylor_predict": dict(plane_stride=512, ldf=64, n=2, coef="auto", ldx=64, ldo=64, rows=8, dim=64, mod_stride=64, fdtype=0),
    "fino_fastercache_supported": dict(planes=1, height=4, width=4),
    "fino_fastercache_delta": dict(planes=2, height=8, width=8),
    "fino_fastercache_apply": dict(n=64),
    "fino_rmsnorm_silu_cl": dict(rows=8, c_valid=60, c_pad=64, silu=1),
    "fino_rmsnorm_silu_cl_f32": dict(rows=8, c_valid=60, c_pad=64, silu=1, nseg=0, planes_packed=0),
    "fino_softmax_rows": dict(rows=8, n=16, ld=16),
    "fino_dup_up3d_add": dict(t_in=2, h_in=4, w_in=4, c_in=8, c_in_pad=8, c_out=4, c_out_pad=8, factor_t=2, factor_s=2),
    "fino_avg_down3d_add": dict(t_in=2, h_in=4, w_in=4, c_in=4, c_in_pad=8, c_out=8, c_out_pad=8, factor_t=2, factor_s=2),
    "fino_vae_unpatchify_clamp": dict(t=2, h=4, w=4, c_pad=64, channels=3, patch=2),
    "fino_vae_patchify": dict(t=2, h=4, w=4, c_pad=64, channels=3, patch=2),
    "fino_split_bf16": dict(rows=8, cols=64, ldx=64, ldo=128, nseg=2, planes_packed=4),
    "fino_guider_workspace_bytes": dict(n=64),
    "fino_guider_coefs": dict(rows=4, row_len=64, row_stride=64, kind=0, norm_threshold=0.0, eta=1.0, guidance_rescale=0.5,
                              workspace_bytes=1 << 20),
    "fino_token_score": dict(rows=8, cols=16, ld=16, batch=1),
    "fino_token_select": dict(n=16, k=4),
    "fino_gather_rows": _MOVE, "fino_scatter_rows": _MOVE,
    "fino_groupnorm_workspace_bytes": dict(c_pad=64),
    "fino_groupnorm_cl": dict(t=2, h=4, w=4, channels=32, c_pad=64, groups=4, tz=1, hz=2, wz=2, silu=1, workspace_bytes=1 << 24),
    "fino_avg_pool_time2": dict(t_in=3, h=4, w=4, c_pad=8),
    "fino_vae_blend_tiles": dict(t=2, h_a=4, w_a=4, h_b=4, w_b=4, c_pad=8, extent=2, axis=0),
    "fino_resize_area_pad_u8": dict(src_h=8, src_w=8, region_h=4, region_w=4, out_h=8, out_w=8, off_y=2, off_x=2, fill=0),
    "fino_u8_hwc_to_chw_unit": dict(height=4, width=4),
    "fino_traj_paint": dict(frames=2, height=4, width=4, radius=1),
    "fino_traj_blur_quantize": dict(taps=5, planes=2, height=4, width=4),
    # the adapter arrays are host arrays of n_adapters entries, every entry a0 / lda0 / b0 / ldb0 / rank0 / scale0
    "fino_lora_merge": dict(ldw_base=64, ldw_out=64, n=16, k=64, n_adapters=1, a="auto", lda="auto", b="auto", ldb="auto",
                            rank="auto", scale="auto", a0=PTR, lda0=64, b0=PTR, ldb0=8, rank0=8, scale0=1.0),
}
_LORA_ARRAYS = dict(a=ctypes.c_void_p, lda=ctypes.c_int64, b=ctypes.c_void_p, ldb=ctypes.c_int64, rank=ctypes.c_int,
                    scale=ctypes.c_float)


def _defaults(entry):
    d = dict(DEFAULTS[entry])
    for name, ctype in zip(ORDER[entry], _lib.SIGNATURES[entry]):
        if name in d:
            continue
        if name == "stream" or name == "dtype":
            d[name] = 0
        elif ctype is ctypes.c_void_p:
            d[name] = PTR
        elif ctype in (ctypes.c_float, ctypes.c_double):
            d[name] = 1.0
        else:
            raise KeyError("%s: no default for %s" % (entry, name))
    return d


def _call(lib, entry, changes):
    d = _defaults(entry)
    assert set(changes) <= set(d) or entry == "fino_step_cache_probe", (entry, changes)
    d.update(changes)
    keep = []                                        # the host arrays stay alive across the call
    if entry == "fino_step_cache_probe" and d["segs"] == "auto":
        segs = (_lib.StepCacheSegment * 4)()
        for i in range(4):
            for field, _ in _lib.StepCacheSegment._fields_:
                setattr(segs[i], field, d.get("seg%d_%s" % (i, field), d["seg_" + field]))
        keep.append(segs)
        d["segs"] = ctypes.addressof(segs)
    if entry == "fino_lora_merge":
        for name, ctype in _LORA_ARRAYS.items():
            if d[name] == "auto":
                keep.append((ctype * 8)(*[d[name + "0"]] * 8))
                d[name] = keep[-1]
            else:
                d[name] = None
    if entry == "fino_taylor_predict":
        keep.append((ctypes.c_float * 4)(1.0, 0.5, 0.25, 0.125))
        d["coef"] = keep[-1] if d["coef"] == "auto" else None
    rc = getattr(lib, entry)(*[d[name] for name in ORDER[entry]])
    if entry in VALUES:
        return rc, None
    return rc, lib.fino_last_error().decode() if rc else None


VALUES = ("fino_magcache_workspace_bytes", "fino_fastercache_supported", "fino_guider_workspace_bytes",
          "fino_groupnorm_workspace_bytes")
CASES = []          # (entry point, what is wrong with the call, kind): "refused" | "empty" (FINO_OK, nothing launched) | "value"


def R(entry, **changes):
    CASES.append((entry, changes, "refused"))


def E(entry, **changes):
    CASES.append((entry, changes, "empty"))


def V(entry, **changes):
    CASES.append((entry, changes, "value"))


def each(fn, entry, name, *values):
    for v in values:
        fn(entry, **{name: v})


def nulls(entry, *names):
    for name in names:
        R(entry, **{name: 0})


def off16(entry, *names, by=8):
    for name in names:
        R(entry, **{name: PTR + by})


# ---- fino_elementwise.hip ----
for _e in ("fino_adaln_modulate", "fino_ln_mxfp8", "fino_layernorm", "fino_layernorm_zero", "fino_gated_residual",
           "fino_gated_residual_staged", "fino_rmsnorm_rope", "fino_rmsnorm_rope_scaled", "fino_rmsnorm_rope_scatter",
           "fino_qkv_rmsnorm_rope", "fino_qkv_rmsnorm_rope_rows"):
    _x = "qkv" if "qkv" in _e else "x"
    each(R, _e, "dtype", 7, 2, -1)
    each(R, _e, "rows", -1)
    each(R, _e, "dim", 0, -8, 12)
    E(_e, rows=0)
    E(_e, **{"rows": 0, _x: 0})                      # the empty input returns in front of the pointer checks
    E(_e, rows=0, ldx=3)
    R(_e, dtype=7, rows=-1)
    R(_e, **{"dim": 12, _x: 0})
    R(_e, rows=0, dim=12)
    R(_e, rows=0, dtype=7)
    nulls(_e, _x)
    R(_e, ldx=68)
    off16(_e, _x)
    R(_e, **{_x: 0, "ldx": 68})
for _e in ("fino_adaln_modulate", "fino_layernorm", "fino_layernorm_zero"):
    nulls(_e, "y")
    R(_e, ldy=68)
    off16(_e, "y")
    R(_e, dim=4104, ldx=4104, ldy=4104)              # beyond eight passes: refused behind the validation, nothing launched
    R(_e, dim=4104, ldx=4104, ldy=4104, y=PTR + 8)
for _e in ("fino_adaln_modulate", "fino_layernorm_zero"):
    nulls(_e, "shift", "scale")
    R(_e, mod_stride=2)
    off16(_e, "shift", "scale", by=4)
    R(_e, shift=0, mod_stride=2)
for _e in ("fino_layernorm", "fino_layernorm_zero"):
    off16(_e, "w", "b", by=4)
each(R, "fino_ln_mxfp8", "mode", -1, 3)
nulls("fino_ln_mxfp8", "q", "scales", "shift", "scale")
R("fino_ln_mxfp8", dim=64, ldx=64)
R("fino_ln_mxfp8", dim=192, ldx=192)
R("fino_ln_mxfp8", ldx=132)
R("fino_ln_mxfp8", mod_stride=2)
off16("fino_ln_mxfp8", "shift", "scale", "w", "b", "q", by=4)
R("fino_ln_mxfp8", mode=3, shift=0)
R("fino_ln_mxfp8", mode=1, shift=0, dim=64, ldx=64)
R("fino_ln_mxfp8", shift=0, dim=64, ldx=64)
R("fino_ln_mxfp8", dim=64, ldx=64, x=PTR + 8)
R("fino_ln_mxfp8", dim=4224, ldx=4224)
R("fino_ln_mxfp8", mode=0, dim=4224, ldx=4224)
R("fino_ln_mxfp8", mode=1, dim=4224, ldx=4224, shift=0, scale=0)
for _e in ("fino_gated_residual", "fino_gated_residual_staged"):
    nulls(_e, "y", "out")
    each(R, _e, "ldy", 68)
    each(R, _e, "ldo", 68)
    R(_e, mod_stride=2)
    off16(_e, "y", "out")
    off16(_e, "gate", by=4)
    R(_e, out=0, ldo=68)
for _e in ("fino_rmsnorm_rope", "fino_rmsnorm_rope_scaled", "fino_rmsnorm_rope_scatter"):
    off16(_e, "weight", "cos_t", "sin_t", by=4)
    nulls(_e, "cos_t", "sin_t")
    each(R, _e, "head_dim", 0, 12, 48)
    R(_e, dim=4104, ldx=4104, head_dim=8)
    R(_e, weight=PTR + 4, cos_t=0)
    R(_e, cos_t=0, head_dim=12)
    R(_e, head_dim=12, ldx=68)
for _e in ("fino_rmsnorm_rope_scaled", "fino_rmsnorm_rope_scatter"):
    each(R, _e, "out_scale", 0.0, -1.0)
    R(_e, out_scale=0.0, weight=PTR + 4)
    R(_e, out_scale=0.0, x=0)
nulls("fino_rmsnorm_rope_scatter", "out", "head_off", "head_ld")
off16("fino_rmsnorm_rope_scatter", "out")
R("fino_rmsnorm_rope_scatter", cos_t=0, sin_t=0, head_dim=0)      # the scatter needs head_dim without RoPE too
R("fino_rmsnorm_rope_scatter", out=0, dtype=7)
R("fino_rmsnorm_rope_scatter", head_off=0, rows=0)
nulls("fino_qkv_rmsnorm_rope", "out", "head_off", "head_ld", "cos_t", "sin_t")
each(R, "fino_qkv_rmsnorm_rope", "q_out_scale", 0.0)
off16("fino_qkv_rmsnorm_rope", "q_weight", "k_weight", "cos_t", "sin_t", by=4)
off16("fino_qkv_rmsnorm_rope", "out")
each(R, "fino_qkv_rmsnorm_rope", "head_dim", 0, 12, 48)
R("fino_qkv_rmsnorm_rope", dim=4104, ldx=12312, head_dim=8)
R("fino_qkv_rmsnorm_rope", out=0, head_off=0, head_ld=0, dim=4104, ldx=12312, head_dim=8)
R("fino_qkv_rmsnorm_rope", out=0, dtype=7)
R("fino_qkv_rmsnorm_rope", q_out_scale=0.0, k_weight=PTR + 4)
R("fino_qkv_rmsnorm_rope", k_weight=PTR + 4, sin_t=0)
_e = "fino_qkv_rmsnorm_rope_rows"
nulls(_e, "q_weight", "k_weight", "cos_t", "sin_t", "kcache", "vcache")
each(R, _e, "q_out_scale", 0.0, -2.0)
each(R, _e, "head_dim", 0, 12, 48)
each(R, _e, "n", 0, B31)
R(_e, idx=0, n=4)
each(R, _e, "ldx", 128, 191)
each(R, _e, "ld_cache", 56, 68)
R(_e, ldx=196)
off16(_e, "kcache", "vcache")
off16(_e, "cos_t", "sin_t", "q_weight", "k_weight", by=4)
R(_e, dim=4104, ldx=12312, ld_cache=4104, head_dim=8)
R(_e, kcache=0, q_out_scale=0.0)
R(_e, q_out_scale=0.0, head_dim=12)
R(_e, head_dim=12, n=0)
R(_e, n=0, ldx=128)
R(_e, ldx=128, vcache=PTR + 8)
R(_e, vcache=PTR + 8, dim=4104, ldx=12312, ld_cache=4104, head_dim=8)
_e = "fino_row_rrms"
each(R, _e, "dtype", 7, 2)
nulls(_e, "x", "rrms")
each(R, _e, "rows", -1)
each(R, _e, "dim", 0, 12)
R(_e, ldx=68)
off16(_e, "x")
E(_e, rows=0)
R(_e, dim=4104, ldx=4104)
R(_e, dtype=7, x=0)
R(_e, rows=0, x=0)
R(_e, rows=0, dim=4104, ldx=4100)
for _e in ("fino_headnorm_rope", "fino_headnorm_rope_scaled"):
    each(R, _e, "dtype", 7, 2)
    nulls(_e, "x")
    R(_e, batch=-1)
    R(_e, rows=-1)
    each(R, _e, "heads", 0, -1)
    each(R, _e, "head_dim", 0, 8, 48, 256)
    nulls(_e, "w", "b", "cos_t", "sin_t")
    R(_e, ldx=132)
    R(_e, batch_stride=1028)
    off16(_e, "x")
    off16(_e, "w", "b", "cos_t", "sin_t", by=4)
    E(_e, rows=0)
    E(_e, batch=0)
    R(_e, dtype=7, x=0)
    R(_e, x=0, head_dim=48)
    R(_e, head_dim=48, w=0)
    R(_e, w=0, ldx=132)
    R(_e, ldx=132, rows=0)
each(R, "fino_headnorm_rope_scaled", "out_scale", 0.0, -1.0)
for _e, _a, _b, _c, _ld in (("fino_patchify", "x", "a", "channels", "lda"), ("fino_unpatchify", "y", "out", "cout", "ldy")):
    each(R, _e, "dtype", 7, 2)
    nulls(_e, _a, _b)
    each(R, _e, _c, 0)
    each(R, _e, "pt", 0)
    each(R, _e, "ph", 0)
    each(R, _e, "pw", 0)
    R(_e, **{"pt": 2, "frames": 3, _ld: 32})
    R(_e, height=5)
    R(_e, width=5)
    each(R, _e, _ld, 8, 15)
    E(_e, frames=0)
    R(_e, **{"dtype": 7, _a: 0})
    R(_e, **{_a: 0, "height": 5})
    R(_e, **{"height": 5, _ld: 8})
    R(_e, **{"frames": 0, _ld: 8})
_e = "fino_wan_model_input"
each(R, _e, "dtype", 7, 2)
nulls(_e, "lat", "cond", "traj", "out", "id_lat")
each(R, _e, "channels", 0)
each(R, _e, "gen_frames", 0)
each(R, _e, "id_frames", -1)
each(R, _e, "height", 0)
each(R, _e, "width", 0)
R(_e, dtype=7, lat=0)
R(_e, lat=0, channels=0)
for _e, _ptrs in (("fino_cfg_vpred_step", ("pred", "lat", "coef_dev")),
                  ("fino_cfg_dpm_step", ("pred", "lat", "x0_old", "noise", "coef_dev")),
                  ("fino_guided_vpred_step", ("pred", "lat", "coef_dev", "ab_dev")),
                  ("fino_guided_dpm_step", ("pred", "lat", "x0_old", "noise", "coef_dev", "ab_dev"))):
    each(R, _e, "dtype", 7, 2)
    nulls(_e, *_ptrs)
    each(R, _e, "n_lat", 0, -4)
    each(R, _e, "batch_stride", 32, 63)
    R(_e, dtype=7, pred=0)
    R(_e, dtype=7, n_lat=0)
for _e, _ptrs in (("fino_cfg_unipc_step", ("cond_pred", "x", "last", "m0", "m1", "coef_dev")),
                  ("fino_cfg_euler_step", ("cond_pred", "lat", "dt_dev")),
                  ("fino_guided_unipc_step", ("cond_pred", "uncond_pred", "x", "last", "m0", "m1", "coef_dev", "ab_dev")),
                  ("fino_guided_euler_step", ("cond_pred", "uncond_pred", "lat", "ab_dev", "dt_dev"))):
    each(R, _e, "dtype", 7, 2)
    nulls(_e, *_ptrs)
    each(R, _e, "channels", 0)
    each(R, _e, "gen_frames", 0)
    each(R, _e, "total_frames", 1)
    each(R, _e, "height", 0)
    each(R, _e, "width", 0)
    R(_e, dtype=7, cond_pred=0)
    R(_e, cond_pred=0, channels=0)

# ---- fino_step_cache.hip ----
_e = "fino_step_cache_probe"
each(R, _e, "dtype", 7, -1)
nulls(_e, "segs")
each(R, _e, "nseg", 0, 5)
nulls(_e, "sums", "workspace")
off16(_e, "sums", "workspace")
each(R, _e, "dim", 0, 12)
R(_e, dim=6, dtype=2)
for _f in ("h0", "h1", "r"):
    R(_e, **{"seg_" + _f: 0})
each(R, _e, "seg_rows", -1, B40)
for _f in ("h0", "h1", "p", "r", "h1_copy"):
    R(_e, **{"seg_ld_" + _f: 56})
    R(_e, **{"seg_ld_" + _f: 68})
    R(_e, **{"seg_" + _f: PTR + 8})
R(_e, dtype=2, seg_ld_p=66)
R(_e, nseg=2, seg1_h0=0)                             # the message names the segment
R(_e, nseg=3, seg2_ld_r=56)
R(_e, nseg=2, seg1_r=PTR + 8, seg0_ld_r=68)
R(_e, dtype=7, segs=0)
R(_e, nseg=0, sums=0)
R(_e, sums=0, dim=12)
R(_e, dim=12, seg_h0=0)
R(_e, seg_h0=0, seg_rows=-1)
R(_e, seg_rows=-1, seg_ld_h0=56)
R(_e, seg_ld_h0=56, seg_h1=PTR + 8)
for _e, _abc in (("fino_step_cache_residual", (("a", "lda"), ("b", "ldb"), ("out", "ldo"))),
                 ("fino_pab_broadcast", (("x", "ldx"), ("y", "ldy"), ("out", "ldo")))):
    each(R, _e, "dtype", 7, -1)
    each(R, _e, "rows", -1)
    each(R, _e, "dim", 0, 12)
    R(_e, rows=B31, dim=8)
    for _p, _ld in _abc:
        nulls(_e, _p)
        R(_e, **{_ld: 56})
        R(_e, **{_ld: 68})
        off16(_e, _p)
    E(_e, rows=0)
    R(_e, dtype=7, rows=-1)
    R(_e, **{"rows": -1, _abc[0][0]: 0})
    R(_e, **{_abc[0][0]: 0, _abc[1][1]: 56})
    R(_e, **{_abc[1][1]: 56, _abc[2][0]: PTR + 8})
    R(_e, **{_abc[2][0]: PTR + 8, "rows": 0})
R("fino_step_cache_residual", dim=6, dtype=2)
R("fino_step_cache_residual", dtype=2, lda=66)
R("fino_pab_broadcast", dtype=2)
off16("fino_pab_broadcast", "gate", by=4)
R("fino_pab_broadcast", mod_stride=2)
each(V, "fino_magcache_workspace_bytes", "rows", 0, -3, 1, 8, 9, 8192, 8193, 10 ** 6)
_e = "fino_magcache_calibrate"
each(R, _e, "dtype", 7, -1)
each(R, _e, "rows", 0, -1, B31)
each(R, _e, "dim", 0, 12)
R(_e, dim=6, dtype=2)
nulls(_e, "x_out", "x_in", "r_prev", "r_new", "stats", "workspace")
for _p, _ld in (("x_out", "ld_out"), ("x_in", "ld_in"), ("r_prev", "ld_prev"), ("r_new", "ld_new")):
    R(_e, **{_ld: 56})
    R(_e, **{_ld: 68})
    off16(_e, _p)
off16(_e, "stats", "workspace")
R(_e, ld_new=128)                                     # r_new is r_prev (both PTR): the strides must agree
R(_e, ld_prev=72)
each(R, _e, "workspace_bytes", 0, 63)
R(_e, rows=10 ** 6, workspace_bytes=4096)
R(_e, dtype=7, rows=0)
R(_e, rows=0, dim=12)
R(_e, dim=12, x_out=0)
R(_e, x_out=0, ld_in=56)
R(_e, ld_in=56, stats=PTR + 8)
R(_e, stats=PTR + 8, ld_new=128)
R(_e, ld_new=128, workspace_bytes=0)
_e = "fino_taylor_update"
each(R, _e, "dtype", 7, 2)
each(R, _e, "fdtype", 7, -1)
each(R, _e, "rows", -1)
each(R, _e, "dim", 0, 12)
R(_e, rows=B31, dim=8)
each(R, _e, "n_old", -1, 5)
each(R, _e, "n_new", 0, 3)
R(_e, n_old=4, n_new=5)
R(_e, delta=0)
R(_e, delta=-2, n_new=2)
nulls(_e, "y", "factors")
R(_e, ldy=56)
R(_e, ldy=68)
off16(_e, "y", "factors")
each(R, _e, "ldf", 56, 68)
each(R, _e, "plane_stride", 516, 256, 511)
R(_e, fdtype=2, ldf=66)
E(_e, rows=0)
E(_e, rows=0, delta=0, n_new=1)
R(_e, dtype=7, fdtype=7)
R(_e, fdtype=7, rows=-1)
R(_e, rows=-1, n_new=0)
R(_e, n_new=3, delta=0)
R(_e, delta=0, y=0)
R(_e, y=0, factors=0)
R(_e, factors=0, rows=0)
_e = "fino_taylor_predict"
each(R, _e, "dtype", 7, 2)
each(R, _e, "fdtype", 7, -1)
each(R, _e, "rows", -1)
each(R, _e, "dim", 0, 12)
each(R, _e, "n", 0, 5)
nulls(_e, "coef", "out", "factors")
each(R, _e, "ldo", 56, 68)
each(R, _e, "ldx", 56, 68)
R(_e, x=0)                                            # a gate needs x
off16(_e, "out", "x", "factors")
off16(_e, "gate", by=4)
R(_e, mod_stride=2)
each(R, _e, "ldf", 56, 68)
each(R, _e, "plane_stride", 516, 256)
E(_e, rows=0)
E(_e, rows=0, x=0, gate=0)
R(_e, dtype=7, fdtype=7)
R(_e, fdtype=7, dim=12)
R(_e, dim=12, n=0)
R(_e, n=0, out=0)
R(_e, out=0, x=0)
R(_e, x=0, factors=0)
R(_e, factors=0, rows=0)
_e = "fino_fastercache_supported"
V(_e, planes=1)
each(V, _e, "planes", 0, -1)
each(V, _e, "height", 0, 16384, 16385, 4096, 4097)
each(V, _e, "width", 0, 4096, 4097)
V(_e, height=128, width=128)
V(_e, height=256, width=128)
_e = "fino_fastercache_delta"
each(R, _e, "dtype", 7, 2)
nulls(_e, "uncond", "cond", "d_low", "d_high")
off16(_e, "uncond", "cond", "d_low", "d_high")
each(R, _e, "planes", 0, B31)
each(R, _e, "height", 0, 16385)
each(R, _e, "width", 0)
R(_e, height=200, width=100)
R(_e, dtype=7, cond=0)
R(_e, cond=0, d_low=PTR + 8)
R(_e, d_low=PTR + 8, planes=0)
_e = "fino_fastercache_apply"
each(R, _e, "dtype", 7, 2)
nulls(_e, "cond", "d_low", "d_high", "out")
off16(_e, "cond", "d_low", "d_high", "out")
each(R, _e, "n", 0, -8)
R(_e, dtype=7, cond=0)
R(_e, cond=0, out=PTR + 8)
R(_e, out=PTR + 8, n=0)

# ---- fino_vae.hip ----
for _e in ("fino_rmsnorm_silu_cl", "fino_rmsnorm_silu_cl_f32"):
    nulls(_e, "x", "y", "gamma")
    each(R, _e, "rows", -1)
    each(R, _e, "c_valid", 0, 65)
    each(R, _e, "c_pad", 56, 68)
    off16(_e, "x", "y")
    off16(_e, "gamma", by=4)
    E(_e, rows=0)
    R(_e, x=0, y=PTR + 8)
    R(_e, rows=0, y=PTR + 8)
    R(_e, rows=0, c_valid=0)
each(R, "fino_rmsnorm_silu_cl", "dtype", 7, 2)
R("fino_rmsnorm_silu_cl", dtype=7, x=0)
each(R, "fino_rmsnorm_silu_cl_f32", "nseg", -1, 7)
R("fino_rmsnorm_silu_cl_f32", x=0, nseg=7)
R("fino_rmsnorm_silu_cl_f32", nseg=7, y=PTR + 8)
_e = "fino_softmax_rows"
each(R, _e, "dtype", 7, -1)
nulls(_e, "s")
each(R, _e, "rows", -1)
each(R, _e, "n", 0)
each(R, _e, "ld", 8)
E(_e, rows=0)
E(_e, rows=0, dtype=2)
R(_e, dtype=7, s=0)
R(_e, rows=0, s=0)
for _e in ("fino_dup_up3d_add", "fino_avg_down3d_add"):
    each(R, _e, "dtype", 7, -1)
    nulls(_e, "main_in", "x", "out")
    each(R, _e, "t_in", 0)
    each(R, _e, "factor_t", 0)
    each(R, _e, "factor_s", 0)
    R(_e, dtype=7, x=0)
R("fino_dup_up3d_add", c_in=5)
each(R, "fino_dup_up3d_add", "c_out_pad", 12)
each(R, "fino_dup_up3d_add", "c_in_pad", 12)
R("fino_dup_up3d_add", x=0, c_in=5)
R("fino_dup_up3d_add", c_in=5, c_out_pad=12)
R("fino_avg_down3d_add", c_out=5)
R("fino_avg_down3d_add", h_in=5)
R("fino_avg_down3d_add", w_in=5)
R("fino_avg_down3d_add", x=0, h_in=5)
for _e, _a, _b in (("fino_vae_unpatchify_clamp", "y", "out"), ("fino_vae_patchify", "x", "y")):
    each(R, _e, "dtype", 7, -1)
    nulls(_e, _a, _b)
    each(R, _e, "t", 0)
    each(R, _e, "h", 0)
    each(R, _e, "w", 0)
    each(R, _e, "patch", 0)
    each(R, _e, "channels", 17)
    R(_e, c_pad=8)
    R(_e, **{"dtype": 7, _a: 0})
_e = "fino_split_bf16"
nulls(_e, "x", "out")
each(R, _e, "rows", -1)
each(R, _e, "cols", 0, 12)
each(R, _e, "ldx", 56, 66)
each(R, _e, "nseg", 0, 7)
each(R, _e, "ldo", 64, 132)
each(R, _e, "planes_packed", 3, 12, 15)
off16(_e, "x", "out")
E(_e, rows=0)
R(_e, x=0, nseg=0)
R(_e, nseg=0, planes_packed=3)
R(_e, planes_packed=12, out=PTR + 8)
R(_e, out=PTR + 8, rows=0)

# ---- fino_guidance.hip ----
each(V, "fino_guider_workspace_bytes", "n", 0, -1, 1, 16384, 16385, B40, B40 + 1)
_e = "fino_guider_coefs"
each(R, _e, "dtype", 7, 2)
each(R, _e, "kind", 3, -1)
nulls(_e, "cond_pred", "uncond_pred", "g_dev", "workspace", "ab_dev")
each(R, _e, "rows", 0)
each(R, _e, "row_len", 0)
each(R, _e, "row_stride", 32)
R(_e, rows=B40, row_len=2, row_stride=2)
each(R, _e, "guidance_rescale", -0.25, 1.5)
R(_e, eta=NAN)
R(_e, norm_threshold=NAN)
R(_e, workspace=PTR + 4)
each(R, _e, "workspace_bytes", 0, 39)
R(_e, rows=1024, workspace_bytes=40)
R(_e, dtype=7, kind=3)
R(_e, kind=3, g_dev=0)
R(_e, g_dev=0, rows=0)
R(_e, rows=0, guidance_rescale=1.5)
R(_e, guidance_rescale=1.5, workspace=PTR + 4)
R(_e, workspace=PTR + 4, workspace_bytes=0)

# ---- fino_token_select.hip ----
_e = "fino_token_score"
each(R, _e, "dtype", 7, 2)
nulls(_e, "po", "score_out")
each(R, _e, "rows", 0, B31)
each(R, _e, "cols", 0)
each(R, _e, "ld", 8)
each(R, _e, "batch", 0, 65)
R(_e, dtype=7, po=0)
R(_e, po=0, rows=0)
_e = "fino_token_select"
nulls(_e, "score", "idx_out")
each(R, _e, "n", 0)
each(R, _e, "k", 0, 17)
R(_e, n=65537)
R(_e, score=0, k=0)
R(_e, n=65537, k=0)
R(_e, n=65537, k=65537)
for _e in ("fino_gather_rows", "fino_scatter_rows"):
    nulls(_e, "src", "idx", "dst")
    each(R, _e, "k", -1, B31)
    each(R, _e, "n", 0, B31)
    each(R, _e, "row_bytes", 0, 6, -4)
    R(_e, row_bytes=B31, ld_src=B31, ld_dst=B31)
    each(R, _e, "ld_src", 32, 66)
    each(R, _e, "ld_dst", 32, 66)
    off16(_e, "src", "dst", by=2)
    E(_e, k=0)
    R(_e, src=0, k=-1)
    R(_e, k=-1, row_bytes=6)
    R(_e, row_bytes=6, ld_src=4)
    R(_e, ld_src=32, dst=PTR + 2)
    R(_e, dst=PTR + 2, k=0)

# ---- fino_vae_cog.hip ----
each(V, "fino_groupnorm_workspace_bytes", "c_pad", 0, -64, 64, 2048)
_e = "fino_groupnorm_cl"
each(R, _e, "dtype", 7, 2)
nulls(_e, "x", "y", "gamma", "beta", "workspace")
each(R, _e, "t", 0)
each(R, _e, "h", 0)
each(R, _e, "w", 0)
each(R, _e, "channels", 0, 65)
each(R, _e, "c_pad", 32, 192, 4096)
each(R, _e, "groups", 0, 5)
nulls(_e, "mod_scale", "mod_shift")
each(R, _e, "tz", 0, 3)
each(R, _e, "hz", 0)
each(R, _e, "wz", 0)
R(_e, t=3, tz=1)
each(R, _e, "workspace_bytes", 0, 524799)
R(_e, workspace=PTR + 8)
R(_e, dtype=7, x=0)
R(_e, x=0, t=0)
R(_e, t=0, mod_scale=0)
R(_e, mod_scale=0, tz=0)
R(_e, tz=0, workspace_bytes=0)
_e = "fino_avg_pool_time2"
each(R, _e, "dtype", 7, 2)
nulls(_e, "x", "y")
each(R, _e, "t_in", 1, 0)
each(R, _e, "h", 0)
each(R, _e, "w", 0)
each(R, _e, "c_pad", 0, 12)
R(_e, dtype=7, x=0)
_e = "fino_vae_blend_tiles"
each(R, _e, "dtype", 7, 2)
nulls(_e, "a", "b")
for _f in ("t", "h_a", "w_a", "h_b", "w_b", "c_pad"):
    each(R, _e, _f, 0)
R(_e, c_pad=12)
each(R, _e, "axis", 2, -1)
off16(_e, "a", "b")
R(_e, w_b=8)
R(_e, axis=1, h_b=8)
each(E, _e, "extent", 0, -3)
R(_e, dtype=7, a=0)
R(_e, a=0, w_b=8)
R(_e, w_b=8, extent=0)

# ---- fino_conditions.hip ----
_e = "fino_resize_area_pad_u8"
nulls(_e, "src", "dst")
for _f in ("src_h", "src_w", "region_h", "region_w", "out_h", "out_w"):
    each(R, _e, _f, 0)
each(R, _e, "off_y", -1, 6)
each(R, _e, "off_x", -1, 6)
each(R, _e, "fill", -1, 256)
R(_e, src=0, fill=256)
_e = "fino_u8_hwc_to_chw_unit"
nulls(_e, "src", "dst")
each(R, _e, "height", 0)
each(R, _e, "width", 0)
_e = "fino_traj_paint"
nulls(_e, "points", "frame_offsets", "canvas")
each(R, _e, "frames", 0)
each(R, _e, "height", 0)
each(R, _e, "width", 0)
each(R, _e, "radius", -1)
R(_e, canvas=0, radius=-1)
_e = "fino_traj_blur_quantize"
nulls(_e, "canvas", "scratch", "out", "taps_dev")
each(R, _e, "taps", 0, 4, -1)
each(R, _e, "planes", 0)
each(R, _e, "height", 0)
each(R, _e, "width", 0)
R(_e, out=0, taps=4)

# ---- fino_lora.hip ----
_e = "fino_lora_merge"
each(R, _e, "dtype", 7, -1)
each(R, _e, "n", -1)
each(R, _e, "k", -1)
each(R, _e, "n_adapters", -1, 9)
each(R, _e, "ldw_base", 32)
each(R, _e, "ldw_out", 32)
each(E, _e, "n", 0)
each(E, _e, "k", 0)
E(_e, n=0, w_base=0, a=0)
nulls(_e, "w_base", "w_out", "a", "lda", "b", "ldb", "rank", "scale", "a0", "b0")
each(R, _e, "rank0", 0, -1)
each(R, _e, "lda0", 32)
each(R, _e, "ldb0", 4)
R(_e, dtype=2, n=B40)                                 # refused behind the validation, in front of the launch
R(_e, n_adapters=8, rank0=129, ldb0=136)
R(_e, n_adapters=8, rank0=129, ldb0=136, dtype=1)
R(_e, k=1 << 38, ldw_base=1 << 38, ldw_out=1 << 38, lda0=1 << 38)
R(_e, dtype=7, n=-1)
R(_e, n=-1, n_adapters=9)
R(_e, n_adapters=9, ldw_base=32)
R(_e, ldw_base=32, n=0)
R(_e, w_base=0, a=0)
R(_e, a=0, a0=0)
R(_e, a0=0, rank0=0)
R(_e, rank0=0, lda0=32)
R(_e, n_adapters=3, lda0=32, dtype=2, n=B40)


def _case_id(c):
    return "%s-%s" % (c[0], "+".join("%s=%s" % kv for kv in c[1].items()))


def record(lib):
    """{case id: [rc, message]} from `lib` (tools/record_row_kernels_abi.py writes it to GOLDEN)"""
    return {_case_id(c): list(_call(lib, c[0], c[1])) for c in CASES}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("entry,changes,kind", CASES, ids=[_case_id(c) for c in CASES])
def test_bad_arguments_keep_their_return_code_and_message(lib, golden, entry, changes, kind):
    rc, message = golden[_case_id((entry, changes))]
    if kind == "refused":                             # ... by a check, never by a launch that failed
        assert rc in (ARG, UNSUPPORTED) and "launch" not in message and "hipFuncSetAttribute" not in message
    elif kind == "empty":
        assert (rc, message) == (OK, None)
    assert _call(lib, entry, changes) == (rc, message)


def test_every_entry_point_of_the_eight_files_is_covered(golden):
    here = os.path.dirname(os.path.abspath(__file__))
    entries = set()
    for unit in ("elementwise", "step_cache", "vae", "guidance", "token_select", "vae_cog", "conditions", "lora"):
        text = open(os.path.join(here, "..", "frameino_amd", "csrc", "fino_%s.hip" % unit)).read()
        entries |= set(re.findall(r'extern "C" \w+ (fino_\w+)\(', text))
    assert len(entries) == 58
    assert {c[0] for c in CASES} == entries == set(DEFAULTS)
    assert len({_case_id(c) for c in CASES}) == len(CASES)
    assert set(golden) == {_case_id(c) for c in CASES}
    # every int entry point with more than one check has a case that breaks two at once
    for entry in entries - set(VALUES) - {"fino_u8_hwc_to_chw_unit"}:
        assert any(c[0] == entry and len(c[1]) >= 2 for c in CASES), entry
