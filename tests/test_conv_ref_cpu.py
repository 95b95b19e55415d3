"""The float64 convolution reference and the derived per-element bound of tests/conv_ref.py, checked without a GPU:
  * conv_ref64 equals a naive nested-loop convolution on one tiny case per feature (causal pad, stride, up2x, far-edge pad);
  * the bound has teeth: on every geometry of the edge table, four gather mistakes of the kind an implicit-GEMM kernel can make
    -- applied to the REFERENCE alone -- each put at least one element outside the bound, while the honest reference rounded
    once to T stays inside it.  This is the evidence that tests/test_conv3d_edges_gpu.py would fail on a subtly wrong kernel;
  * expected_loop restates conv3d_impl's loop choice and returns what the table claims for every row."""
import pytest
import torch

from tests.conv_ref import (BM, GEOMS, SPLIT_NPROD, SPLIT_ROWS, bound, conv_ref64, expected_loop, make_operands, out_thw,
                            taps)

DTYPES = [torch.bfloat16, torch.float16]


# ------------------------------------------------------------------------------------------------ reference vs nested loops
def _naive(x, w, b, kernel, stride, pad, up, out):
    """the definition, one multiply at a time (float64); taps outside the (upsampled) input contribute zero"""
    t_in, h_in, w_in, cin = x.shape
    kt, kh, kw = kernel
    hl, wl = (2 * h_in, 2 * w_in) if up else (h_in, w_in)
    y = torch.zeros(*out, w.shape[0], dtype=torch.float64)
    w5 = w.double().reshape(w.shape[0], kt, kh, kw, cin)
    for t in range(out[0]):
        for h in range(out[1]):
            for v in range(out[2]):
                for co in range(w.shape[0]):
                    s = float(b[co])
                    for dt in range(kt):
                        for dh in range(kh):
                            for dw in range(kw):
                                ti, hi, wi = t * stride[0] + dt - pad[0], h * stride[1] + dh - pad[1], v * stride[2] + dw - pad[2]
                                if not (0 <= ti < t_in and 0 <= hi < hl and 0 <= wi < wl):
                                    continue
                                if up:
                                    hi, wi = hi // 2, wi // 2
                                for ci in range(cin):
                                    s += float(x[ti, hi, wi, ci]) * float(w5[co, dt, dh, dw, ci])
                    y[t, h, v, co] = s
    return y


@pytest.mark.parametrize("name,kernel,stride,pad,up,thw,out", [
    ("causal pad", (3, 3, 3), (1, 1, 1), (2, 1, 1), False, (3, 3, 4), (3, 3, 4)),
    ("stride", (3, 1, 1), (2, 1, 1), (0, 0, 0), False, (7, 2, 3), (3, 2, 3)),
    ("up2x", (1, 3, 3), (1, 1, 1), (0, 1, 1), True, (2, 3, 2), (2, 6, 4)),
    ("far-edge pad", (1, 3, 3), (1, 2, 2), (0, 0, 0), False, (2, 4, 6), (2, 2, 3)),
])
def test_conv_ref64_equals_the_nested_loop_definition(name, kernel, stride, pad, up, thw, out):
    gen = torch.Generator().manual_seed(3)
    cin, cout = 3, 2
    x = torch.randn(*thw, cin, generator=gen)
    w = torch.randn(cout, kernel[0] * kernel[1] * kernel[2] * cin, generator=gen)
    b = torch.randn(cout, generator=gen)
    ref, s = conv_ref64(x, w, b, kernel, stride, pad, up, out)
    want = _naive(x, w, b, kernel, stride, pad, up, out)
    assert (ref - want).abs().max().item() < 1e-12, name
    want_s = _naive(x.abs(), w.abs(), b.abs(), kernel, stride, pad, up, out)
    assert (s - want_s).abs().max().item() < 1e-12 and (s >= ref.abs() - 1e-12).all(), name


# ------------------------------------------------------------------------------------------------ mutants
def _gather_conv(x, w, b, g, mutant=None):
    """the convolution as the kernels see it -- per tap, a gather of one A row per output position, then a GEMM -- in float64,
    with one of the mistakes below applied.  Returns y [To, Ho, Wo, Cout]."""
    t_in, h_in, w_in = g.thw
    to, ho, wo = out_thw(g)
    kt, kh, kw = g.kernel
    st, sh, sw = g.stride
    pt, ph, pw = g.pad
    hl, wl = (2 * h_in, 2 * w_in) if g.up else (h_in, w_in)
    hw = ho * wo
    m = torch.arange(to * hw)
    t, h, v = m // hw, (m % hw) // wo, m % wo
    x64 = x.double()
    w3 = w.double().reshape(g.cout_pad, taps(g), g.cin_pad)
    y = b.double()[None].repeat(m.numel(), 1)
    tile1 = (m >= BM) & (m < 2 * BM)
    base1 = (BM // hw) * st - pt                                     # first input frame of M tile 1 before the max(0, .)
    m_star = m.numel() // 2                                          # mutant (a): one output position, one tap, 8 channels
    tap_star = ((kt - 1) * kh + min(ph, kh - 1)) * kw + min(pw, kw - 1)
    for tap in range(taps(g)):
        dt, dh, dw = tap // (kh * kw), (tap // kw) % kh, tap % kw
        ti, hi, wi = t * st + dt - pt, h * sh + dh - ph, v * sw + dw - pw
        if mutant == "b" and dw == kw - 1:                           # the last kernel column reads one pixel to the right
            wi = wi + 1
        ok = (ti >= 0) & (ti < t_in) & (hi >= 0) & (hi < hl) & (wi >= 0) & (wi < wl)
        if mutant == "c" and pt > 0:                                 # time taps in front of the clip clamp to frame 0
            ok = (ti < t_in) & (hi >= 0) & (hi < hl) & (wi >= 0) & (wi < wl)
        if mutant == "d" and base1 < 0 and bool(tile1.any()):        # tile 1 addresses relative to its unclamped base
            ti = torch.where(tile1, ti - base1, ti)
            ok = ok & (ti < t_in)
        ti, hi, wi = ti.clamp(0, t_in - 1), hi.clamp(0, hl - 1), wi.clamp(0, wl - 1)
        if g.up:
            hi, wi = hi // 2, wi // 2
        a = x64[ti, hi, wi] * ok[:, None]
        if mutant == "a" and tap == tap_star:                        # one 16-byte DMA granule of one row is lost
            assert bool(ok[m_star]), "mutant (a) needs a tap inside the input"
            a[m_star, :8] = 0
        y += a @ w3[:, tap].T
    return y.reshape(to, ho, wo, g.cout_pad)


def _ratio(diff, bnd):
    """max |diff| / bound; an element with bound 0 (pad channel: ref = S = 0) must have diff 0"""
    r = torch.where(bnd > 0, diff / bnd.clamp_min(1e-300), torch.where(diff > 0, float("inf"), 0.0).double())
    return r.max().item()


_CACHE = {}


def _case(g):
    if g.id not in _CACHE:
        x, w, b, _ = make_operands(g)
        _CACHE[g.id] = (x, w, b) + conv_ref64(x, w, b, g.kernel, g.stride, g.pad, g.up, out_thw(g))
    return _CACHE[g.id]


@pytest.mark.parametrize("g", GEOMS, ids=[g.id for g in GEOMS])
def test_the_bound_rejects_every_mutant_and_accepts_the_rounded_reference(g):
    x, w, b, ref, s = _case(g)
    k = taps(g) * g.cin_pad
    honest = _gather_conv(x, w, b, g)
    assert _ratio((honest - ref).abs(), 1e-12 * s + 1e-300) <= 1, "the gather formulation is the same convolution"
    bounds = [(str(dt).split(".")[1], bound(ref, s, k, dt)) for dt in DTYPES]
    if g.id in SPLIT_ROWS:      # (the split bound, on the same operands: the drop term is a property of the formula, not of the data)
        bounds += [(f"split{p}", bound(ref, s, k * SPLIT_NPROD[p], torch.float32, planes=p)) for p in (2, 3)]
    for dt in DTYPES:
        r = _ratio((ref.to(dt).double() - ref).abs(), bound(ref, s, k, dt))
        print(f"{g.id:16s} honest  {str(dt).split('.')[1]:8s} worst |round(ref) - ref| / bound = {r:.3f}")
        assert r < 1, (g.id, dt, r)
    for mutant in "abcd":
        y = _gather_conv(x, w, b, g, mutant)
        if not bool((y != honest).any()):   # the mutation leaves this geometry's mathematics alone (table in the next test)
            print(f"{g.id:16s} mutant ({mutant}) does not apply")
            continue
        for name, bnd in bounds:
            r = _ratio((y - ref).abs(), bnd)
            print(f"{g.id:16s} mutant ({mutant}) {name:8s} worst |mutant - ref| / bound = {r:.1f}")
            assert r > 1, (g.id, mutant, name, r)


def test_each_mutant_applies_where_the_geometry_says():
    """(a) everywhere; (b) everywhere but one-pixel (W = 1: the last kernel column and its right neighbour are both padding);
    (c) wherever pt > 0; (d) only where M tile 1 exists and its unclamped base is negative: causal-midrow"""
    for g in GEOMS:
        x, w, b, _, _ = _case(g)
        honest = _gather_conv(x, w, b, g)
        want = {"a": True, "b": g.id != "one-pixel", "c": g.pad[0] > 0, "d": g.id == "causal-midrow"}
        for mutant in "abcd":
            assert bool((_gather_conv(x, w, b, g, mutant) != honest).any()) == want[mutant], (g.id, mutant)


# ------------------------------------------------------------------------------------------------ loop predictor
@pytest.mark.parametrize("g", GEOMS, ids=[g.id for g in GEOMS])
def test_expected_loop_matches_the_table(g):
    assert expected_loop(g) == g.loop
    assert expected_loop(g, tune=1) == "one_barrier" and expected_loop(g, pingpong_env=False) == "one_barrier"
    for planes in (2, 3):       # the split conv runs where the ping-pong loop does, and refuses elsewhere (narrow-N)
        if g.id in SPLIT_ROWS:
            assert expected_loop(g, planes) == "pingpong"
    if g.id == "narrow-N":
        assert expected_loop(g, 3) == "one_barrier"


def test_expected_loop_thresholds():
    """each clause of the condition on its own, at the value where it flips"""
    g = GEOMS[0]
    assert expected_loop(g._replace(cout_pad=96)) == "pingpong" and expected_loop(g._replace(cout_pad=72)) == "one_barrier"
    assert expected_loop(g._replace(thw=(300, 1, 1))) == "one_barrier"                          # t_span = 256
    assert expected_loop(g._replace(thw=(300, 1, 2), pad=(2, 1, 1))) == "pingpong"              # hw = 2: t_span = 129
    wide = g._replace(kernel=(1, 1, 1), pad=(0, 0, 0), thw=(1, 1, 4096))
    assert expected_loop(wide) == "one_barrier" and expected_loop(wide._replace(thw=(1, 1, 4095))) == "pingpong"
    # (t_span * st + kt) * H * W * c_in_pad * 2 bytes against 2 GiB: hw_out = 1024 * 1024 -> t_span = 2, (2 + 3) frames
    big = g._replace(thw=(4, 1024, 1024), cin_pad=256)                                          # 5 * 2^20 * 512 B = 2.5 GiB
    assert expected_loop(big) == "one_barrier" and expected_loop(big._replace(cin_pad=128)) == "pingpong"
