"""First-block caching on the Wan DiT (tiny random model, 3 blocks) against the cache-disabled forward and against the
restatement in tests/step_cache_ref.py (the oracle's blocks in bf16).  Tolerance of a forward against the bf16 oracle: the one
test_wan_model_gpu.py states, rel-RMS <= 1.5e-2.  Thresholds come from the restatement's diffs with at least 20 % margin, so
the small difference between the HIP path and the oracle cannot flip a decision."""
import pytest
import torch

from frameino_amd.step_cache import FirstBlockCacheConfig
from oracle import wan_dit as W
from tests.parity import bf16_state_dict, hip_wan_model, rel_rms
from tests.step_cache_ref import FirstBlockCacheRef, relative_l1

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = dict(W.WAN22_5B_CFG, num_attention_heads=4, attention_head_dim=128, in_channels=16, out_channels=8, text_dim=256,
           ffn_dim=1024, num_layers=3)
TS = torch.tensor([811.0])


@pytest.fixture(scope="module")
def setup():
    sd = W.wan_random_state_dict(CFG, seed=11, dtype=torch.float32, std=0.04)
    g = torch.Generator().manual_seed(12)
    x = torch.randn(1, 16, 5, 16, 20, generator=g)
    dx = torch.randn(1, 16, 5, 16, 20, generator=g)
    txt = torch.randn(1, 77, 256, generator=g)
    return sd, bf16_state_dict(sd), x, dx, txt


def _model(sd, threshold=None):
    m = hip_wan_model(CFG, sd, DEV)
    if threshold is not None:
        m.enable_cache(FirstBlockCacheConfig(threshold=threshold))
    return m


def _fwd(m, ctx, x, txt, ts=TS):
    with m.cache_context(ctx):
        return m(x.to(DEV).bfloat16(), ts.to(DEV), txt.to(DEV).bfloat16(), return_dict=False)[0]


def test_threshold_zero_equals_the_uncached_forward(setup):
    sd, _, x, dx, txt = setup
    plain, cached = _model(sd), _model(sd, 0.0)
    for i, ts in enumerate((811.0, 700.0, 650.0)):
        xi, t = x + 0.1 * i * dx, torch.tensor([ts])
        assert torch.equal(_fwd(cached, "c", xi, txt, t), _fwd(plain, "c", xi, txt, t))
    assert [e[3] for e in cached.cache_log] == [True, True, True]


def test_repeated_input_skips_and_matches_the_restatement(setup):
    sd, sdb, x, _, txt = setup
    m = _model(sd, 0.05)
    ref = FirstBlockCacheRef(sdb, CFG, 0.05)
    for _ in range(2):
        out = _fwd(m, "c", x, txt)
        want = ref("c", x.bfloat16(), TS, txt.bfloat16())
        assert rel_rms(out, want) < 1.5e-2
    assert [e[3] for e in m.cache_log] == [True, False] == [e[3] for e in ref.log]
    assert m.cache_log[1][2] == 0.0


def test_the_comparison_is_against_the_last_computed_residual(setup):
    """a, b, c with diff(c, a) > threshold > diff(b, a), diff(c, b): b skips, and c computes because it is compared with a"""
    sd, sdb, x, dx, txt = setup
    ref = FirstBlockCacheRef(sdb, CFG, 0.0)
    for s in (0.5, 1.0, 2.0, 0.25):
        a, b, c = x, x + 0.5 * s * dx, x + s * dx
        ra, rb, rc = (ref.head_residual(v.bfloat16(), TS, txt.bfloat16()) for v in (a, b, c))
        d_ba, d_cb, d_ca = relative_l1(rb, ra), relative_l1(rc, rb), relative_l1(rc, ra)
        lo, hi = max(d_ba, d_cb), d_ca
        if hi > 1.2 * 1.2 * lo:
            break
    assert hi > 1.44 * lo, (d_ba, d_cb, d_ca)
    thr = (lo * hi) ** 0.5                                  # >= 20 % from both sides
    m = _model(sd, thr)
    ref = FirstBlockCacheRef(sdb, CFG, thr)
    for v in (a, b, c):
        out = _fwd(m, "c", v, txt)
        assert rel_rms(out, ref("c", v.bfloat16(), TS, txt.bfloat16())) < 1.5e-2
    assert [e[3] for e in m.cache_log] == [True, False, True] == [e[3] for e in ref.log]


def test_a_batch_under_one_context_decides_jointly(setup):
    """batch 2 under one context: one decision over both samples.  Sample 0 repeats, sample 1 changes: the joint diff is below
    the threshold although sample 1's own diff is above it -- both skip"""
    sd, sdb, x, dx, txt = setup
    ref = FirstBlockCacheRef(sdb, CFG, 0.0)
    x1, x1b = x + 0.3 * dx, x - 0.5 * dx
    r0, r1, r1b = (ref.head_residual(v.bfloat16(), TS, txt.bfloat16()) for v in (x, x1, x1b))
    joint = relative_l1(torch.cat([r0, r1b]), torch.cat([r0, r1]))
    alone = relative_l1(r1b, r1)
    assert alone > 1.44 * joint, (joint, alone)
    thr = (joint * alone) ** 0.5
    m = _model(sd, thr)
    ref = FirstBlockCacheRef(sdb, CFG, thr)
    t2 = txt.repeat(2, 1, 1)
    for xs in (torch.cat([x, x1]), torch.cat([x, x1b])):
        out = _fwd(m, "c", xs, t2)
        assert rel_rms(out, ref("c", xs.bfloat16(), TS, t2.bfloat16())) < 1.5e-2
    assert [(e[0], e[3]) for e in m.cache_log] == [("c", True), ("c", False)] == [(e[0], e[3]) for e in ref.log]


def test_contexts_are_independent_and_a_context_is_required(setup):
    sd, _, x, dx, txt = setup
    m = _model(sd, 0.05)
    _fwd(m, "cond", x, txt)
    _fwd(m, "uncond", x + dx, txt)                          # its own state: computes
    _fwd(m, "cond", x, txt)                                 # same as cond's last computed step: skips
    assert [(e[0], e[1], e[3]) for e in m.cache_log] == [("cond", 0, True), ("uncond", 0, True), ("cond", 1, False)]
    with pytest.raises(ValueError, match="No context is set"):
        m(x.to(DEV).bfloat16(), TS.to(DEV), txt.to(DEV).bfloat16(), return_dict=False)
    m.disable_cache()
    m(x.to(DEV).bfloat16(), TS.to(DEV), txt.to(DEV).bfloat16(), return_dict=False)     # no cache: no context needed


def test_mxfp8_linears_at_threshold_zero_equal_mxfp8_without_the_cache(setup):
    sd, _, x, dx, txt = setup
    plain, cached = _model(sd).enable_mxfp8_linears(), _model(sd, 0.0).enable_mxfp8_linears()
    for i in range(2):
        assert torch.equal(_fwd(cached, "c", x + 0.2 * i * dx, txt), _fwd(plain, "c", x + 0.2 * i * dx, txt))
    assert [e[3] for e in cached.cache_log] == [True, True]
