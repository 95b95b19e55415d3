"""Region-adaptive sampling on the Wan DiT (enable_cache(RegionAdaptiveSamplingConfig(...))) against the cache-disabled model and
the restatement in tests/ras_ref.py.  The tiny model of tests/test_window_attention_wan_gpu.py (4 heads x 128, 2 blocks), 12
latent frames of 9 x 11 = 99 tokens (L = 1188), batch 2 as the pipeline's CFG batch (two prompts, two timesteps), the last frame
an ID frame.

Tolerance of a partial forward: the dense forward's own rel-RMS error against the same restatement, measured in the same test, times
1.5 -- as tests/test_sparse_attention_fp8_wan_gpu.py allows for the same reason: the partial forward shares every rounding point
with the dense one but the summation order (its GEMMs run on other row tiles, its attention walks the keys of the planes)."""
import math

import pytest
import torch

from frameino_amd.step_cache import RegionAdaptiveSamplingConfig, ras_active_count
from oracle import wan_dit as W
from tests import ras_ref as R
from tests.parity import bf16_state_dict, hip_wan_model, record, rel_rms

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = dict(W.WAN22_5B_CFG, num_attention_heads=4, attention_head_dim=128, in_channels=16, out_channels=8, text_dim=256,
           ffn_dim=1024, num_layers=2)
FRAMES, TPF = 12, 99
L = FRAMES * TPF
TS = torch.tensor([811.0, 650.0])
CTX = ("cond", "uncond")


@pytest.fixture(scope="module")
def setup():
    """weights, three different latents and the restatement's full forwards of the first two (computed once, on the CPU, in
    bf16) with their head rows and per-layer K / V"""
    sd = W.wan_random_state_dict(CFG, seed=11, dtype=torch.float32, std=0.04)
    sdb = bf16_state_dict(sd)
    g = torch.Generator().manual_seed(12)
    xs = [torch.randn(2, 16, FRAMES, 18, 22, generator=g) + torch.randn(2, 16, FRAMES, 1, 1, generator=g) for _ in range(3)]
    txt = torch.randn(2, 77, 256, generator=g)
    ref = [R.ras_forward(sdb, CFG, x.bfloat16(), TS, txt.bfloat16()) for x in xs[:2]]
    return sd, sdb, xs, txt, ref


def _model(sd, mx=False, **cfg):
    m = hip_wan_model(CFG, sd, DEV)
    if mx:
        m.enable_mxfp8_linears()
    if cfg:
        m.enable_cache(RegionAdaptiveSamplingConfig(**cfg))
    return m


def _fwd(m, x, txt, **kw):
    with m.cache_context("cfg"):
        return m(x.to(DEV, torch.bfloat16), TS.to(DEV), txt.to(DEV, torch.bfloat16), return_dict=False,
                 **({"_cache_contexts": CTX} if m.is_cache_enabled else {}), **kw)[0]


def _rows(pred):
    """a prediction [b, C, F, H, W] as head rows [b, L, C * 4] (the inverse of unpatchify, patch (1, 2, 2))"""
    b, c, f, h, w = pred.shape
    return pred.reshape(b, c, f, 1, h // 2, 2, w // 2, 2).permute(0, 2, 4, 6, 3, 5, 7, 1).reshape(b, f * (h // 2) * (w // 2), -1)


def test_full_forwards_and_an_all_rows_list_are_the_uncached_forward_bit_for_bit(setup):
    sd, _, xs, txt, _ = setup
    plain = _model(sd)
    want = [_fwd(plain, x, txt) for x in xs]
    m = _model(sd, sample_ratio=0.4, warmup_steps=2, full_step_interval=50)
    assert torch.equal(_fwd(m, xs[0], txt), want[0])
    assert torch.equal(_fwd(m, xs[1], txt), want[1])
    assert torch.equal(_fwd(m, xs[2], txt, _active_rows=torch.arange(L)), want[2])
    assert m.cache_log == [(c, s, f, L) for s, f in ((0, True), (1, True), (2, False)) for c in CTX]
    # sample_ratio = 1: every forward is full
    m = _model(sd, sample_ratio=1.0, warmup_steps=1)
    for x, w in zip(xs, want):
        assert torch.equal(_fwd(m, x, txt), w)
    assert all(e[2] for e in m.cache_log)


@pytest.mark.parametrize("mx", [False, True], ids=["bf16", "mxfp8"])
def test_a_partial_forward_over_a_scattered_list(setup, mx):
    """measured on an MI355X (rel-RMS of the active rows against the restatement / the dense forward's own error against it):
    bf16 3.89e-3 / 3.94e-3, MXFP8 2.07e-2 / 2.09e-2; the bound is 1.5 x the dense error of the same run"""
    sd, sdb, xs, txt, ref = setup
    g = torch.Generator().manual_seed(5)
    idx = torch.randperm(L, generator=g)[:R.LIST_ROWS].sort().values
    assert idx.shape[0] == R.LIST_ROWS and R.LIST_ROWS % 64 and int(idx[0]) < 99 and int(idx[-1]) >= L - 99
    m = _model(sd, mx=mx, sample_ratio=0.4, warmup_steps=2, full_step_interval=50)
    first, second = _fwd(m, xs[0], txt), _fwd(m, xs[1], txt)              # two full forwards on different inputs
    out = _fwd(m, xs[2], txt, _active_rows=idx)
    inactive = torch.ones(L, dtype=torch.bool)
    inactive[idx] = False
    got, prev = _rows(out).cpu(), _rows(second).cpu()
    assert torch.equal(got[:, inactive], prev[:, inactive])               # inactive rows: the previous forward's, bit for bit
    assert not torch.equal(prev[:, inactive], _rows(first).cpu()[:, inactive])
    # the restatement: the list over the stale K / V and head rows of the second full forward
    want, _, _ = R.ras_forward(sdb, CFG, xs[2].bfloat16(), TS, txt.bfloat16(), idx, ref[1][2], ref[1][1])
    err = rel_rms(got[:, idx], _rows(want)[:, idx])
    dense = rel_rms(second, ref[1][0])                                    # the dense tiny forward's own error, same restatement
    print(f"partial forward ({'mxfp8' if mx else 'bf16'}): active rows rel-RMS {err:.3e}, dense forward {dense:.3e}, "
          f"bound {1.5 * dense:.3e}")
    record(f"test_ras_wan_gpu::partial_forward[{'mxfp8' if mx else 'bf16'}]", "active_rows_rel_rms", err, 1.5 * dense)
    record(f"test_ras_wan_gpu::partial_forward[{'mxfp8' if mx else 'bf16'}]", "dense_forward_rel_rms", dense, 1.5 * dense)
    assert err < 1.5 * dense
    # ... and it is not the dense forward of that input
    far = rel_rms(got[:, idx], _rows(_fwd(_model(sd, mx=mx), xs[2], txt)).cpu()[:, idx])
    print(f"   against the dense forward of the same input: {far:.3e}")
    assert m.cache_log[-2:] == [("cond", 2, False, R.LIST_ROWS), ("uncond", 2, False, R.LIST_ROWS)]


def test_the_models_own_list_is_the_restatements(setup):
    sd, _, xs, txt, _ = setup
    la = ras_active_count(0.4, L - 99)
    m = _model(sd, sample_ratio=0.4, warmup_steps=1, full_step_interval=50)
    live = (0, L - 99)                                                    # the ID frame's prediction is dropped by the loop
    first = _fwd(m, xs[0], txt, live_rows=live)
    st = m._step_cache_states[CTX]
    po = st.po.clone()
    assert torch.equal(po.view(2, L, -1)[:, :L - 99], _rows(first)[:, :L - 99])
    elig = torch.zeros(L, dtype=torch.uint8)
    elig[:L - 99] = 1
    counters = torch.zeros(L, dtype=torch.int32)
    for step, x in enumerate(xs[1:], 1):
        idx, counters = R.select_ref(R.score_ref(st.po.cpu(), 2, counters, 0.1, elig), la, counters)
        _fwd(m, x, txt, live_rows=live)
        assert torch.equal(st.idx.cpu(), idx) and torch.equal(st.counters.cpu(), counters), step
        assert int(st.idx.max()) < L - 99                                 # the ID frame never joins the list
    assert m.cache_log[-1] == ("uncond", 2, False, la)


def test_starvation_brings_the_quietest_row_onto_the_list_when_the_formula_says():
    """sample_ratio = 0.25 on rows whose raw scores do not move (the same kept prediction every step).  The formula: a row that
    has sat out k steps scores s * exp(starvation_scale * k), so the quietest row, which sits out from the start, joins at the
    first step k at which s_q * exp(scale * k) reaches that step's threshold (the La-th largest score, every other row boosted
    by its own counter) -- the restatement walks the steps and says which k that is; the kernels must put the row on the list
    at that step and at no earlier one.  It cannot be before n / La - 1 steps (every row that has sat out as long outranks
    it) nor after the step at which it outscores the largest raw score boosted by as many sit-outs as a round of all rows
    takes."""
    from frameino_amd import ops
    n, la, scale = L, ras_active_count(0.25, L), 0.1
    g = torch.Generator().manual_seed(9)
    po = torch.randn(n, 32, generator=g) * torch.linspace(1.0, 1.2, n)[torch.randperm(n, generator=g)][:, None]
    quiet = 321
    po[quiet] *= 0.4
    po = po.bfloat16()
    base = R.score_ref(po)
    assert int(base.argmin()) == quiet
    counters_ref = torch.zeros(n, dtype=torch.int32)
    want_step = None
    for step in range(40):
        score = R.score_ref(po, 1, counters_ref, scale)
        idx, counters_ref = R.select_ref(score, la, counters_ref)
        crossed = float(base[quiet]) * math.exp(scale * step) >= float(score[idx.long()].min())
        assert crossed == (quiet in idx.tolist())                         # the formula against that step's threshold
        if crossed:
            want_step = step
            break
    rounds = -(-n // la)
    assert want_step is not None and rounds - 1 <= want_step <= R.starvation_steps(float(base[quiet]), float(base.max()), scale) + rounds
    counters, pod = torch.zeros(n, dtype=torch.int32, device=DEV), po.to(DEV)
    for step in range(want_step + 1):
        idx = ops.token_select(ops.token_score(pod, counters=counters, starvation_scale=scale), la, counters=counters)
        assert (quiet in idx.tolist()) == (step == want_step), step
    assert int(counters[quiet]) == 0


def test_always_active_rows_are_on_every_list_and_the_forward_sees_its_refusals(setup):
    sd, _, xs, txt, _ = setup
    mask = torch.zeros(L, dtype=torch.bool)
    mask[[3, 400, 401, 1100]] = True
    m = _model(sd, sample_ratio=0.25, warmup_steps=1, full_step_interval=50, always_active=mask)
    _fwd(m, xs[0], txt)
    _fwd(m, xs[1], txt)
    idx = m._step_cache_states[CTX].idx.tolist()
    assert len(idx) == ras_active_count(0.25, L) and all(r in idx for r in (3, 400, 401, 1100))
    # what only the forward can see: a mask of another length, fp8 attention switched on behind the cache's back, the hook
    # without planes
    m.disable_cache()
    m.enable_cache(RegionAdaptiveSamplingConfig(always_active=mask[:100]))
    with pytest.raises(ValueError, match="always_active has 100 entries"):
        _fwd(m, xs[0], txt)
    m.disable_cache()
    m.enable_cache(RegionAdaptiveSamplingConfig())
    with pytest.raises(RuntimeError, match="K / V planes of a full forward"):
        _fwd(m, xs[0], txt, _active_rows=torch.arange(10))
    m.fp8_attention = True
    with pytest.raises(NotImplementedError, match="fp8 attention.*region-adaptive sampling"):
        _fwd(m, xs[0], txt)
    m.fp8_attention = False
    assert math.isfinite(float(_fwd(m, xs[0], txt).float().abs().max()))
