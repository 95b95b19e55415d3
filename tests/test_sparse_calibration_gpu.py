"""Calibration of the sparse attention's per-head thresholds (frameino_amd/sparse_calibration.py).

Attention level: the shape and generator of tests/test_attention_tile_plan_gated_gpu.py (B = 2, H = 3, Lq = 600, Lk = 1100; seed
4335 + dh) with the structure's strength per head (1, 0.5, 0.1), so that the heads differ: the weaker the structure, the flatter
the pooled softmax and the larger the threshold a head needs.  Grid (0.5, 0.7, 0.9, 0.97), l1_bound 0.12, no gate, no forced
tiles.  The float64 restatement (tests/sparse_gate_ref.py) chooses (0.9, 0.97, 0.97) at both head dims, and every one of its
errors is at least 21 % of the bound away from it (measured: 0.284 at head_dim 128, 0.211 at 64; tests/test_sparse_gate_cpu.py
asserts the choice and MARGIN on the restatement alone).  That margin is a condition on the inputs.  What the GPU adds to an error
is several times smaller: a bf16 output rounds at 2^-9 relative, and a mask may differ from the restatement's only in tiles within
1e-3 of the threshold mass.  So the GPU's choice must equal the restatement's.

Model level: the tiny Wan model of tests/test_sparse_attention_wan_gpu.py."""
import pytest
import torch

from frameino_amd.window_attention import SparseAttentionConfig
from tests import sparse_gate_ref as G
from tests.test_attention_tile_plan_gated_gpu import HEADS
from tests.test_attention_tile_plan_gated_gpu import _inputs as _gated_inputs

GRID = (0.5, 0.7, 0.9, 0.97)
BOUND = 0.12
STRENGTH = (1.0, 0.5, 0.1)
CHOICE = (0.9, 0.97, 0.97)
MARGIN = 0.20            # smallest relative distance of a restatement error to BOUND, rounded down
SEED = 4335


def _inputs(dtype, dh, device="cpu"):
    return _gated_inputs(dtype, dh, device, strength=STRENGTH, seed=SEED)


@pytest.mark.gpu
@pytest.mark.parametrize("dh", [128, 64])
def test_attention_level_choice_equals_the_restatement(dh):
    from types import SimpleNamespace
    from frameino_amd import ops
    from frameino_amd.sparse_calibration import _Calibration, _report
    q, k, v = _inputs(torch.bfloat16, dh, "cuda")
    want = G.l1_errors(q, k, v, HEADS, GRID)
    state = _Calibration(GRID, None)
    out = state.attend(None, ops, q, k, v, HEADS, SimpleNamespace(layer=0, keep=None))
    assert torch.equal(out, ops.attention(q, k, v, HEADS))                      # the call continues with the dense output
    state.attend(None, ops, q, k, v, HEADS, SimpleNamespace(layer=0, keep=None))          # a second call adds to the same sums
    rep = _report(state, BOUND)
    err = torch.tensor(rep["error"][0], dtype=torch.float64)
    print(f"dh {dh}: GPU errors\n{err}\nrestatement\n{want}\nthresholds {rep['thresholds'][0]}; densities {rep['density'][0]}")
    assert rep["calls"] == {0: 2} and rep["thresholds"][0] == list(CHOICE) == G.choose(want, GRID, BOUND).tolist()
    for h, g in enumerate(CHOICE):
        j = GRID.index(g)
        assert err[h, j] <= BOUND and err[h, j - 1] > BOUND, (h, err[h].tolist())
    closest = float(((err - BOUND).abs() / BOUND).min())
    print(f"closest GPU error to the bound: {closest:.3f} of the bound (the restatement's margin: >= {MARGIN})")
    if closest < MARGIN / 3:
        print("NOTE: a GPU error sits closer to the bound than a third of the restatement's margin")
    dens = torch.tensor(rep["density"][0])
    assert tuple(dens.shape) == (HEADS, len(GRID)) and bool((dens[:, 1:] >= dens[:, :-1]).all()) and 0 < float(dens.min()) and float(dens.max()) < 1


@pytest.fixture(scope="module")
def tiny():
    from tests.test_sparse_attention_wan_gpu import _model
    from tests.test_window_attention_wan_gpu import _inputs as wan_inputs
    sd, _, x, txt = wan_inputs(4.0)
    return sd, x, txt, _model


@pytest.mark.gpu
def test_model_level_calibration_is_a_dense_run_and_its_config_runs(tiny):
    from frameino_amd.sparse_calibration import calibrate_sparse_attention
    from tests.test_window_attention_wan_gpu import CFG, _fwd
    sd, x, txt, _model = tiny
    dense = _model(sd, sparse=False)
    want = [_fwd(dense, x, txt[:1], id_frames=1), _fwd(dense, x, txt[1:2], id_frames=1)]
    m = _model(sd, sparse=False)
    got = []

    def run():
        assert m.is_sparse_calibrating
        got.append(_fwd(m, x, txt[:1], id_frames=1))
        got.append(_fwd(m, x, txt[1:2], id_frames=1))

    base = SparseAttentionConfig(0.9, similarity_threshold=0.05, skip_layers=())
    cfg, report = calibrate_sparse_attention(m, run, l1_bound=0.2, grid=(0.5, 0.9), base=base)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])        # calibration forwards are dense forwards
    assert not m.is_sparse_calibrating and not m.is_sparse_attention_enabled
    heads, layers = CFG["num_attention_heads"], CFG["num_layers"]
    assert sorted(cfg.head_thresholds) == list(range(layers)) and all(len(r) == heads for r in cfg.head_thresholds.values())
    assert all(t in (0.5, 0.9, 1.0) for r in cfg.head_thresholds.values() for t in r)
    assert report["calls"] == {li: 2 for li in range(layers)} and cfg.similarity_threshold == 0.05 and cfg.cdf_threshold == 0.9
    for li in range(layers):
        err = torch.tensor(report["error"][li])
        assert tuple(err.shape) == (heads, 2) and bool(torch.isfinite(err).all()) and float(err.min()) >= 0
        for h, t in enumerate(cfg.head_thresholds[li]):
            assert t == (0.5 if err[h, 0] <= 0.2 and err[h, 1] <= 0.2 else 0.9 if err[h, 1] <= 0.2 else 1.0)
    print(f"thresholds {cfg.head_thresholds}; errors {report['error']}; densities {report['density']}")
    # a skipped layer gets no thresholds
    cfg1, rep1 = calibrate_sparse_attention(m, lambda: _fwd(m, x, txt[:1], id_frames=1), l1_bound=0.2, grid=(0.5, 0.9),
                                            base=SparseAttentionConfig(0.9, skip_layers=(0,)))
    assert sorted(cfg1.head_thresholds) == [1] and rep1["calls"] == {1: 1}
    # the returned config runs
    m.enable_sparse_attention(cfg)
    out = _fwd(m, x, txt[:1], id_frames=1)
    assert bool(torch.isfinite(out).all())


@pytest.mark.gpu
def test_the_pipeline_loop_runs_eagerly_while_calibrating(golden):
    from frameino_amd.sparse_calibration import calibrate_sparse_attention
    from tests.test_window_attention_pipeline_gpu import _pipe
    pipe, args = _pipe(golden)
    pipe.use_hip_graph = False
    dense = pipe.denoise(*args)
    pipe.use_hip_graph = None                                                   # the default: eager while calibrating
    got = []
    cfg, report = calibrate_sparse_attention(pipe.transformer, lambda: got.append(pipe.denoise(*args)), l1_bound=0.1, grid=(0.5, 0.9))
    assert torch.equal(got[0], dense)
    assert sorted(cfg.head_thresholds) == list(range(len(pipe.transformer.blocks)))
    pipe.use_hip_graph = True
    with pytest.raises(RuntimeError, match="calibrated"):
        calibrate_sparse_attention(pipe.transformer, lambda: pipe.denoise(*args), l1_bound=0.1, grid=(0.5, 0.9))
    assert not pipe.transformer.is_sparse_calibrating and not pipe.transformer.is_sparse_attention_enabled
