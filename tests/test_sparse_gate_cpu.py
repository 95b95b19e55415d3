"""The similarity gate, the per-head thresholds and the calibration of the dynamic block-sparse self-attention (DESIGN.md section
6k): everything that needs no GPU -- the config's new fields and their JSON form, the host path's decisions with a recording
stand-in for `ops`, the C ABI's surface, the float64 restatement's own hand cases, and the conditions on the inputs of the GPU
tests (tests/test_attention_tile_plan_gated_gpu.py, tests/test_sparse_calibration_gpu.py), asserted on the restatement alone."""
import ctypes
import dataclasses
import os
from types import SimpleNamespace

import pytest
import torch

from frameino_amd.window_attention import SparseAttentionConfig, window_attention_runs_eagerly
from tests import sparse_attn_ref as R
from tests import sparse_gate_ref as G


def _tiny_model(layers=2):
    from frameino_amd.transformer_wan import WanTransformer3DModel
    return WanTransformer3DModel(num_attention_heads=2, attention_head_dim=64, in_channels=4, out_channels=4, text_dim=32,
                                 freq_dim=32, ffn_dim=64, num_layers=layers)


def test_config_validation_of_the_new_fields():
    c = SparseAttentionConfig()
    assert c.similarity_threshold is None and c.head_thresholds is None
    assert [f.name for f in dataclasses.fields(c)][:5] == ["cdf_threshold", "window_frames", "sink_frames", "skip_layers", "keep_masks"]
    assert [f.name for f in dataclasses.fields(c)][5:] == ["similarity_threshold", "head_thresholds"]
    c = SparseAttentionConfig(0.5, 0, (0,), (), False, 1, {1: [0.5, 2], 0: (0.25, 0.75)})          # positional, as before + two
    assert c.similarity_threshold == 1.0 and c.head_thresholds == {1: (0.5, 2.0), 0: (0.25, 0.75)}
    assert c.key() == SparseAttentionConfig(0.9).key()                                            # key() is unchanged
    for bad in (dict(similarity_threshold=0), dict(similarity_threshold=-0.1), dict(similarity_threshold=1.01),
                dict(similarity_threshold=float("nan")), dict(similarity_threshold="0.5"), dict(similarity_threshold=True),
                dict(head_thresholds=[(0.5, 0.5)]), dict(head_thresholds={-1: (0.5,)}), dict(head_thresholds={"0": (0.5,)}),
                dict(head_thresholds={0: 0.5}), dict(head_thresholds={0: ()}), dict(head_thresholds={0: (0.5, 0.0)}),
                dict(head_thresholds={0: (0.5, float("inf"))}), dict(head_thresholds={0: (0.5, float("nan"))}),
                dict(head_thresholds={0: (0.5, "1")}), dict(head_thresholds={True: (0.5,)})):
        with pytest.raises(ValueError):
            SparseAttentionConfig(**bad)
    m = _tiny_model()
    with pytest.raises(ValueError, match="layer 2"):
        m.enable_sparse_attention(SparseAttentionConfig(0.5, head_thresholds={2: (0.5, 0.5)}))
    with pytest.raises(ValueError, match="3 entries"):
        m.enable_sparse_attention(SparseAttentionConfig(0.5, head_thresholds={1: (0.5, 0.5, 0.5)}))
    assert not m.is_sparse_attention_enabled
    m.enable_sparse_attention(SparseAttentionConfig(0.5, similarity_threshold=0.3, head_thresholds={1: (0.5, 1.0)}))
    assert m.is_sparse_attention_enabled and m.sparse_attention_similarity() == {} and not m.is_sparse_calibrating


def test_json_round_trip(tmp_path):
    from frameino_amd.sparse_calibration import load_sparse_thresholds, save_sparse_thresholds
    import json
    c = SparseAttentionConfig(0.8, window_frames=1, sink_frames=(0, -1), skip_layers=(3,), keep_masks=True,
                              similarity_threshold=0.3, head_thresholds={0: (0.5, 0.95), 7: (1.0, 0.6)})
    path = str(tmp_path / "thr.json")
    save_sparse_thresholds(path, c)
    d = json.load(open(path))
    assert d["head_thresholds"] == {"0": [0.5, 0.95], "7": [1.0, 0.6]} and d["similarity_threshold"] == 0.3
    back = load_sparse_thresholds(path)
    assert back == dataclasses.replace(c, keep_masks=False)
    save_sparse_thresholds(path, SparseAttentionConfig(0.7))
    assert load_sparse_thresholds(path) == SparseAttentionConfig(0.7)
    open(path, "w").write("{}")
    with pytest.raises(ValueError, match="save_sparse_thresholds"):
        load_sparse_thresholds(path)


def _fake_ops_bytes():
    plain = lambda b, h, lq, lk, dh: 4 * b * h * dh * (-(-lq // 256) + -(-lk // 64))                        # noqa: E731
    gated = lambda b, h, lq, lk, dh: plain(b, h, lq, lk, dh) + 4 * b * h * (-(-lq // 256) + -(-lk // 64))   # noqa: E731
    return SimpleNamespace(attention_tile_plan_bytes=plain, attention_tile_plan_gated_bytes=gated)


def test_the_dense_shortcut_with_head_thresholds():
    m = _tiny_model(layers=3)
    m.ops = _fake_ops_bytes()
    ws = SimpleNamespace()
    # cdf_threshold >= 1 alone plans nothing; with a table the named layers are planned, the others are dense
    m.enable_sparse_attention(SparseAttentionConfig(1.0))
    assert m._sparse_begin(12, 99, 0, "cpu", ws, 1, 2, 64) is None
    m.enable_sparse_attention(SparseAttentionConfig(1.0, head_thresholds={1: (0.5, 1.0)}))
    sp = m._sparse_begin(12, 99, 0, "cpu", ws, 1, 2, 64)
    L = 12 * 99
    assert sp is not None and sp.dense == frozenset({0, 2})
    assert m._sparse_tiles(sp, 0, (0, L)) is None and m._sparse_tiles(sp, 2, (0, L)) is None
    t1 = m._sparse_tiles(sp, 1, (0, L))
    assert t1.layer == 1 and t1.cdf_heads.tolist() == [0.5, 1.0] and t1.cdf_heads.dtype == torch.float32
    assert m._sparse_tiles(sp, 1, (0, L)).cdf_heads is t1.cdf_heads                     # the table cache
    assert sum(k[0] == "sparse_cdf" for k in m._rope_cache) == 1
    assert not hasattr(sp, "similarity")
    assert sp.workspace.numel() * 4 == m.ops.attention_tile_plan_bytes(1, 2, L, L, 64)  # no gate: the ungated size
    # a layer whose heads are all >= 1 takes the dense call; a layer that is not named uses the scalar
    m.enable_sparse_attention(SparseAttentionConfig(0.5, head_thresholds={0: (1.0, 2.0), 2: (0.6, 0.7)}, skip_layers=(2,)))
    sp = m._sparse_begin(12, 99, 0, "cpu", ws, 1, 2, 64)
    assert sp.dense == frozenset({0}) and m._sparse_tiles(sp, 0, (0, L)) is None
    t1 = m._sparse_tiles(sp, 1, (0, L))
    assert t1 is not None and t1.cdf_heads is None and sp.cdf == 0.5
    assert m._sparse_tiles(sp, 2, (0, L)) is None                                       # skip_layers wins
    m.reset_caches()
    assert not any(k[0] in ("sparse", "sparse_cdf") for k in m._rope_cache)
    # the gate: the workspace holds the similarities too
    ws = SimpleNamespace()
    m.enable_sparse_attention(SparseAttentionConfig(0.5, similarity_threshold=0.25))
    sp = m._sparse_begin(12, 99, 0, "cpu", ws, 1, 2, 64)
    assert sp.similarity == 0.25 and not hasattr(sp, "cdf_heads") and not hasattr(sp, "dense")
    assert sp.workspace.numel() * 4 == m.ops.attention_tile_plan_gated_bytes(1, 2, L, L, 64)
    # a forward whose head count is not the table's is refused before anything is launched
    m.enable_sparse_attention(SparseAttentionConfig(0.5, head_thresholds={0: (0.5, 0.5)}))
    with pytest.raises(ValueError, match="2 entries"):
        m._sparse_begin(12, 99, 0, "cpu", ws, 1, 3, 64)


class _Ops:
    """records the plan's keywords exactly as `_attend_tiles` passes them"""

    def __init__(self):
        self.calls = []

    def attention_tile_plan(self, q, k, heads, cdf, **kw):
        self.calls.append(("attention_tile_plan", (q, k, heads, cdf), kw))
        kw["out"].fill_(7)
        return kw["out"]

    def attention_tiles(self, *a, **kw):
        self.calls.append(("attention_tiles", a, kw))
        return "attention_tiles"


def test_attend_tiles_names_the_new_keywords_only_when_they_are_set():
    m = _tiny_model()
    q, k, v = torch.zeros(2, 600, 128), torch.zeros(2, 1100, 128), torch.zeros(2, 1100, 128)
    table = torch.zeros(3, 3, 2, dtype=torch.int32)
    old_kw = {"keep_ranges", "scale", "out", "workspace"}

    def sp_(**extra):
        nq, nt = 3, 18
        ws = torch.arange(2 * 2 * (nq + nt) * 64 + 2 * 2 * (nq + nt), dtype=torch.float32)
        return SimpleNamespace(keep=lambda q_rows: table, skip=frozenset(), cdf=0.5, words=1, lk=1100,
                               mask=torch.zeros(2 * 2 * 3, dtype=torch.int32), workspace=ws, keep_masks=True, **extra)

    m.enable_sparse_attention(SparseAttentionConfig(0.5, keep_masks=True, similarity_threshold=0.25))
    o = _Ops()
    m._attend(o, q, k, v, 2, fp8=False, tiles=m._sparse_tiles(sp_(), 0, (0, 600)), scale=-1.0)
    assert set(o.calls[0][2]) == old_kw and m._sparse_sims == {}                       # as before this change
    heads = torch.tensor([0.5, 0.9])
    o = _Ops()
    m._attend(o, q, k, v, 2, fp8=False, tiles=m._sparse_tiles(sp_(cdf_heads=lambda li: heads), 0, (0, 600)))
    assert set(o.calls[0][2]) == old_kw | {"cdf_heads"} and o.calls[0][2]["cdf_heads"] is heads
    o = _Ops()
    m._attend(o, q, k, v, 2, fp8=False, tiles=m._sparse_tiles(sp_(cdf_heads=lambda li: None), 0, (0, 600)))
    assert set(o.calls[0][2]) == old_kw                                                # a layer that is not named: the scalar
    o = _Ops()
    sp = sp_(similarity=0.25, cdf_heads=lambda li: heads)
    assert m._attend(o, q, k, v, 2, fp8=False, tiles=m._sparse_tiles(sp, 1, (0, 600))) == "attention_tiles"
    assert set(o.calls[0][2]) == old_kw | {"cdf_heads", "similarity_threshold"} and o.calls[0][2]["similarity_threshold"] == 0.25
    # with keep_masks the similarities are copied from the workspace's tail, behind the pooled means
    sims, shape = m._sparse_sims[1]
    at = 2 * 2 * (3 + 18) * 64
    assert shape == (2, 2, 3, 18) and sims.tolist() == sp.workspace[at:at + 2 * 2 * 21].tolist()
    got = m.sparse_attention_similarity()[1]
    assert got[0] == pytest.approx(float(sims[:12].mean())) and got[2:] == (0.0, 0.0)


def test_calibration_runs_eagerly_and_refuses_a_forced_graph():
    m = _tiny_model()
    assert window_attention_runs_eagerly(m, True) is False
    m._sparse_calib = object()
    assert m.is_sparse_calibrating and window_attention_runs_eagerly(m, None) is True and window_attention_runs_eagerly(m, False) is True
    with pytest.raises(RuntimeError, match="calibrated"):
        window_attention_runs_eagerly(m, True)
    m._sparse_calib = None
    from frameino_amd.sparse_calibration import calibrate_sparse_attention, choose_thresholds
    for bad in (dict(l1_bound=0), dict(l1_bound=0.1, grid=()), dict(l1_bound=0.1, grid=(0.9, 0.5)), dict(l1_bound=0.1, grid=(0.5, 1.0))):
        with pytest.raises(ValueError):
            calibrate_sparse_attention(m, lambda: None, **bad)
    with pytest.raises(TypeError):
        calibrate_sparse_attention(m, lambda: None, l1_bound=0.1, base={"cdf_threshold": 0.5})
    # a run that makes no eligible call: no thresholds, the model's setting is put back
    before = SparseAttentionConfig(0.7)
    m.enable_sparse_attention(before)
    seen = []
    cfg, report = calibrate_sparse_attention(m, lambda: seen.append((m.is_sparse_calibrating, m._sparse.cdf_threshold)), l1_bound=0.1)
    assert seen == [(True, 0.5)] and cfg.head_thresholds == {} and report["error"] == {} and m._sparse is before
    assert not m.is_sparse_calibrating
    # the choice: the smallest g such that g and every larger grid value pass; the package's and the restatement's agree
    grid = (0.5, 0.7, 0.9, 0.97)
    err = torch.tensor([[0.3, 0.1, 0.2, 0.05], [0.01, 0.02, 0.01, 0.0], [1.0, 1.0, 1.0, 1.0], [0.5, 0.12, 0.12, 0.12],
                        [0.1, 0.1, 0.1, float("nan")]], dtype=torch.float64)
    assert G.choose(err, grid, 0.12).tolist() == [0.97, 0.5, 1.0, 0.7, 1.0]
    assert choose_thresholds(err, grid, 0.12).tolist() == [0.97, 0.5, 1.0, 0.7, 1.0]


def test_the_header_the_signatures_and_the_library_carry_the_gated_entry_points():
    from frameino_amd import _lib
    names = ("fino_attn_tile_plan_gated_bytes", "fino_attn_tile_plan_gated")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "frameino_hip.h")).read()
    lib = _lib.load()
    for n in names:
        assert n + "(" in header and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert "#define FINO_VERSION 103" in header and lib.fino_version() == 103
    assert len(_lib.SIGNATURES["fino_attn_tile_plan_gated"]) == 24
    plain = lib.fino_attn_tile_plan_bytes(2, 24, 12320, 12320, 128)
    assert lib.fino_attn_tile_plan_gated_bytes(2, 24, 12320, 12320, 128) == plain + 2 * 24 * (49 + 193) * 4
    assert lib.fino_attn_tile_plan_gated_bytes(2, 24, 12320, 12320, 96) == 0
    # argument checks come before any launch
    f1, h, z = ctypes.c_float(1.0), ctypes.c_float(0.5), ctypes.c_float(0.0)

    def call(cdf=h, cdf_heads=0, sim=z, mask=16, ws_bytes=1 << 20, dh=128):
        return lib.fino_attn_tile_plan_gated(16, 16, 1, 1, 8, 8, dh, *([8] * 6), f1, 0, cdf, cdf_heads, sim, 0, mask, 1, 16, ws_bytes, 0)

    assert call(mask=0) == -1 and b"fino_attn_tile_plan_gated: null pointer" in lib.fino_last_error()
    assert call(cdf=z) == -1 and b"cdf" in lib.fino_last_error()
    assert call(cdf_heads=18) == -1 and b"cdf_heads" in lib.fino_last_error()
    assert call(sim=ctypes.c_float(1.5)) == -1 and b"sim_threshold" in lib.fino_last_error()
    assert call(sim=ctypes.c_float(float("nan"))) == -1 and b"sim_threshold" in lib.fino_last_error()
    assert call(dh=96) == -3 and b"head_dim" in lib.fino_last_error()
    # the gate needs the tail behind the pooled means: 1 x 1 x (1 + 1) x 128 x 4 = 1024 bytes do without it only
    assert call(sim=h, ws_bytes=1024) == -1 and b"workspace of 1032" in lib.fino_last_error()
    assert call(ws_bytes=1023) == -1 and b"workspace of 1024" in lib.fino_last_error()


# ---------------------------------------------------------------------------------------------- the restatement's own cases
def test_the_restatement_with_the_gate_off_is_the_ungated_one():
    from tests.test_attention_tile_plan_gpu import HEADS, KEEP, _inputs
    q, k = _inputs(torch.bfloat16, 64)
    for cdf in (0.5, 0.9):
        want, p = R.plan(q, k, HEADS, cdf, KEEP)
        for theta in (None, 0.0):
            keep, pg, dense, unpred = G.plan_gated(q, k, HEADS, cdf, KEEP, theta)
            assert torch.equal(keep, want) and torch.equal(pg, p) and not dense.any() and not unpred.any()
        same = G.plan_gated(q, k, HEADS, 0.123, KEEP, None, cdf_heads=[cdf] * HEADS)[0]
        assert torch.equal(same, want)


def _blocks(q_dirs, k_dirs, dh=64):
    """q-blocks / key tiles whose rows all equal their given row (similarity 1), or, for None, alternate +-e0 (similarity 0)"""
    def rows(dirs, n):
        out = []
        for d in dirs:
            if d is None:
                blk = torch.zeros(n, dh)
                blk[::2, 0], blk[1::2, 0] = 1.0, -1.0
            else:
                blk = torch.as_tensor(d, dtype=torch.float32).expand(n, dh).clone()
            out.append(blk)
        return torch.cat(out)[None]
    return rows(q_dirs, 256), rows(k_dirs, 64)


def test_hand_cases():
    dh = 64
    e = torch.eye(dh)
    # a zero row adds 0 to the normalised sum but counts in n: 63 equal rows and one zero row -> (63 / 64)^2
    q, k = _blocks([e[0]], [e[0], e[1]])
    k[0, 5] = 0
    sq, sk = G.similarity(q, k, 1)
    assert sq.tolist() == [[[1.0]]] and sk[0, 0].tolist() == pytest.approx([(63 / 64) ** 2, 1.0], abs=1e-15)
    assert float(G.similarity(torch.zeros(1, 256, dh), k, 1)[0]) == 0.0                 # all rows zero: 0, not NaN
    # +-e0 alternating: similarity 0; the ragged block uses its real rows only
    q, k = _blocks([e[0], None], [e[0], None, 8 * e[0]])
    sq, sk = G.similarity(q[:, :256 + 7], k[:, :128 + 3], 1)
    assert sq[0, 0].tolist() == pytest.approx([1.0, (1 / 7) ** 2]) and sk[0, 0].tolist() == pytest.approx([1.0, 0.0, 1.0])
    # the gate: tile 1 is unpredictable -> kept in every row and outside the softmax; q-block 1 is dense
    keep, p, dense, unpred = G.plan_gated(q, k, 1, 0.5, None, 0.5)
    assert dense[0, 0].tolist() == [False, True] and unpred[0, 0].tolist() == [False, True, False]
    assert p[0, 0, 0, 1] == 0 and float(p[0, 0, 0].sum()) == pytest.approx(1.0) and float(p[0, 0, 0, 2]) == pytest.approx(1 / (1 + 2.718281828459045 ** -0.875))
    assert keep[0, 0].tolist() == [[False, True, True], [True, True, True]]
    # ... against the ungated plan, which predicts from the meaningless mean of tile 1 and thins q-block 1
    assert R.plan(q, k, 1, 0.5)[0][0, 0, 0].tolist() == [False, False, True]
    # m_F counts F \\ U only: forcing the unpredictable tile adds no mass
    keep = G.plan_gated(q, k, 1, 0.5, torch.tensor([[[1, 2], [0, 0], [0, 0]]] * 2), 0.5)[0]
    assert keep[0, 0, 0].tolist() == [False, True, True]
    # all tiles unpredictable: sum w = 0, U (and F) alone -- which is everything
    q, k = _blocks([e[0]], [None, None, None])
    keep, p, dense, unpred = G.plan_gated(q, k, 1, 0.5, None, 0.5)
    assert unpred.all() and not dense.any() and float(p.abs().sum()) == 0.0 and keep.all()
    # a head at threshold 1.0 is full, whatever its p; the other head keeps its scalar mask
    q2, k2 = _blocks([e[0]], [e[0], 2 * e[0], 8 * e[0]])
    q2, k2 = torch.cat([q2, q2], dim=2), torch.cat([k2, k2], dim=2)
    keep = G.plan_gated(q2, k2, 2, 0.9, None, None, cdf_heads=[0.5, 1.0])[0]
    assert keep[0, 1].all() and torch.equal(keep[0, 0], R.plan(q2, k2, 2, 0.5)[0][0, 0]) and not keep[0, 0].all()


# ---------------------------------------------------------------------------------------------- conditions on the GPU tests' inputs
def test_the_gated_plan_inputs_separate_the_blocks():
    from tests.test_attention_tile_plan_gated_gpu import B, CDFS, HEADS, KEEP, NQB, NT, THETA, _gated_properties, _inputs
    for dh in (128, 64):
        for dtype in (torch.bfloat16, torch.float16):
            q, k, _ = _inputs(dtype, dh)
            sq, sk = G.similarity(q, k, HEADS)
            every = torch.cat([sq.flatten(), sk.flatten()])
            gap, lo, hi = float((every - THETA).abs().min()), float(every[every < THETA].max()), float(every[every > THETA].min())
            n_unpred = (sk < THETA).sum(-1)
            print(f"dh {dh} {dtype}: similarities <= {lo:.3f} or >= {hi:.3f} (gap to theta {gap:.3f}); unpredictable tiles per "
                  f"(b, h) {int(n_unpred.min())} .. {int(n_unpred.max())} of {NT}")
            assert gap >= 0.13                                            # (measured: 0.146 at head_dim 128, 0.204 at 64)
            assert hi >= 0.45 and lo <= 0.12
            assert 1 <= int(n_unpred.min()) and int(n_unpred.max()) <= 10
            assert (sq < THETA).tolist() == [[[False, True, False]] * HEADS] * B  # exactly the middle q-block is dense
            # the reference itself has the properties, and they bite
            forced = R.forced_tiles(KEEP, NQB, NT)
            for cdf in CDFS:
                keep, p, dense, unpred = G.plan_gated(q, k, HEADS, cdf, KEEP, THETA)
                bit = _gated_properties(keep, p, dense, unpred, forced, cdf, "reference")
                assert bit["order"] > 0 and bit["minimal"] > 0
                n = keep[:, :, [0, 2]].sum(-1)
                assert int(n.max()) < NT and not torch.equal(keep, R.plan(q, k, HEADS, cdf, KEEP)[0])


def test_the_calibration_inputs_have_a_clear_choice():
    from tests.test_sparse_calibration_gpu import BOUND, CHOICE, GRID, HEADS, MARGIN, STRENGTH, _inputs
    for dh in (128, 64):
        q, k, v = _inputs(torch.bfloat16, dh)
        err = G.l1_errors(q, k, v, HEADS, GRID)
        margin = float(((err - BOUND).abs() / BOUND).min())
        print(f"dh {dh}: reference errors per head {STRENGTH} over the grid {GRID}:\n{err}\nsmallest relative distance to the "
              f"bound {margin:.3f}")
        assert G.choose(err, GRID, BOUND).tolist() == list(CHOICE)
        assert margin >= 0.10 and margin >= MARGIN


def test_the_examples_flags_parse():
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "run_wan_frameino.py"), "--help"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0
    for flag in ("--sparse-similarity THETA", "--sparse-calibrate OUT.json", "--sparse-l1 X", "--sparse-thresholds FILE"):
        assert flag in r.stdout, flag
