"""Block-Hadamard rotation of the MXFP6 linears, the part that needs no GPU: the algebra, what the restatement
(tests/mxfp6_rot_ref.py) gains on the very tensors the GPU GEMM test uses, the new entry in header, ctypes table and library
with its error paths, and the routing of `enable_mxfp6_linears(rotate=...)` seen by a recording `ops`."""
import os

import pytest
import torch

from frameino_amd import _lib
from tests import mxfp6_ref as R
from tests import mxfp6_rot_ref as RR
from tests.test_host_cpu import _tiny
from tests.test_mx_linears_cpu import MODELS, _Recorder


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------- algebra
def test_rotation_is_the_hadamard_matrix_and_keeps_the_dot_product():
    h = RR.rotate(torch.eye(32))                                      # row i = H e_i
    assert torch.equal(h, h.T) and torch.equal(h.abs(), torch.ones(32, 32))
    assert torch.equal(h @ h, 32 * torch.eye(32))
    assert torch.equal(h[:, 0], torch.ones(32)) and h[1].tolist() == [1.0, -1.0] * 16
    g = torch.Generator().manual_seed(3)
    a = torch.randn(7, 96, generator=g, dtype=torch.float64)
    w = torch.randn(5, 96, generator=g, dtype=torch.float64)
    hd = h.double()
    ra = (a.view(7, 3, 32) @ hd).reshape(7, 96)
    rw = (w.view(5, 3, 32) @ hd).reshape(5, 96)
    ref = a @ w.T
    assert float(((ra @ rw.T / 32 - ref).abs().max() / ref.abs().max())) <= 1e-9
    # the fp32 butterflies on bf16 inputs are H v exactly at these magnitudes (sums of 32 bf16 values fit 24 bits here)
    x = torch.randint(-64, 64, (4, 64), generator=g).float().bfloat16()
    assert torch.equal(RR.rotate(x).double(), (x.double().view(4, 2, 32) @ hd).reshape(4, 64))


def test_weight_mode_shifts_the_exponent_by_five_and_clamps():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(9, 128, generator=g).bfloat16()
    x[0, :32] = 0
    x[1, 32:64] = 0
    x[1, 40] = 2.0 ** -125                                            # e = -127 after the clamp of the rule; stays -127
    ca, ea = RR.quantize_ref(x, "act")
    cw, ew = RR.quantize_ref(x, "weight")
    assert torch.equal(ca, cw)
    assert int(ea[0, 0]) == -127 and int(ew[0, 0]) == -127 and int(ew[1, 1]) == -127
    live = ea > -122
    assert torch.equal(ew[live], ea[live] - 5) and bool(live.sum() >= 9 * 4 - 2)
    # one non-zero element c rotates to +-c in all 32 places: codes all the same magnitude
    x = torch.zeros(1, 32)
    x[0, 5] = -3.0
    codes, e = RR.quantize_ref(x.bfloat16(), "act")
    assert int(e[0, 0]) == -1 and set((codes & 31).flatten().tolist()) == {int(R.quantize_ref(torch.tensor([[6.0] + [0.0] * 31]))[0][0, 0])}
    assert torch.equal(RR.decode(codes, e).abs(), torch.full((1, 32), 3.0))


# ------------------------------------------------------------------------------------------- what the rotation gains, restated
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_restated_rotation_gains_on_the_gemm_tests_outlier_tensors_and_costs_nothing_on_gaussian_ones(dtype):
    a, w = RR.gemm_operands(dtype)
    plain, rot = RR.restated_errors(a, w)
    print(f"[{dtype}] outlier columns: e2m3 {plain:.4f}  rotated {rot:.4f}  ratio {rot / plain:.3f}")
    assert rot <= 0.85 * plain
    a, w = RR.gemm_operands(dtype, outliers=False)
    plain, rot = RR.restated_errors(a, w)
    print(f"[{dtype}] N(0,1): e2m3 {plain:.4f}  rotated {rot:.4f}  ratio {rot / plain:.3f}")
    assert rot <= 1.05 * plain


# -------------------------------------------------------------------------------------------------------------------- ABI
def test_entry_in_header_table_and_library_and_its_error_paths(lib):
    name = "fino_quantize_mxfp6_rot"
    assert name in _lib.declared_symbols() and name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES[name]) == len(_lib.SIGNATURES["fino_quantize_mxfp6"]) + 1
    header = open(_lib.HEADER_PATH).read()
    assert "#define FINO_MX_ROT_ACT 1" in header and "#define FINO_MX_ROT_WEIGHT 2" in header
    assert lib.fino_version() == 103 and _lib.ABI_VERSION == 103      # additive
    from frameino_amd import ops
    assert ops.MX_ROTATE == {"act": 1, "weight": 2}
    # every failure returns before a launch (no GPU here; pointers are never dereferenced on the host)
    for mode in (0, 3, -1):
        rc = lib.fino_quantize_mxfp6_rot(16, 16, 16, 4, 128, 128, 0, mode, 0)
        err = lib.fino_last_error()
        assert rc == -1 and b"fino_quantize_mxfp6_rot" in err and f"mode {mode}".encode() in err
    for mode in (1, 2):
        rc = lib.fino_quantize_mxfp6_rot(16, 16, 16, 4, 100, 104, 0, mode, 0)
        assert rc == -1 and b"fino_quantize_mxfp6_rot" in lib.fino_last_error() and b"multiple of 128" in lib.fino_last_error()
        rc = lib.fino_quantize_mxfp6_rot(16, 16, 16, 4, 128, 128, 7, mode, 0)
        assert rc == -1 and b"dtype" in lib.fino_last_error()
        rc = lib.fino_quantize_mxfp6_rot(16, 0, 16, 4, 128, 128, 0, mode, 0)
        assert rc == -1 and b"null" in lib.fino_last_error()
        rc = lib.fino_quantize_mxfp6_rot(16, 24, 16, 4, 128, 128, 0, mode, 0)
        assert rc == -1 and b"alignment" in lib.fino_last_error()
    rc = lib.fino_quantize_mxfp6(16, 16, 16, 4, 100, 104, 0, 0)      # the old entry names itself, as before
    assert rc == -1 and lib.fino_last_error().startswith(b"fino_quantize_mxfp6: cols must be a multiple of 128")


def test_front_end_refuses_an_unknown_rotation_before_the_library(lib):
    from frameino_amd import ops
    with pytest.raises(ValueError, match="rotate"):
        ops.quantize_mxfp6(torch.zeros(4, 128, dtype=torch.bfloat16), rotate="both")


# ---------------------------------------------------------------------------------------------------------------- routing
class _RotRecorder(_Recorder):
    """the recorder whose MXFP6 quantiser also takes `rotate=` (the base class's takes `x` alone: a stray keyword on the
    unrotated path is a TypeError there)"""

    def quantize_mxfp6(self, x, **kw):
        i = self._note("quantize_mxfp6", x, **kw)
        return ("q6", i), ("s6", i)


@pytest.fixture(params=sorted(MODELS))
def model(request):
    return MODELS[request.param][0], MODELS[request.param][1]


def _drive(m, rec, **enable_kw):
    """switch on, run `_lin` plain, with keep and with a residual epilogue; -> the recorded (name, kwargs) sequence"""
    x, w, b = torch.zeros(3, 8), torch.zeros(5, 8), torch.zeros(5)
    m.enable_mxfp6_linears(**enable_kw)
    m._lin(0, "qkv", x, w, b)
    m._lin(0, "qkv", x, w, b, 2, residual=x, keep=x, tile_m=4)
    return [(c[0], len(c[1]), tuple(sorted(c[2])), c[2].get("rotate")) for c in rec.calls]


def test_rotate_false_makes_exactly_the_calls_of_today(model):
    make, n_weights = model
    seqs = []
    for kw in ({}, {"rotate": False}, {"enabled": True, "rotate": False}):
        m = make()
        m.ops = rec = _Recorder()                                     # strict: quantize_mxfp6(x) takes no keyword
        seqs.append(_drive(m, rec, **kw))
        assert m.mxfp6_rotate is False
        assert all("rotate" not in keys for _, _, keys, _ in seqs[-1])
    assert seqs[0] == seqs[1] == seqs[2]
    assert [s[0] for s in seqs[0]] == ["quantize_mxfp6"] * n_weights + ["quantize_mxfp6", "gemm_mxfp6"] * 2
    assert seqs[0][-1][2] == ("keep", "residual")


def test_rotate_true_sends_weight_for_weights_and_act_for_activations(model):
    make, n_weights = model
    m = make()
    m.ops = rec = _RotRecorder()
    assert m.mxfp6_rotate is False
    seq = _drive(m, rec, rotate=True)
    assert m.mxfp6_rotate is True and m._mx_fmt == 6 and len(m._fp8) == n_weights
    assert seq[:n_weights] == [("quantize_mxfp6", 1, ("rotate",), "weight")] * n_weights
    assert seq[n_weights:] == [("quantize_mxfp6", 1, ("rotate",), "act"), ("gemm_mxfp6", 6, (), None),
                               ("quantize_mxfp6", 1, ("rotate",), "act"), ("gemm_mxfp6", 6, ("keep", "residual"), None)]
    with pytest.raises(AttributeError):
        m.mxfp6_rotate = False                                        # read-only


def test_flag_survives_invalidation_and_changing_it_requantises(model):
    make, n_weights = model
    m = make()
    m.ops = rec = _RotRecorder()
    m.enable_mxfp6_linears(rotate=True)
    rec.calls.clear()
    assert m._mx_invalidate() is True
    assert not m._fp8 and m._fp8_pending and m.mxfp6_rotate is True and rec.calls == []
    m._mx_requantise_if_pending()
    assert [(c[0], c[2]) for c in rec.calls] == [("quantize_mxfp6", {"rotate": "weight"})] * n_weights
    assert m.mxfp6_rotate is True and not m._fp8_pending and len(m._fp8) == n_weights
    rec.calls.clear()
    m.to(torch.float64)                                               # the public route to the same invalidation
    assert m._fp8_pending and m.mxfp6_rotate is True and rec.calls == []
    m._mx_requantise_if_pending()
    assert [c[2] for c in rec.calls] == [{"rotate": "weight"}] * n_weights
    rec.calls.clear()
    m.enable_mxfp6_linears(True, rotate=False)                        # another value while on: the weights are quantised anew
    assert [(c[0], c[2]) for c in rec.calls] == [("quantize_mxfp6", {})] * n_weights and m.mxfp6_rotate is False
    rec.calls.clear()
    m.enable_mxfp6_linears(True, rotate=True)
    assert [c[2] for c in rec.calls] == [{"rotate": "weight"}] * n_weights and m.mxfp6_rotate is True
    m._mx_invalidate()
    m.enable_mxfp6_linears(False)                                     # off while pending: nothing left
    assert not m._fp8 and not m._fp8_pending and m.mxfp6_rotate is False and m._mx_rotate is False
    rec.calls.clear()
    x, w, b = torch.zeros(3, 8), torch.zeros(5, 8), torch.zeros(5)
    m._lin(0, "qkv", x, w, b)
    assert rec.names() == ["gemm"]
    m.enable_mxfp6_linears()                                          # and the next plain switch-on is unrotated
    assert m.mxfp6_rotate is False and all(c[2] == {} for c in rec.calls[1:])


def test_mxfp8_takes_no_rotation_and_is_not_disturbed_by_the_flag(model):
    make, n_weights = model
    m = make()
    m.ops = rec = _RotRecorder()
    with pytest.raises(TypeError):
        m.enable_mxfp8_linears(rotate=True)
    with pytest.raises(TypeError):
        m.enable_mxfp8_linears(True, True)
    assert "e4m3" in type(m).enable_mxfp8_linears.__doc__ and "rotat" in type(m).enable_mxfp8_linears.__doc__
    m.enable_mxfp6_linears(rotate=True)
    with pytest.raises(ValueError, match="enable_mxfp8_linears"):
        m.enable_mxfp8_linears()
    m.enable_mxfp6_linears(False)
    rec.calls.clear()
    m.enable_mxfp8_linears()
    assert rec.names() == ["quantize_mxfp8"] * n_weights and m.mxfp6_rotate is False
    m.enable_mxfp6_linears(False, rotate=True)                        # the other precision's off-switch: MXFP8 stays
    assert m._mx_fmt == 8 and len(m._fp8) == n_weights and m.mxfp6_rotate is False


def test_wan_token_shard_blocks_are_quantised_as_rotated_weights_on_first_use():
    m = _tiny()
    m.ops = rec = _RotRecorder()
    x, w, b = torch.zeros(3, 8), torch.zeros(5, 8), torch.zeros(5)
    m.enable_mxfp6_linears(rotate=True)
    rec.calls.clear()
    for key in ("kv", "q"):
        m._lin(0, key, x, w, b)
    assert [(c[0], c[2]) for c in rec.calls] == [("quantize_mxfp6", {"rotate": "weight"}), ("quantize_mxfp6", {"rotate": "act"}),
                                                 ("gemm_mxfp6", {})] * 2
    assert rec.calls[0][1][0].shape == w.shape and (0, "kv") in m._fp8 and (0, "q") in m._fp8


@pytest.mark.parametrize("script", ["run_wan_frameino.py", "run_cogvideox_frameino.py"])
def test_examples_take_the_rotation_only_with_the_mxfp6_switch(script):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "examples", script), "--mxfp6-rotate"], capture_output=True, text=True)
    assert r.returncode == 2 and "--mxfp6-rotate needs --mxfp6" in r.stderr
