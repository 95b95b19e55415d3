"""fino_gemm_mxfp8_keep / fino_gemm_mxfp6_keep (`ops.gemm_mxfp8(..., keep=)`, `ops.gemm_mxfp6(..., keep=)`): an MX GEMM with a
residual epilogue that also stores y = T(acc + bias), the value the shared epilogue stages before its gate multiply and residual
add (csrc/fino_gemm_common.h: the KEEP flag of gemm_epilogue_t, instantiated for the MX kernels).  Pyramid Attention Broadcast
caches the out-projection of an MX model with it in one launch.

Nothing here has a tolerance: `keep` must be the bits FINO_EPI_NONE writes, `out` the bits of the same call without `keep`, and
the re-use arithmetic on the kept y -- `ops.pab_broadcast` for the two unstaged epilogues, `ops.gated_residual(staged=True)` for
the staged one -- the bits of the epilogue itself.  Shapes at the edges of the one MX tile (256 x 256, K-tiles of 128): one row, a
ragged last tile row (33), an exact tile (256), a tile plus a ragged one (300); a ragged last tile column (264) and an exact one;
one K-tile and three."""
import pytest
import torch

from frameino_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 1234.0          # exactly representable in bf16 and fp16
EPILOGUES = {"residual": ops.EPI_RESIDUAL, "gated": ops.EPI_GATED_RESIDUAL, "gated_staged": ops.EPI_GATED_RESIDUAL_STAGED}
SHAPES = [(m, n, k) for m in (1, 33, 256, 300) for n in (264, 256) for k in (128, 384)]
FORMATS = {"mxfp8": (ops.quantize_mxfp8, ops.gemm_mxfp8), "mxfp6": (ops.quantize_mxfp6, ops.gemm_mxfp6)}


def _operands(m, n, k, epi, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    a = torch.randn(m, k, device=DEV, generator=g).to(dtype)
    w = (torch.randn(n, k, device=DEV, generator=g) * k ** -0.5).to(dtype)
    bias = torch.randn(n, device=DEV, generator=g).to(dtype)
    res = torch.randn(m, n, device=DEV, generator=g).to(dtype)
    gated = epi != ops.EPI_RESIDUAL
    gate = torch.randn(2, n, device=DEV, generator=g) if gated else None               # two gate rows ...
    sel = (torch.arange(m, device=DEV) % 3 == 1).to(torch.int32) if gated else None    # ... picked per row
    return a, w, bias, res, gate, sel


def _reuse(epi, res, y, gate, sel):
    """what a re-using step of Pyramid Attention Broadcast launches on the kept y"""
    if epi == ops.EPI_GATED_RESIDUAL_STAGED:
        return ops.gated_residual(res, y, gate, sel, staged=True)
    return ops.pab_broadcast(res, y, gate, sel)


def _check(fmt, m, n, k, epi, dtype, seed=0):
    quantize, gemm = FORMATS[fmt]
    a, w, bias, res, gate, sel = _operands(m, n, k, epi, dtype, seed)
    (aq, sa), (wq, sw) = quantize(a), quantize(w)
    y = gemm(aq, sa, wq, sw, bias, ops.EPI_NONE, out_dtype=dtype)
    want = gemm(aq, sa, wq, sw, bias, epi, residual=res, gate=gate, sel=sel, out_dtype=dtype)
    # ldk > N, and sentinel rows below M: whatever the kernel writes outside [M, N] shows
    keep_buf = torch.full((m + 3, n + 24), SENTINEL, device=DEV, dtype=dtype)
    keep = keep_buf[:m, :n]
    x = res.clone()
    out = gemm(aq, sa, wq, sw, bias, epi, residual=x, gate=gate, sel=sel, out=x, out_dtype=dtype, keep=keep)   # out aliases residual
    what = f"{fmt} M={m} N={n} K={k} epilogue={epi} {dtype}"
    assert out is x and torch.equal(x, want), f"{what}: out differs from the call without keep"
    assert torch.equal(keep, y), f"{what}: keep differs from EPI_NONE"
    assert bool((keep_buf[m:] == SENTINEL).all()) and bool((keep_buf[:, n:] == SENTINEL).all()), f"{what}: wrote outside [M, N]"
    assert torch.equal(_reuse(epi, res, keep, gate, sel), want), f"{what}: the re-use arithmetic differs from the epilogue"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("epi", list(EPILOGUES.values()), ids=list(EPILOGUES))
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_keep_is_epi_none_and_out_is_unchanged(fmt, epi, dtype):
    for i, (m, n, k) in enumerate(SHAPES):
        _check(fmt, m, n, k, epi, dtype, seed=i)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_the_staged_reuse_reproduces_the_model_dtype_gemm_too(dtype):
    """the same re-use launch serves the model-dtype out-projection (`ops.gemm(..., keep=)`, staged epilogue)"""
    epi = ops.EPI_GATED_RESIDUAL_STAGED
    for i, (m, n, k) in enumerate(SHAPES):
        a, w, bias, res, gate, sel = _operands(m, n, k, epi, dtype, 100 + i)
        keep = torch.empty(m, n, device=DEV, dtype=dtype)
        want = ops.gemm(a, w, bias, epi, residual=res, gate=gate, sel=sel, keep=keep)
        assert torch.equal(ops.gated_residual(res, keep, gate, sel, staged=True), want), (m, n, k)


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_argument_errors(fmt):
    from frameino_amd import _lib
    lib = _lib.lib()
    entry = getattr(lib, f"fino_gemm_{fmt}_keep")
    t = torch.zeros(8, 128, device=DEV, dtype=torch.bfloat16)
    p = t.data_ptr()

    def call(epi, dtype=ops.BF16, keep=p, ldk=8, n=8):
        return entry(p, p, p, p, 0, p, 8, n, 128, 8, epi, p, 8, p, 0, 0, dtype, keep, ldk, 0)

    for epi in (ops.EPI_NONE, ops.EPI_GELU_TANH, 9):
        assert call(epi) == -1 and b"epilogue" in lib.fino_last_error() and fmt.encode() in lib.fino_last_error()
    for epi in EPILOGUES.values():
        assert call(epi, keep=0) == -1 and b"keep" in lib.fino_last_error()                 # null
        assert call(epi, keep=p + 2) == -1 and b"keep" in lib.fino_last_error()             # misaligned
        assert call(epi, ldk=4) == -1 and b"keep" in lib.fino_last_error()                  # ldk < N
        assert call(epi, ldk=12) == -1 and b"keep" in lib.fino_last_error()                 # ldk not a multiple of 8
    assert call(ops.EPI_RESIDUAL, dtype=2) == -1 and b"dtype" in lib.fino_last_error()
    # through ops: a non-residual epilogue with keep=
    quantize, gemm = FORMATS[fmt]
    (aq, sa), (wq, sw) = quantize(t), quantize(t)
    with pytest.raises(RuntimeError, match=f"fino_gemm_{fmt}_keep"):
        gemm(aq, sa, wq, sw, None, ops.EPI_NONE, keep=torch.zeros(8, 8, device=DEV, dtype=torch.bfloat16))
