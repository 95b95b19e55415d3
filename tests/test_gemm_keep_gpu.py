"""fino_gemm_keep (`ops.gemm(..., keep=)`): a residual epilogue that also stores y = T(acc + bias), the value the epilogue stages
before its gate multiply and residual add (csrc/fino_gemm_common.h: the KEEP flag of gemm_epilogue_t).  Pyramid Attention
Broadcast caches an attention branch's output with it.

Nothing here has a tolerance: `keep` must be the bits FINO_EPI_NONE writes, `out` the bits of the same call without `keep`, and
`ops.pab_broadcast` on the kept y the bits of the epilogue itself.  Shapes: the ragged last tile row and column (M = 33, 300;
N = 8, 264), one row, exact tiles, K on the DMA path (64) and on the generic one (200); the smallest and the tallest tile and the
planner's; a two-launch plan (leading 256-row tiles + lower ones: the keep buffer's row offset)."""
import pytest
import torch

from frameino_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 1234.0          # exactly representable in bf16 and fp16
EPILOGUES = {"residual": ops.EPI_RESIDUAL, "gated": ops.EPI_GATED_RESIDUAL, "gated_staged": ops.EPI_GATED_RESIDUAL_STAGED}
SHAPES = [(m, n, k) for m in (1, 33, 256, 300) for n in (8, 256, 264) for k in (64, 200)]


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


def _check(m, n, k, epi, dtype, tile_m, seed=0):
    a, w, bias, res, gate, sel = _operands(m, n, k, epi, dtype, seed)
    y = ops.gemm(a, w, bias, ops.EPI_NONE, tile_m=tile_m)
    want = ops.gemm(a, w, bias, epi, residual=res, gate=gate, sel=sel, tile_m=tile_m)
    # ldk > N, and sentinel rows below M: whatever the kernel writes outside [M, N] shows
    keep_buf = torch.full((m + 3, n + 24), SENTINEL, device=DEV, dtype=dtype)
    keep = keep_buf[:m, :n]
    x = res.clone()
    out = ops.gemm(a, w, bias, epi, residual=x, gate=gate, sel=sel, out=x, tile_m=tile_m, keep=keep)      # out aliases residual
    what = f"M={m} N={n} K={k} epilogue={epi} {dtype} tile_m={tile_m}"
    assert out is x and torch.equal(x, want), f"{what}: out differs from the call without keep"
    assert torch.equal(keep, y), f"{what}: keep differs from EPI_NONE"
    assert bool((keep_buf[m:] == SENTINEL).all()) and bool((keep_buf[:, n:] == SENTINEL).all()), f"{what}: wrote outside [M, N]"
    if epi != ops.EPI_GATED_RESIDUAL_STAGED:
        # the re-use step of Pyramid Attention Broadcast: the epilogue's arithmetic on the kept y, bit for bit
        assert torch.equal(ops.pab_broadcast(res, keep, gate, sel), want), f"{what}: pab_broadcast differs from the epilogue"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("epi", list(EPILOGUES.values()), ids=list(EPILOGUES))
@pytest.mark.parametrize("tile_m", [0, 2, 5, 8])
def test_keep_is_epi_none_and_out_is_unchanged(dtype, epi, tile_m):
    for i, (m, n, k) in enumerate(SHAPES):
        _check(m, n, k, epi, dtype, tile_m, seed=i)


@pytest.mark.parametrize("epi", [ops.EPI_RESIDUAL, ops.EPI_GATED_RESIDUAL], ids=["residual", "gated"])
def test_a_two_launch_plan_offsets_the_keep_buffer(epi):
    m, n = 24640 // 4 + 70, 512
    r256, rest = ops.gemm_plan(m, n)
    print(f"plan for {m} x {n}: {r256} rows of 256-row tiles + {rest}-row tiles")
    _check(m, n, 64, epi, torch.bfloat16, 0, seed=7)


def test_bad_epilogue_or_dtype_is_an_argument_error():
    from frameino_amd import _lib
    lib = _lib.lib()
    t = torch.zeros(8, 64, device=DEV, dtype=torch.bfloat16)
    p = t.data_ptr()

    def call(epi, dtype, keep=p, ldk=64):
        return lib.fino_gemm_keep(p, p, 0, p, 8, 8, 64, 64, 64, 64, epi, p, 64, p, 0, 0, dtype, keep, ldk, 0, 0)

    for epi in (ops.EPI_NONE, ops.EPI_GELU_TANH, ops.EPI_F32, ops.EPI_F32_RESIDUAL, 9):
        assert call(epi, ops.BF16) == -1 and b"epilogue" in lib.fino_last_error()
    assert call(ops.EPI_RESIDUAL, 2) == -1 and b"dtype" in lib.fino_last_error()          # fp32 storage: not a GEMM dtype
    assert call(ops.EPI_RESIDUAL, ops.BF16, keep=0) == -1 and b"keep" in lib.fino_last_error()
    assert call(ops.EPI_RESIDUAL, ops.BF16, ldk=4) == -1 and b"keep" in lib.fino_last_error()
    with pytest.raises(RuntimeError, match="fino_gemm_keep"):
        ops.gemm(t, t[:8], None, ops.EPI_NONE, keep=torch.zeros(8, 8, device=DEV, dtype=torch.bfloat16))
