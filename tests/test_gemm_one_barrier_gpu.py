"""The one-barrier loop of fino_gemm (gemm_kernel with GENERIC = false, CONV = false) against the ping-pong loop, bit for bit.
The library reads FINO_GEMM_PP once per process, so the one-barrier side runs in ONE fresh child process with FINO_GEMM_PP=0
(this file as a script), which saves its outputs; this process runs the same seeded inputs on the default path.

Operands, bias and residual are small integers in [-3, 3]: every product and every partial sum is exact in fp32 whatever the
order, so both loops hand the shared epilogue the same accumulators and the outputs must be EQUAL; for the plain epilogue they
must also equal the fp32 restatement rounded once.  Shapes: one K-tile with ragged M and N; two K-tiles (the prologue stages
both); three (the in-loop LDS-DMA of tile t + 2 runs); a sliver."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(257, 264, 64), (300, 256, 128), (513, 264, 192), (5, 8, 256)]
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
KINDS = ("bias", "gated", "keep")
CASES = [(m, n, k, dt, kind) for (m, n, k) in SHAPES for dt in DTYPES for kind in KINDS]


def _id(case):
    return "%dx%dx%d-%s-%s" % case


def _inputs(case):
    m, n, k, dt, kind = case
    g = torch.Generator().manual_seed(1000 + CASES.index(case))

    def ints(*shape):
        return torch.randint(-3, 4, shape, generator=g).to(DTYPES[dt]).to(DEV)
    t = dict(a=ints(m, k), w=ints(n, k), bias=ints(n), r=ints(m, n))
    # a two-row selector: the gate row changes inside a tile and at odd places
    t["gate"] = (torch.randint(-3, 4, (2, n), generator=g).float() * 0.5).to(DEV)
    t["sel"] = (torch.randint(0, 2, (m,), generator=g)).to(torch.int32).to(DEV)
    return t


def _run(ops, case):
    """the outputs of one case on whatever loop this process runs, on the CPU"""
    t = _inputs(case)
    kind = case[4]
    if kind == "bias":
        out = (ops.gemm(t["a"], t["w"], t["bias"]),)
    elif kind == "gated":
        out = (ops.gemm(t["a"], t["w"], t["bias"], ops.EPI_GATED_RESIDUAL, residual=t["r"], gate=t["gate"], sel=t["sel"]),)
    else:
        keep = torch.empty_like(t["r"])
        out = (ops.gemm(t["a"], t["w"], t["bias"], ops.EPI_RESIDUAL, residual=t["r"], keep=keep), keep)
    torch.cuda.synchronize()
    return tuple(o.cpu() for o in out)


def _run_all():
    from frameino_amd import ops
    return {_id(c): _run(ops, c) for c in CASES}


@pytest.fixture(scope="module")
def one_barrier(tmp_path_factory):
    """every case on the one-barrier loop: one child process; a child that does not exit 0 fails every test of the module here,
    before this process has touched the GPU"""
    path = str(tmp_path_factory.mktemp("one_barrier") / "out.pt")
    env = dict(os.environ, FINO_GEMM_PP="0")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), path]
    try:
        r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        pytest.fail("the FINO_GEMM_PP=0 child did not finish in 300 s")
    if r.returncode != 0:
        pytest.fail("the FINO_GEMM_PP=0 child exited %d:\n%s" % (r.returncode, r.stderr[-2000:]))
    return torch.load(path)


@pytest.fixture(scope="module")
def ping_pong(one_barrier):
    assert os.environ.get("FINO_GEMM_PP", "1") != "0", "this process must run the default (ping-pong) path"
    return _run_all()


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_one_barrier_loop_equals_ping_pong_loop(one_barrier, ping_pong, case):
    got, want = one_barrier[_id(case)], ping_pong[_id(case)]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and torch.equal(g, w)


@pytest.mark.parametrize("case", [c for c in CASES if c[4] != "gated"], ids=[_id(c) for c in CASES if c[4] != "gated"])
def test_one_barrier_loop_equals_fp32_restatement(one_barrier, ping_pong, case):
    """y = T(a w^T + bias): the plain epilogue's output, and what the keep buffer receives beside a residual epilogue"""
    t = _inputs(case)
    y = (t["a"].float() @ t["w"].float().t() + t["bias"].float()).to(DTYPES[case[3]]).cpu()
    for res in (one_barrier, ping_pong):
        assert torch.equal(res[_id(case)][-1], y)
    if case[4] == "keep":       # c = T(r + y), one more rounding (exact here: small integers)
        c = (t["r"].float().cpu() + y.float()).to(DTYPES[case[3]])
        assert torch.equal(one_barrier[_id(case)][0], c)


if __name__ == "__main__":
    assert os.environ.get("FINO_GEMM_PP") == "0"
    sys.path.insert(0, ROOT)
    torch.save(_run_all(), sys.argv[1])
