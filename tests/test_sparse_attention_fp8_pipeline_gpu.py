"""Sparse attention with fp8 attention through the FrameINO Wan denoise loop, at the shape of
tests/test_sparse_attention_pipeline_gpu.py: the tiny DiT of the golden wan_pipe_tiny (head_dim 128), 693 rows (three q-blocks,
eleven key tiles), 4 Euler steps, CFG 5.  The predictor, the one mask buffer and the fp8 workspace are static on the device, so the
default hipGraph loop stays and must equal the eager loop bit for bit -- the property section 6j has."""
import pytest
import torch

from tests.test_sparse_attention_pipeline_gpu import _sparse
from tests.test_window_attention_pipeline_gpu import _pipe

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fp8", [{}, dict(smooth_k=True, smooth_v=True)], ids=["plain", "smooth-k-v"])
def test_graph_replay_equals_eager_with_fp8_and_sparse_attention(golden, fp8):
    pipe, args = _pipe(golden)
    tr = pipe.transformer
    assert tr.config.attention_head_dim == 128
    tr.enable_fp8_attention(**fp8)
    pipe.use_hip_graph = False
    dense = pipe.denoise(*args)                                        # fp8 attention alone
    _sparse(pipe)
    assert tr.fp8_attention and tr.is_sparse_attention_enabled
    eager = pipe.denoise(*args)
    dens = tr.sparse_attention_density()
    print(f"densities after the eager loop: {dens}")
    assert sorted(dens) == list(range(len(tr.blocks))) and all(0.0 < d < 1.0 for d in dens.values())
    pipe.use_hip_graph = True                                          # a failed capture is an error
    graphed = pipe.denoise(*args)
    assert torch.equal(eager, graphed)
    assert torch.isfinite(eager).all() and not torch.equal(eager, dense)
    rel = ((eager - dense).pow(2).mean().sqrt() / dense.pow(2).mean().sqrt()).item()
    print(f"fp8 {fp8} + sparse vs fp8 dense latents after 4 steps: rel-RMS {rel:.3e}")
    pipe.use_hip_graph = None                                          # the default: still the graph loop
    assert torch.equal(pipe.denoise(*args), eager)
    _sparse(pipe, cdf_threshold=1.0)                                   # a threshold of 1: the dense fp8 loop, bit for bit
    assert torch.equal(pipe.denoise(*args), dense)
