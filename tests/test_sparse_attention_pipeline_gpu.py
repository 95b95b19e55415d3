"""Sparse attention through the FrameINO Wan denoise loop (pipeline_wan_i2v_motion_frameino.py), at the shape of
tests/test_window_attention_pipeline_gpu.py: the tiny DiT of the golden wan_pipe_tiny, 6 generated latent frames + 1
identity-reference frame of 9 x 11 tokens (693 rows: three q-blocks, eleven key tiles), 4 Euler steps, CFG 5.  The predictor runs
on the device and the mask buffer is allocated once, so the default hipGraph loop stays and must equal the eager loop bit for bit."""
import pytest
import torch

from frameino_amd.window_attention import SparseAttentionConfig
from tests.test_window_attention_pipeline_gpu import FG, NID, _pipe

pytestmark = pytest.mark.gpu


def _sparse(pipe, **kw):
    pipe.transformer.disable_sparse_attention()
    pipe.transformer.enable_sparse_attention(SparseAttentionConfig(**{"cdf_threshold": 0.5, "keep_masks": True, **kw}))


def test_graph_replay_equals_eager_and_differs_from_dense(golden):
    pipe, args = _pipe(golden)
    pipe.use_hip_graph = False
    dense = pipe.denoise(*args)
    _sparse(pipe)
    eager = pipe.denoise(*args)
    tr = pipe.transformer
    assert any(k[0] == "sparse" and k[4] == NID for k in tr._rope_cache)          # id_frames reached the model
    dens = tr.sparse_attention_density()
    print(f"densities after the eager loop: {dens}")
    assert sorted(dens) == list(range(len(tr.blocks))) and all(0.0 < d < 1.0 for d in dens.values())
    pipe.use_hip_graph = True                                          # a failed capture is an error
    graphed = pipe.denoise(*args)
    assert torch.equal(eager, graphed)
    assert torch.isfinite(eager).all() and not torch.equal(eager, dense)
    rel = ((eager - dense).pow(2).mean().sqrt() / dense.pow(2).mean().sqrt()).item()
    print(f"sparse vs dense latents after 4 steps: rel-RMS {rel:.3e}")
    pipe.use_hip_graph = None                                          # the default: still the graph loop
    assert torch.equal(pipe.denoise(*args), eager)
    # a threshold of 1, and forced tiles that cover the clip: the dense loop, bit for bit
    _sparse(pipe, cdf_threshold=1.0)
    assert torch.equal(pipe.denoise(*args), dense)
    _sparse(pipe, window_frames=FG + NID)
    assert torch.equal(pipe.denoise(*args), dense)


def test_a_parallel_plan_is_refused(golden):
    pipe, args = _pipe(golden)
    _sparse(pipe)
    pipe.parallel = object()
    with pytest.raises(NotImplementedError, match="sparse attention runs on one GPU"):
        pipe.denoise(*args)


def test_the_examples_flags_parse():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "run_wan_frameino.py"), "--help"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "--sparse-attention TAU" in r.stdout and "--sparse-window-frames N" in r.stdout
