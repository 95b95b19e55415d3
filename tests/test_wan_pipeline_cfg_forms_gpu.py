"""The Wan loop's CFG execution forms on one GPU -- one batch-2 forward, two forwards one after the other, two forwards on two
streams -- each eager and replayed from the captured step: the same kernels on the same rows, so the same bits (golden
wan_pipe_tiny, no step cache)."""
import pytest
import torch

from tests.test_wan_pipeline_gpu import _pipe, _run

pytestmark = pytest.mark.gpu

FORMS = {"batch_cfg": dict(batch_cfg=True, cfg_streams=False), "sequential": dict(batch_cfg=False, cfg_streams=False),
         "cfg_streams": dict(batch_cfg=True, cfg_streams=True)}


def test_every_cfg_form_eager_and_graphed_equals_the_sequential_eager_loop(golden):
    pipe, a = _pipe(golden)
    outs = {}
    for form, flags in FORMS.items():
        for graph in (False, None):
            pipe.batch_cfg, pipe.cfg_streams, pipe.use_hip_graph = flags["batch_cfg"], flags["cfg_streams"], graph
            outs[form, graph] = _run(pipe, a)
    torch.cuda.synchronize()
    want = outs["sequential", False]
    assert len(outs) == 6 and bool(torch.isfinite(want).all())
    different = [k for k, v in outs.items() if not torch.equal(v, want)]
    assert not different, different
