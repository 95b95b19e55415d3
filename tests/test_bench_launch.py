"""`python bench.py --gpus N` must start by itself: the driver's multi-GPU leg may run the bare command.

CPU: the parent starts its ranks as a child `torch.distributed.run` and hands the child's failure on (there is no GPU here,
so the ranks die at `torch.cuda.set_device`) -- no re-exec, no silent success.
GPU: the bare command with 2 gloo ranks on the one GPU prints a line with n_gpus = 2, and the forced-shard rehearsal drives
the N > 1 code path through a real RCCL communicator of one rank.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(args, env_extra=None, timeout=900):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None), env.pop("RANK", None), env.pop("LOCAL_RANK", None)
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, env=env,
                       timeout=timeout, cwd=ROOT)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{"metric"')]
    return p, lines


def test_bare_command_launches_ranks_and_propagates_failure():
    import torch
    if torch.cuda.is_available():
        pytest.skip("CPU-box check (on a GPU box the ranks succeed: see the gpu tests)")
    p, lines = run_bench(["--gpus", "2", "--workload", "tiny", "--steps", "1", "--warmup", "0"])
    assert "starting -m torch.distributed.run" in p.stderr, p.stderr[-2000:]
    assert "--nproc-per-node=2" in p.stderr
    assert p.returncode != 0 and not lines, (p.returncode, lines)


@pytest.mark.gpu
def test_bare_command_two_gloo_ranks_on_one_gpu():
    p, lines = run_bench(["--gpus", "2", "--workload", "tiny", "--steps", "2", "--warmup", "1"],
                         {"FINO_DIST_BACKEND": "gloo"})
    assert p.returncode == 0 and len(lines) == 1, (p.returncode, p.stderr[-3000:])
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 2 and out["value"] > 0
    assert out["config"]["ranks_seen"] == 2 and out["config"]["backend"] == "gloo"


@pytest.mark.gpu
def test_bare_command_eight_gloo_ranks_on_one_gpu():
    """The machine the driver will use is 8 ranks: the bare `bench.py --gpus 8` starts its 8 ranks itself, builds every communicator
    of both plans in the same order on every rank (split: 2 token groups of 4 + 4 cfg pairs; interleave: 2 groups of 8), measures
    split-kv in full, probes the other plan x exchange combinations, and prints exactly ONE line.  gloo on the one GPU: the
    rehearsal of the launch, the groups and the probe protocol -- not of the links."""
    import time
    t0 = time.time()
    p, lines = run_bench(["--gpus", "8", "--workload", "tiny", "--steps", "2", "--warmup", "1", "--full"],
                         {"FINO_DIST_BACKEND": "gloo"}, timeout=600)
    took = time.time() - t0
    assert p.returncode == 0 and len(lines) == 1, (p.returncode, p.stderr[-3000:])
    out = json.loads(lines[0])
    c = out["config"]
    assert out["n_gpus"] == 8 and c["ranks_seen"] == 8 and c["rccl_ranks"] == 8 and c["backend"] == "gloo"
    probes = c["plan_probe_ms_per_step"]
    assert set(probes) == {"cfg2xtoken4", "cfg2xtoken4-heads", "cfg2xtoken4-kvg2", "token8x2branches-interleaved",
                           "token8x2branches-interleaved-heads"}, probes
    assert all(v > 0 for v in probes.values()) and c["parallelism"] in probes
    # round 6: the metric's second half on the ranks -- one real pipe(...) call under the best plan, VAE decode in 8 slabs
    assert c["sec_per_clip_measured"] and c["sec_per_clip_measured"] > 0 and c["vae_decode_slabs"] == 8, c.get("sec_per_clip_measured_what")
    assert "finite=True" in c["sec_per_clip_measured_what"]
    assert took < 420, took                    # (120 s of it is the budget of the run itself; the rest is 8 cold interpreter starts)


@pytest.mark.gpu
@pytest.mark.parametrize("plan,exchange", [("split", "kv"), ("interleave", "kv"), ("interleave", "heads"), ("split", "heads")])
def test_forced_shard_path_through_rccl_of_one_rank(plan, exchange):
    p, lines = run_bench(["--gpus", "1", "--force-shard", "--plan", plan, "--exchange", exchange, "--workload", "tiny",
                          "--steps", "2", "--warmup", "1", "--full"])
    assert p.returncode == 0 and len(lines) == 1, (p.returncode, p.stderr[-3000:])
    out = json.loads(lines[0])
    assert out["n_gpus"] == 1 and out["config"]["ranks_seen"] == 1 and out["config"]["backend"] == "nccl"
    assert out["config"]["parallelism"] != "single"
    assert out["config"]["sec_per_clip_measured"] > 0 and "finite=True" in out["config"]["sec_per_clip_measured_what"]


def test_steps_below_one_is_refused():
    p, lines = run_bench(["--gpus", "1", "--workload", "tiny", "--steps", "0"])
    assert p.returncode == 2 and not lines and "--steps" in p.stderr, (p.returncode, p.stderr[-2000:])


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_last_ones_latents(tmp_path):
    """a plain run: the line carries the headline keys and nothing that --full measures; --dump-outputs writes the latents
    of the last timed step, and the same arguments give the same inputs (the two dumps agree)"""
    import numpy as np
    dumps = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        p, lines = run_bench(["--gpus", "1", "--workload", "tiny", "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)])
        assert p.returncode == 0 and len(lines) == 1, (p.returncode, p.stderr[-3000:])
        out = json.loads(lines[0])
        assert out["steps"] == 3 and out["ms_per_step"] > 0 and abs(out["value"] * out["ms_per_step"] - 1e3) < 1e-3
        assert out["unit"] == "denoise-steps/s" and out["higher_is_better"] is True and out["dtype"] == "bf16"
        assert "roofline" not in out and "cpu_baseline" not in out and "secondary" not in out["config"]
        assert sorted(os.listdir(d)) == ["latents.npy"]
        lat = np.load(d / "latents.npy")
        assert lat.dtype == np.float32 and lat.shape == (4, 3, 8, 12) and np.isfinite(lat).all()
        dumps.append(lat)
    np.testing.assert_allclose(dumps[0], dumps[1], rtol=1e-2, atol=1e-2)
