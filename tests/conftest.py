import glob
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def golden_arrays(name):
    """the arrays of fixture `name` in their recorded order: tests/golden/<name>.npz, or a fixture too large for one committed
    file spread over <name>.part<i>.npz, its largest arrays cut along axis 0 into `<key>#<j>` pieces
    (tools/golden/make_golden.py::savez_parts)"""
    path = os.path.join(GOLDEN, name + ".npz")
    if os.path.exists(path):
        with np.load(path) as z:
            return {k: z[k] for k in z.files}
    parts = sorted(glob.glob(os.path.join(GOLDEN, glob.escape(name) + ".part*.npz")),
                   key=lambda p: int(p[:-len(".npz")].rsplit(".part", 1)[1]))
    assert parts, f"no fixture {name} under {GOLDEN}"
    out, pieces = {}, {}
    for p in parts:
        with np.load(p) as z:
            for k in z.files:
                base, cut, j = k.rpartition("#")
                if cut:
                    out.setdefault(base, None)
                    pieces.setdefault(base, {})[int(j)] = z[k]
                else:
                    out[k] = z[k]
    for k, d in pieces.items():
        out[k] = np.concatenate([d[j] for j in range(len(d))])
    return out


def load_golden(name):
    cfg, sd, arr = {}, {}, {}
    for k, v in golden_arrays(name).items():
        if k.startswith("cfg/"):
            v = v.tolist()
            cfg[k[4:]] = tuple(v) if isinstance(v, list) and k.endswith("patch_size") and len(v) == 3 else v
        elif k.startswith("sd/"):
            sd[k[3:]] = torch.from_numpy(v)
        else:
            arr[k] = torch.from_numpy(v) if v.dtype.kind in "fiub" else v
    return cfg, sd, arr


@pytest.fixture(scope="session")
def golden():
    return load_golden
