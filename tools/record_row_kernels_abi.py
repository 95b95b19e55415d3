"""Record tests/golden/row_kernels_abi.json: the (return code, message) every case of tests/test_row_kernels_abi_cpu.py gets
from the library FINO_LIB_PATH names (default: the built one).  Run it against the library the contract is taken FROM -- the
commit before a change to the host halves -- never against the code under test.  No GPU needed: no case reaches a launch.

    FINO_LIB_PATH=<old checkout>/frameino_amd/lib/libframeino_parent.so python tools/record_row_kernels_abi.py [out.json]"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from frameino_amd import _lib  # noqa: E402
from tests import test_row_kernels_abi_cpu as cases  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else cases.GOLDEN
    recorded = cases.record(_lib.load())
    for name, (rc, message) in recorded.items():
        assert message is None or ("launch" not in message and "hipFuncSetAttribute" not in message), (name, rc, message)
    with open(out, "w") as f:
        json.dump(recorded, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d cases from %s -> %s" % (len(recorded), _lib.LIB_PATH, out))


if __name__ == "__main__":
    main()
