#!/usr/bin/env python3
"""Generate tests/golden/model_digests.json: the SHA-256 of H, info and status of every solve of
tests/test_gpu_model_digests.py.

Run on an MI355X, against the build whose bits are to be pinned (``APAP_HIP_LIB`` loads a library other than the in-tree
one: the committed fixture was recorded from a build of the commit before the M-step kernels' shared steps were given one
definition each):

    APAP_HIP_LIB=/path/to/libapap_hip.so python tests/golden/make_model_digests_golden.py [out.json]

The inputs and the key of every entry are those of the test module, imported from it: the two cannot drift apart.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import torch  # noqa: E402,F401  (in the process before the library is loaded, as in tests/conftest.py)
from cvx_proj_amd import _native  # noqa: E402
import test_gpu_model_digests as T  # noqa: E402


def main(out_path):
    print(f"library: {_native.LIB_PATH}")
    assert _native.lib().apap_device_count() >= 1, "no GPU"
    sums = {}
    for fn, mode in T.GROUPS:
        got = fn(_native, mode)
        assert not set(got) & set(sums), "duplicate keys"
        sums.update(got)
        print(f"{fn.__name__} {mode}: {len(got)} digests, {len(set(got.values()))} distinct")
    with open(out_path, "w") as f:
        json.dump(sums, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {out_path}: {len(sums)} digests")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "model_digests.json"))
