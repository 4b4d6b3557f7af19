#!/usr/bin/env python3
"""Generate tests/golden/k1_forms_edges_sha.npz: the SHA-256 of the float32 grid of every K1 form at every shape of
tests/test_gpu_k1_forms_edges.py.

Run on an MI355X, against the build whose bits are to be pinned (``APAP_HIP_LIB`` loads a library other than the in-tree
one: the committed fixture was recorded from a build of the commit before the solve kernels' shared steps were given one
definition each):

    APAP_HIP_LIB=/path/to/libapap_hip.so python tests/golden/make_k1_forms_edges_golden.py [out.npz]

The inputs, the forms and the key of every entry are those of the test module, imported from it: the two cannot drift apart.
A grid that is not finite is an error here - the fixture never records one.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import torch  # noqa: E402,F401  (in the process before the library is loaded, as in tests/conftest.py)
from cvx_proj_amd import _native  # noqa: E402
import test_gpu_k1_forms_edges as T  # noqa: E402


def main(out_path):
    print(f"library: {_native.LIB_PATH}")
    assert _native.lib().apap_device_count() >= 1, "no GPU"
    sums = {}
    for cells, n, batch in T.SHAPES:
        out, _, _, _ = T.solve_forms(_native, cells, n, batch)
        for form, H in out.items():
            assert np.isfinite(H).all(), f"cells={cells} n={n} batch={batch} {form}: not finite"
            sums[T.key(cells, n, batch, form)] = T.sha(H)
        print(f"cells={cells} n={n} batch={batch}: {len(out)} forms, {len(set(s.tobytes() for s in map(T.sha, out.values())))} distinct grids")
    np.savez(out_path, **sums)
    print(f"wrote {out_path}: {len(sums)} digests")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "k1_forms_edges_sha.npz"))
