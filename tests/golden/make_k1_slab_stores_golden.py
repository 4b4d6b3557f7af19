#!/usr/bin/env python3
"""Generate tests/golden/k1_slab_stores_sha.npz: the SHA-256 of the whole moment workspace and of the float32 grid of every
solve of tests/test_gpu_k1_slab_stores.py.

Run on an MI355X, against the build whose bits are to be pinned (``APAP_HIP_LIB`` loads a library other than the in-tree
one).  The committed fixture was recorded from a build of commit fe66469 ("Add bilinear sampling to the local warp, the stitch
and the panorama"), the commit before k_assemble_mfma's epilogue wrote the slab in whole lines: its stores went straight from
the MFMA D layout.

    APAP_HIP_LIB=/path/to/libapap_hip.so python tests/golden/make_k1_slab_stores_golden.py [out.npz]

The inputs, the cases and the key of every entry are those of the test module, imported from it: the two cannot drift apart.
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
import test_gpu_k1_slab_stores as T  # noqa: E402


def main(out_path):
    print(f"library: {_native.LIB_PATH}")
    assert _native.lib().apap_device_count() >= 1, "no GPU"
    sums = {}

    def record(case, form, gamma, sigma, table=None):
        work, H, nbytes = T.solve(case, form, gamma, sigma, table)
        assert (work[nbytes:] == T.FILL).all(), "the bytes behind the workspace were written"
        k = T.key(case, form, gamma, sigma, table)
        sums[k + "_work"], sums[k + "_H"] = T.sha(work[:nbytes]), T.sha(H)

    for case in T.CASES:
        for form in T.FORMS:
            for gamma, sigma in T.WEIGHTINGS:
                record(case, form, gamma, sigma)
        print(f"{T.case_id(case)}: {len(T.FORMS) * len(T.WEIGHTINGS)} solves")
    record(T.CAREFUL, "m30", 0.0, 3.0)
    record(T.WRONG_TABLE, "m30", *T.WEIGHTINGS[0], 24)
    np.savez(out_path, **sums)
    print(f"wrote {out_path}: {len(sums)} digests")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "k1_slab_stores_sha.npz"))
