#!/usr/bin/env python3
"""Generate tests/golden/k1_staging_sha.npz: the SHA-256 of the whole moment workspace of every solve of
tests/test_gpu_k1_staging.py.

Run on an MI355X, against the build whose bits are to be pinned (``APAP_HIP_LIB`` loads a library other than the in-tree
one).  The committed fixture was recorded from a build of commit 04ef35b ("Panorama: exposure gain compensation fitted to the
views' overlaps"), the commit before k_assemble_mfma staged its chunks through a buffer window: its loader compared every
row's index with the split's end and stored zeros for the rows behind it.

    APAP_HIP_LIB=/path/to/libapap_hip.so python tests/golden/make_k1_staging_golden.py [out.npz]

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
import test_gpu_k1_staging as T  # noqa: E402


def main(out_path):
    print(f"library: {_native.LIB_PATH}")
    assert _native.lib().apap_device_count() >= 1, "no GPU"
    sums = {}
    for case in T.CASES:
        for kind in T.VERTICES:
            for form in T.FORMS:
                for gamma, sigma in T.WEIGHTINGS:
                    work, nbytes = T.solve(case, kind, form, gamma, sigma)
                    assert (work[nbytes:] == T.FILL).all(), "the bytes behind the workspace were written"
                    T.layout(case, form, nbytes)     # the case has the splits it is meant to have
                    sums[T.key(case, kind, form, gamma, sigma)] = T.sha(work[:nbytes])
        print(f"{T.case_id(case)}: {len(T.VERTICES) * len(T.FORMS) * len(T.WEIGHTINGS)} solves", flush=True)
    np.savez(out_path, **sums)
    print(f"wrote {out_path}: {len(sums)} digests")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "k1_staging_sha.npz"))
