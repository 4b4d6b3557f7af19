#!/usr/bin/env python3
"""Generate tests/golden/sfm_ref.npz FROM THE REFERENCE'S OWN sfm_test.py and utils.py.

    MPLBACKEND=Agg python tests/golden/make_sfm_golden.py <the reference's pyviz directory>

It imports the reference's ``sfm_test.py`` in place (nothing is copied) behind an in-memory ``cv2`` stub - the module only
names ``cv.DMatch`` / ``cv.KeyPoint`` at import - and records, for the seeded inputs of tests/sfm_cases.py:

  tracks_<case>_table / _pts    what its ``get_covid`` returns (rows of 4: cases of fewer views are padded with empty views)
  rays_dirs                     its ``utils.world_frame_ray_dir`` on the pixels of a camera case (its prints swallowed)
  tri_X                         its ``solve_3d_position`` on every track of the ray case
  tri_smin                      the smallest singular value of each track's A, as numpy's SVD gives it
  signatures                    the argument names of its public functions, ``name:arg,arg,...``

Only these outputs go into the file; the inputs are regenerated from their seeds by the tests.
"""
import contextlib
import inspect
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(REPO, "tests"))

import sfm_cases as C  # noqa: E402


class DMatch:
    def __init__(self, queryIdx, trainIdx):
        self.queryIdx, self.trainIdx = queryIdx, trainIdx


def import_reference(ref_dir):
    os.environ.setdefault("MPLBACKEND", "Agg")
    cv2 = types.ModuleType("cv2")
    cv2.DMatch = DMatch
    cv2.KeyPoint = type("KeyPoint", (), {})
    sys.modules["cv2"] = cv2
    sys.path.insert(0, ref_dir)
    import sfm_test as ref  # noqa: E402
    import utils as ref_utils  # noqa: E402
    return ref, ref_utils


def reference_tracks(ref, views):
    views = list(views) + [(np.zeros((0, 2), np.float32), np.zeros(0, np.int32))] * (4 - len(views))      # its rows are 4 long
    src = [[p.reshape(1, 2).copy() for p in pts] for pts, _ in views]
    matches = [[DMatch(0, int(t)) for t in idx] for _, idx in views]
    res, covid = ref.get_covid(src, matches)
    return np.array(covid, np.int32).reshape(-1, 4), np.array(res, np.float32).reshape(-1, 2)


def main():
    ref, ref_utils = import_reference(sys.argv[1])
    out = {}
    for name in C.REFERENCE_TRACK_CASES:
        table, pts = reference_tracks(ref, C.track_cases()[name])
        out[f"tracks_{name}_table"], out[f"tracks_{name}_pts"] = table, pts
        print(name, "tracks", len(table), "seen in 2+ views", int(((table >= 0).sum(1) > 1).sum()))
    cam = C.camera_case(4, 16, seed=21)
    pix = np.concatenate([cam["track_pts"], cam["dst_pts"][:16]]).astype(np.float32).reshape(-1, 2, 1)
    Rs = np.stack([cam["R"][k % len(cam["R"])] for k in range(len(pix))])
    with contextlib.redirect_stdout(io.StringIO()):
        out["rays_dirs"] = ref_utils.world_frame_ray_dir(np.linalg.inv(cam["K"]), pix, Rs)
    o, d, off = C.ray_case(**C.RAY_CASE)
    X, smin = [], []
    for k in range(len(off) - 1):
        ok, dk = o[off[k]:off[k + 1], :, None], d[off[k]:off[k + 1], :, None]
        X.append(ref.solve_3d_position(ok, dk).ravel())
        smin.append(np.linalg.svd((np.eye(3) - dk @ dk.transpose(0, 2, 1)).sum(0))[1][-1])
    out["tri_X"], out["tri_smin"] = np.array(X), np.array(smin)
    print("ray case:", len(X), "tracks,", int((out["tri_smin"] < 1e-3).sum()), "clamped,",
          int(((out["tri_smin"] > 5e-4) & (out["tri_smin"] < 2e-3)).sum()), "inside the threshold band")
    names = ("has_affinity", "match_all", "get_covid", "solve_3d_position", "covid_3d_optimize")
    sigs = [f"{n}:{','.join(inspect.signature(getattr(ref, n)).parameters)}" for n in names]
    sigs.append("world_frame_ray_dir:" + ",".join(inspect.signature(ref_utils.world_frame_ray_dir).parameters))
    out["signatures"] = np.array(sigs)
    path = os.path.join(HERE, "sfm_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
