#!/usr/bin/env python3
"""Generate tests/golden/denoise_notch_ref.npz FROM THE REFERENCE'S OWN median_filter (pyviz/median_filter.py:97-126).

    python tests/golden/make_denoise_golden.py <the reference's pyviz directory>

It imports the reference's ``median_filter.py`` in place (nothing is copied) behind in-memory ``cv2`` and ``matplotlib``
stubs - the module only names them - and runs its ``median_filter`` over the schedule of ``apply_median_filter`` (:143-155,
with each case's r, spacing and sn: the list ``denoise_spec.notch_schedule`` gives, which the fixture's
``schedule_default`` - recorded from the reference's own ``apply_median_filter`` - pins) on the seeded complex128 spectra of tests/denoise_cases.py.  No transform is involved, so
numpy's FFT dtype cannot enter.  For the cases marked "points" the fixture stores the positions the reference changed and their
new values; for those marked "digest" (768 x 768 with the defaults, and r = 6, whose written discs would take 90 KB as
positions) the SHA-256 of the result and the medians of its discs.  Entries the committed fixture already holds must come out
bit for bit as they are: the generator asserts it before it writes.

It also runs the reference's whole ``apply_median_filter`` (equalisation stubbed by the oracle's) once on a seeded picture and
prints its distance from tests/denoise_spec.py: under a numpy whose ``fft2`` keeps float32 input in complex64 that distance is
single-precision rounding.  It is reported in DESIGN.md; no test rests on it.
"""
import hashlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REPO)

import denoise_cases as C  # noqa: E402
import denoise_spec as S  # noqa: E402
from oracle import frontend_oracle as F  # noqa: E402


def import_reference(ref_dir):
    cv2 = types.ModuleType("cv2")
    cv2.equalizeHist = F.equalize_hist_channel
    sys.modules["cv2"] = cv2
    mpl = types.ModuleType("matplotlib")
    mpl.pyplot = types.ModuleType("matplotlib.pyplot")
    sys.modules.setdefault("matplotlib", mpl)
    sys.modules.setdefault("matplotlib.pyplot", mpl.pyplot)
    sys.path.insert(0, ref_dir)
    import median_filter as ref  # noqa: E402
    return ref


def run_reference(ref, f, spacing, r, sn):
    """The reference's ``median_filter`` called once per entry of the schedule; ``img`` only gives it the shape."""
    img = np.zeros(f.shape, np.uint8)
    f = f.copy()
    for uk, vk, r1, r2 in S.notch_schedule(spacing, r, sn):
        f = ref.median_filter(img, f, uk, vk, r1, r2)
    return f


def reference_schedule(ref):
    """What the reference's own ``apply_median_filter`` hands to ``median_filter``, call by call: (uk, vk, radius1, radius2)."""
    seen = []
    real = ref.median_filter

    def recorder(img, f, uk, vk, radius1=10, radius2=10):
        seen.append((uk, vk, radius1, radius2))
        return f

    ref.median_filter = recorder
    try:
        ref.apply_median_filter(C.picture(16, 16, 3))
    finally:
        ref.median_filter = real
    return np.array(seen, np.int32)


def main():
    ref = import_reference(sys.argv[1])
    out = {"schedule_default": reference_schedule(ref)}     # the reference's own loop, which notch_schedule restates
    assert out["schedule_default"].tolist() == [list(c) for c in S.notch_schedule(48, 5, 9)]
    for name in C.NOTCH_CASES:
        f0 = C.notch_input(name)
        p = C.notch_params(name)
        got = run_reference(ref, f0, **p)
        trace = []
        S.notch_spec(f0, trace=trace, **p)
        changed = np.flatnonzero((got != f0).ravel())
        print(name, f0.shape, p, "changed", len(changed), "assignments", len(trace), "empty", sum(t["n"] == 0 for t in trace))
        if name in C.SMALL_CASES:
            out[f"{name}_at"] = changed.astype(np.int32)
            out[f"{name}_values"] = got.ravel()[changed]
        else:
            out[f"{name}_sha256"] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(got).tobytes()).digest(), np.uint8)
            out[f"{name}_medians"] = np.array([t["median"] for t in trace if t["n"]], np.complex128)
    path = os.path.join(HERE, "denoise_notch_ref.npz")
    if os.path.exists(path):    # a new case adds entries; what the fixture held before stays, bit for bit
        with np.load(path) as before:
            for key in before.files:
                assert key in out and out[key].dtype == before[key].dtype and out[key].shape == before[key].shape \
                    and out[key].tobytes() == before[key].tobytes(), f"{key} differs from the committed fixture"
            print("the", len(before.files), "entries of the fixture as it was are unchanged;", len(out) - len(before.files), "added")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    # the reference's whole chain under the installed numpy, for DESIGN.md
    pic = C.picture(768, 768, 42)
    new, _, _, eq = ref.apply_median_filter(pic)
    spec = S.denoise_spec(pic, spacing=48, r=5, sn=9)
    print("apply_median_filter (numpy %s) against denoise_spec at 768 x 768: max |difference| %.3e of max %.1f; equalisation equal: %s"
          % (np.__version__, np.abs(new - spec).max(), spec.max(), np.array_equal(eq, F.equalize_hist_channel(pic))))


if __name__ == "__main__":
    main()
