"""Spectral weights on the MI355X against the reference's own calculate_M (tests/golden/spectral_*.npz, made by
tests/golden/make_golden_spectral.py).  Tolerances (include/apap_hip.h): off-diagonal M bit-identical, diagonal
within 4 fp64 ulp, segment within 1e-9, bool mask and original mask equal, ransac_mask within 1 float32 ulp, lambda within
1e-12 of eigvalsh."""
import glob
import os
import warnings

import numpy as np
import pytest

from conftest import GOLDEN, ulp_diff_f32

pytestmark = pytest.mark.gpu

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "spectral_*.npz")))


def load(path):
    g = dict(np.load(path))
    if "codebook" in g:     # the largest case stores its descriptors as rows of a codebook
        g["c_feats"], g["o_feats"] = g["codebook"][g["c_index"]], g["codebook"][g["o_index"]]
    g["c"] = g["c_feats"].astype(np.float32)
    g["o"] = g["o_feats"].astype(np.float32)
    return g


class KP:
    def __init__(self, x, y):
        self.pt = (float(x), float(y))


class DM:
    def __init__(self, q, t):
        self.queryIdx, self.trainIdx = q, t


class Opts:
    def __init__(self, v):
        self.epi_weight, self.affinity_eps, self.aff_thresh, self.em_radius, self.score_thresh = (float(x) for x in v)


def kw(g):
    e, a, t, r, s = (float(x) for x in g["opts"])
    return dict(epi_weight=e, affinity_eps=a, aff_thresh=t, em_radius=r, score_thresh=s)


def check_outputs(g, seg, rm, om):
    aff = float(g["opts"][2])
    assert np.abs(seg - g["segment"]).max() <= 1e-9
    assert np.array_equal(seg > aff, g["segment"] > aff)
    assert np.array_equal(om, g["original_mask"])
    assert ulp_diff_f32(rm, g["ransac_mask"]).max() <= 1


@pytest.fixture(scope="module")
def spectral(native):
    from cvx_proj_amd import spectral_method
    if native.lib().apap_device_count() < 1:
        pytest.skip("no HIP device")
    return spectral_method


@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
def test_spectral_weights_match_reference(spectral, path):
    g = load(path)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        r = spectral.spectral_weights(g["src"], g["dst"], g["c"], g["o"], g["F"], Hg=g.get("Hg"), mask=g.get("mask"), **kw(g))
    check_outputs(g, r.segment, r.ransac_mask, r.original_mask)
    assert r.converged and r.residual <= 1e-13
    assert abs(r.lam - float(g["lam"])) <= 1e-12 * abs(float(g["lam"]))
    assert r.steps >= 1 and (len(g["src"]) == 1 or r.gap > 0)


@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
def test_calculate_M_surface(spectral, native, path):
    g = load(path)
    n = len(g["src"])
    kc, ko = [KP(*p) for p in g["src"]], [KP(*p) for p in g["dst"]]
    matches = [DM(i, n - 1 - i) for i in range(n)]         # trainIdx != queryIdx: the lookup goes through the match
    ko = ko[::-1]
    c, o = g["c"], g["o"][::-1].copy()
    if "Hg" in g:
        seg, H, rm, om = spectral.calculate_M(kc, c, ko, o, g["F"], matches, Opts(g["opts"]), Hg=g["Hg"])
        assert H is g["Hg"]
        check_outputs(g, seg, rm, om)
    elif n < 4:     # cv.findHomography refuses fewer than 4 points; so does this repository's RANSAC
        with pytest.raises(native.ApapError):
            spectral.calculate_M(kc, c, ko, o, g["F"], matches, Opts(g["opts"]))
    else:
        # no Hg: the mask comes from this repository's GPU RANSAC (swap=True: other image -> centre), not cv's
        seg, H, rm, om = spectral.calculate_M(kc, c, ko, o, g["F"], matches, Opts(g["opts"]))
        assert np.abs(seg - g["segment"]).max() <= 1e-9
        _, mask = native.find_homography_ransac(g["dst"], g["src"], 5.0)
        assert np.array_equal(om, mask.ravel().astype(np.float32))
        aff = float(g["opts"][2])
        want = np.where(seg > aff, seg.astype(np.float32), om * np.float32(aff))
        assert np.array_equal(rm, want)


@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
def test_resident_form(spectral, native, path):
    import torch
    from cvx_proj_amd import resident
    g = load(path)
    dev = torch.device("cuda", 0)

    def t(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)

    status = torch.zeros(1, dtype=torch.int32, device=dev)
    seg, rm, om, info = resident.hip_spectral(
        t(g["src"], np.float32), t(g["dst"], np.float32), t(g["c"], np.float32), t(g["o"], np.float32), t(g["F"], np.float64),
        native.spectral_params(*g["opts"]), Hg=None if "Hg" not in g else t(g["Hg"], np.float32),
        mask=None if "mask" not in g else t(g["mask"], np.float32), status=status)
    torch.cuda.synchronize()
    check_outputs(g, seg.cpu().numpy(), rm.cpu().numpy(), om.cpu().numpy())
    info = info.cpu().numpy()
    assert int(status.cpu()[0]) == 0 and info[3] == 0
    assert abs(info[0] - float(g["lam"])) <= 1e-12 * abs(float(g["lam"]))


@pytest.mark.parametrize("path", [p for p in FIXTURES if "M_off" in np.load(p).files], ids=os.path.basename)
def test_affinity_matches_reference_M(native, path):
    g = load(path)
    M = native.spectral_affinity(g["src"], g["dst"], g["c"], g["o"], g["F"], native.spectral_params(*g["opts"]))
    d = np.diag(M).copy()
    off = M.copy()
    np.fill_diagonal(off, 0)
    assert np.array_equal(off.astype(np.float32).astype(np.float64), off)
    assert off.astype(np.float32).view(np.uint32).tobytes() == g["M_off"].view(np.uint32).tobytes()
    ulp = np.spacing(np.abs(g["M_diag"]))
    assert (np.abs(d - g["M_diag"]) <= 4 * ulp).all()
    lam = np.linalg.eigvalsh(M)
    lam = lam[np.argmax(np.abs(lam))]
    assert abs(lam - float(g["lam"])) <= 1e-12 * abs(float(g["lam"]))


def test_restart_cap_sets_status_and_warns(spectral, native):
    g = load(os.path.join(GOLDEN, "spectral_n500.npz"))
    with pytest.warns(RuntimeWarning, match="did not reach"):
        r = spectral.spectral_weights(g["src"], g["dst"], g["c"], g["o"], g["F"], mask=g["mask"], max_restarts=1, **kw(g))
    assert not r.converged and r.restarts == 1
    seg, rm, om, info = native.spectral_weights(g["src"], g["dst"], g["c"], g["o"], g["F"],
                                                native.spectral_params(*g["opts"], max_restarts=1), mask=g["mask"])
    assert int(info[3]) & native.STATUS_NO_CONVERGENCE
    assert np.isfinite(seg).all() and seg.max() == 1.0


def test_profile_slot_counts_a_call(native):
    g = load(os.path.join(GOLDEN, "spectral_n64_hg.npz"))
    ctx = native.Context(profile=1)
    native.spectral_weights(g["src"], g["dst"], g["c"], g["o"], g["F"], native.spectral_params(*g["opts"]), Hg=g["Hg"], ctx=ctx)
    prof = ctx.profile_read()
    assert prof["spectral"][1] == 1 and prof["spectral"][0] > 0
    assert all(cnt == 0 for k, (ms, cnt) in prof.items() if k != "spectral")
