"""What guided matching buys, by the specification alone (no GPU): the look-alike scene of the issue, and the reference
fixture - every match ``rematch`` selects is one the reference's ``recompute_matching`` keeps."""
import numpy as np

import guided_match_spec as S


def test_look_alike_scene_unguided_against_gated():
    q_pts, q_desc, t_pts, t_desc, H, perm = S.scene(0)
    unguided = S.MS.match_int(q_desc, t_desc)[0]
    rec_q, rec_t = S.scene_records(q_pts, t_pts, H)
    r2 = 36.0
    idx, dist, idx2, dist2, count, ridx, rdist = S.match_int(q_desc, t_desc, rec_q, rec_t, S.KIND_POINT, r2)
    share_unguided, share_gated = float(np.mean(unguided == perm)), float(np.mean(idx == perm))
    margin = float(np.abs(S.gate_value(rec_q, rec_t, S.KIND_POINT)[0] / r2 - 1).min())
    print(f"correct partner: unguided {share_unguided:.3f}, gated at 6 px {share_gated:.3f}; candidates per query mean "
          f"{count.mean():.2f} max {count.max()}; nearest gate value to r2: {margin:.3g} relative")
    assert share_unguided <= 0.5 and share_gated >= 0.95
    assert margin > 1e-3
    assert q_pts.shape == (200, 2) and t_pts.shape == (300, 2) and q_pts.dtype == t_pts.dtype == np.float32
    assert 1.0 <= count.mean() <= 2.0


def test_records_follow_the_written_order():
    pts = np.float32([[3, 4], [0.1, -7.25]])
    M = np.arange(1.0, 10.0).reshape(3, 3) / 7
    X, Y = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    line = S.records(pts, M, S.LINE)
    for r in range(3):
        assert np.array_equal(line[:, r], (M[r, 0] * X + M[r, 1] * Y) + M[r, 2])
    proj = S.records(pts, M, S.PROJECT)
    assert np.array_equal(proj, np.stack([line[:, 0] / line[:, 2], line[:, 1] / line[:, 2], np.ones(2)], 1))
    assert np.array_equal(S.records(pts), np.stack([X, Y, np.ones(2)], 1))


def test_the_reference_keeps_every_rematch(golden):
    g = golden("guided_ref")
    em_radius, score_thresh = float(g["em_radius"]), float(g["score_thresh"])
    qi, ti, dist = S.rematch(g["pts_c"], g["feats_c"], g["pts_o"], g["feats_o"], g["H"], em_radius, score_thresh)
    assert np.array_equal(qi, g["query_idx"]) and np.array_equal(ti, g["train_idx"]) and np.array_equal(dist, g["distance"])
    assert len(qi) >= 150 and g["reference_mask"].shape == qi.shape
    assert (g["reference_mask"] == 1).all()      # every match we return is one the reference would have kept
    # the seed was chosen off both thresholds
    rec_q, rec_t = S.records(g["pts_c"]), S.records(g["pts_o"], g["H"], S.PROJECT)
    near_r = np.abs(np.sqrt(S.gate_value(rec_q, rec_t, S.KIND_POINT)[0]) - em_radius).min()
    near_s = np.abs(S.score(np.float32(g["feats_c"]), np.float32(g["feats_o"]), qi, ti) - score_thresh).min()
    assert near_r >= 1e-6 and near_s >= 1e-6
    assert np.mean(ti == g["perm"][qi]) >= 0.95
