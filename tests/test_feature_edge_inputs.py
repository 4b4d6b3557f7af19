"""The inputs of tests/feature_edge_cases.py reach the edges they were built for: asserted from the numpy specifications alone
(tests/corner_spec.py, tests/sift_spec.py), so that tests/test_gpu_feature_edges.py cannot pass without exercising them.  The
constants named here (the corner tile, its list of 512 entries, the LDS sort of 2048, the seven 8-bit radix digits) are those
of csrc/apap_corner.hip."""
import numpy as np
import pytest

import corner_spec as C
import feature_edge_cases as E
import sift_spec as S

TILE_H, TILE_W, LIST_MAX, LDS_SORT = 32, 64, 512, 2048


def corners(img, radius=1):
    """(mask, responses of the corners by response descending then index ascending)."""
    R = C.response(img)
    mask = C.corner_mask(R, radius)
    return mask, C.detect(img, C.bound(img.shape[0], img.shape[1], radius), radius, 0)[1]


def test_dense_image_fills_the_block_list_and_has_one_large_group():
    img = E.dense_image()
    assert img.shape == (96, 128) and C.bound(TILE_H, TILE_W, 1) == LIST_MAX
    mask, resp = corners(img)
    per_tile = {(y0, x0): int(mask[y0:y0 + TILE_H, x0:x0 + TILE_W].sum()) for y0 in (0, 32, 64) for x0 in (0, 64)}
    assert per_tile[(32, 0)] == LIST_MAX and per_tile[(32, 64)] == LIST_MAX          # the list exactly full, twice
    assert per_tile[(0, 0)] == 496 and per_tile[(64, 64)] == 496
    assert int(mask.sum()) == 3008 == len(resp) and C.bound(96, 128, 1) == 3072
    values, counts = np.unique(resp, return_counts=True)
    assert counts.max() == 2790 >= LDS_SORT + 1                                      # a cut inside it sorts in the workspace
    group = values[counts.argmax()]
    first = int(np.flatnonzero(resp == group)[0])
    assert first == 126 and np.all(resp[first:first + 2790] == group)                # rows 126 .. 2915: 2048 and 2049 cut inside
    assert int(np.count_nonzero(1000 * resp >= 1000 * resp[0])) == 62                # quality 1000: the strongest group alone
    assert int(np.count_nonzero(1000 * resp >= 500 * resp[0])) == 2917               # quality 500 keeps the large group


def test_binary_image_reaches_the_top_radix_digit_and_8192_candidates():
    img = E.binary_image()
    assert img.shape == (256, 320) and set(np.unique(img).tolist()) == {0, 255}
    mask, resp = corners(img)
    assert len(resp) == 5399 > 4096                                                  # padded to 8192 for the sort
    top = resp >> 48
    assert int(np.count_nonzero(top)) == 17 and int(top.max()) == 1 and resp[0] < 1 << 56
    assert int(np.count_nonzero(top[:200] == 0)) == 183                              # a cut at 100 selects below the top digit's group
    assert 1000 * int(resp[0]) < 1 << 63
    assert resp[9] != resp[10] and resp[99] != resp[100]
    assert resp[4095] == resp[4096] == resp[4097]                                    # 4096 and 4097 cut through equal responses


def test_prototype_scene_straddles_the_lds_sort():
    img = C.prototype_scene()
    mask, resp = corners(img)
    assert len(resp) == 2324 > LDS_SORT + 1
    assert resp[2046] != resp[2047] != resp[2048] != resp[2049]      # chosen is exactly 2048, then 2049: either side of kLdsSort


def test_structured_images_have_exact_gradient_values_and_saturated_rows():
    imgs = E.structured_images()
    assert list(imgs) == ["vertical step", "horizontal step", "ramp", "diagonal step", "bright pixel"]
    got = {name: E.gradient_classes(g) for name, g in imgs.items()}
    print(got)
    # rows equal: dy is exactly 0; dx differs from 0 in the 14 columns within the 13 taps and the difference of the step
    assert got["vertical step"] == {"dx0": 0, "dy0": 14 * 38, "diag": 0, "both0": 38 * 48 - 14 * 38}
    assert got["horizontal step"] == {"dx0": 14 * 48, "dy0": 0, "diag": 0, "both0": 38 * 48 - 14 * 48}
    assert got["ramp"] == {"dx0": 0, "dy0": 38 * 48, "diag": 0, "both0": 0}
    assert got["diagonal step"] == {"dx0": 0, "dy0": 0, "diag": 730, "both0": 930}
    assert got["bright pixel"] == {"dx0": 38, "dy0": 38, "diag": 20, "both0": 1604}
    for key in ("dx0", "dy0", "diag", "both0"):
        assert sum(g[key] for g in got.values()) > 0
    h, w = E.STRUCTURED_SHAPE
    pts = E.every_pixel_and_a_ring(h, w)
    assert pts.shape == ((h + 4) * (w + 4), 2) and pts.dtype == np.float32 and np.array_equal(pts[0], [0, 0])
    assert np.array_equal(pts[h * w], [-2, -2]) and pts[:, 0].max() == w + 1 and pts[:, 1].max() == h + 1
    saturated = {}
    for name, g in imgs.items():
        f = S.describe(g, pts)
        assert f.tobytes() == S.describe(E.bgr(g), pts).tobytes()                   # three equal planes: the grey plane back
        saturated[name] = int((f == 255).any(axis=1).sum())
    print(saturated)
    assert saturated == {"vertical step": 276, "horizontal step": 316, "ramp": 224, "diagonal step": 798, "bright pixel": 236}
    assert all(saturated[name] > 100 for name in E.STEP_IMAGES)


@pytest.mark.parametrize("n", [9, 65])
def test_batch_images_are_mixed(n):
    imgs = E.batch_images(n)
    assert len(imgs) == n and {im.ndim for im in imgs} == {2, 3} and all(im.dtype == np.uint8 for im in imgs)
    sides = [im.shape[:2] for im in imgs]
    assert (7, 7) in sides and (40, 50) in sides and min(min(s) for s in sides) == 7 and len(set(sides[:4])) == 4
