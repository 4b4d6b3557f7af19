"""Inputs of the two-band blend's tests that tests/panorama_cases.py and tests/panorama_ramp_cases.py do not hold.  Each is a
dict like theirs (``center``, ``layers``, ``geometries``) with ``coords``, the oracle's target coordinates of its layers.
Built once per session and shared: read-only.  tests/test_panorama_band_host.py shows that each reaches its edge."""
import numpy as np

import panorama_cases as E
import panorama_ramp_cases as RC

_cache = {}


def _finish(center, layers):
    return dict(center=center, layers=layers, geometries=[tuple(l.final_size) + tuple(l.offset) for l in layers],
                coords=[RC.layer_coords(l) for l in layers])


def clamp():
    """Overlapping views with bytes in {1, 255} (never 0: that is absence): the centre is noise at the scale of a pixel, a layer
    to its right constant 255 and a layer to its left constant 1.  Where the centre gives the detail over a constant view,
    ``c - b`` is about +-127 around a low band L between the centre's local mean b and the constant.  L lies on the constant's
    side of b, so ``L + c - b`` can leave 0 .. 255 only on that side - above 255 over the layer of 255, below 0 over the layer
    of 1: one constant view cannot reach both ends, hence two, each overlapping the noise in a pair of views."""
    if "clamp" not in _cache:
        rng = np.random.default_rng(255)
        center = np.where(rng.integers(0, 2, (40, 48, 3)) == 1, 255, 1).astype(np.uint8)
        high, low = np.full((40, 48, 3), 255, np.uint8), np.full((40, 48, 3), 1, np.uint8)
        layers = [E.make_layer(rng, center.shape, 48, 40, E.placement(26.0, 6.0, 0.01), 2, 2, img=high),
                  E.make_layer(rng, center.shape, 48, 40, E.placement(-26.0, -6.0, -0.01), 3, 2, img=low)]
        _cache["clamp"] = _finish(center, layers)
    return _cache["clamp"]


def layer_ties():
    """Two layers that are the same picture under the same grid, reaching right of a small centre: where the centre is absent
    both are present with the same D, and the first must give the detail."""
    if "layer_ties" not in _cache:
        rng = np.random.default_rng(1414)
        center = E.picture(rng, 20, 16)
        img = E.picture(rng, 24, 20)
        layers = [E.make_layer(rng, center.shape, 24, 20, E.placement(12.0, -1.0, 0.01), 2, 3, img=img) for _ in range(2)]
        assert np.array_equal(layers[0].local_homography, layers[1].local_homography) and layers[0].img is layers[1].img
        _cache["layer_ties"] = _finish(center, layers)
    return _cache["layer_ties"]


def gains(n_views, seed=7):
    """A q per view, all different, between 0.6 and 1.6."""
    rng = np.random.default_rng(seed)
    q = rng.permutation(np.linspace(0.6 * 4096, 1.6 * 4096, n_views).astype(np.int64))
    return [int(v) for v in q]
