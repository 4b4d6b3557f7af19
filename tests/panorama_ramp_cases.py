"""Inputs of the edge-ramp tests that tests/panorama_cases.py does not hold: the oracle's target coordinates of every layer
of its cases, and the input that fills the ramp's accumulators.  Built once per session and shared: read-only."""
import numpy as np

import panorama_cases as E

ALL_CASES = sorted(E.HOST_CASES) + sorted(E.TILING_CASES)
CONSTANT = ("two_pixels", "white17")        # every weight is 1 / every value is 255: the ramp cannot differ from the mean

_coords = {}
_saturation = {}


def layer_coords(layer):
    """(tx, ty) of one layer's pair canvas by the oracle: float32 inverses of the cells, then the float64 chain."""
    from oracle import apap_oracle as O
    return O.warp_coords_fast(O.invert_cells_f32(layer.local_homography), layer.mesh, layer.final_size, layer.offset)


def oracle_coords(name):
    """Per layer of the case ``name`` of tests/panorama_cases.py, the oracle's (tx, ty)."""
    if name not in _coords:
        _coords[name] = [layer_coords(l) for l in E.get(name)["layers"]]
    return _coords[name]


def engine_coords(native, layers):
    """Per layer the engine's own coordinates (``_native.warp_coords``) as (tx, ty)."""
    out = []
    for l in layers:
        c = native.warp_coords(l.local_homography, l.mesh[0], l.mesh[1], l.final_size[0], l.final_size[1], l.offset[0], l.offset[1])
        out.append((c[..., 0], c[..., 1]))
    return out


def saturation(white=False):
    """A 512 x 512 centre and 16 layers that are ONE 512 x 512 picture object, each placed on the centre through a 1 x 1 mesh:
    around the middle all 17 samples are 256 or more pixels from their borders, so with ramp = 256 the weight sum reaches
    17 x 256 = 4352 - and, with ``white`` (every byte 255), the weighted sums 4352 x 255 = 1 109 760.  The case carries the
    oracle's coordinates of its layers (all 16 are the same array)."""
    if white not in _saturation:
        rng = np.random.default_rng(4352)
        center = E.picture(rng, 512, 512)
        img = E.picture(rng, 512, 512)
        if white:
            center, img = np.full_like(center, 255), np.full_like(img, 255)
        layers = [E.make_layer(rng, center.shape, 512, 512, E.placement(0.0, 0.0), 1, 1, img=img) for _ in range(16)]
        geos = [tuple(l.final_size) + tuple(l.offset) for l in layers]
        assert geos == [(512, 512, 0, 0)] * 16 and all(l.img is img for l in layers)
        _saturation[white] = dict(center=center, layers=layers, geometries=geos, coords=[layer_coords(layers[0])] * 16)
    return _saturation[white]
