"""The two-band blend's low-pass picture on the GPU (k_box_blur through apap_box_blur and apap_box_blur_device): byte for byte
``panorama_band_spec.box_blur``, at the kernel's tile edges, at every radius 1 .. 32 (the LDS layout is a function of the
radius) with the tile-edge shapes on both sides of the switch of the tile height (r = 16 and r = 17), at radii larger than the
picture, at every alignment of the rows, and without a byte written outside the output."""
import numpy as np
import pytest

import panorama_band_spec as P

pytestmark = pytest.mark.gpu

RADII = (1, 2, 8, 32)
# k_box_blur's tile (csrc/apap_panorama.hip): kBlurCols = 64 columns; 32 rows up to r = 16, 16 rows above
TILE_COLS, TILE_ROWS_SMALL_R, TILE_ROWS_LARGE_R = 64, 32, 16
SHAPES = [(1, 1), (1, 300), (300, 1), (2, 2), (33, 65), (64, 64), (65, 257), (130, 67),
          (31, 63), (32, 64), (33, 129),        # a column and a row short of the tile, the tile, one more (r <= 16)
          (15, 127), (16, 128), (17, 65)]       # the same against the 16-row tile of r = 32


@pytest.fixture(scope="module")
def native_gpu(native):
    if native.lib().apap_device_count() < 1:
        pytest.skip("no HIP device")
    return native


def same(got, want, what):
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} bytes differ, first at (y, x, c) = {tuple(bad[0])}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_and_radii(native_gpu, hw):
    """Random bytes through the host-buffer form, and through the device form with the picture and the output at every
    alignment 0 .. 3 over the radii, the output pre-filled with 0xA5 between guard bytes."""
    import torch
    from cvx_proj_amd import resident
    assert (TILE_COLS, TILE_ROWS_SMALL_R, TILE_ROWS_LARGE_R) == (64, 32, 16)
    rng = np.random.default_rng(hw[0] * 1000 + hw[1])
    img = rng.integers(0, 256, hw + (3,), dtype=np.uint8)
    dev = torch.device("cuda", 0)
    nbytes = img.size
    for i, r in enumerate(RADII):
        want = P.box_blur(img, r)
        same(native_gpu.box_blur(img, r), want, f"{hw}, r = {r}, host buffers")
        shift_in, shift_out = i, (i + 1) % 4
        src = torch.zeros(nbytes + 8, dtype=torch.uint8, device=dev)
        d_img = src[shift_in:shift_in + nbytes].view(*img.shape)
        d_img.copy_(torch.from_numpy(img).to(dev))
        guard = 4096 + shift_out
        buf = torch.full((guard + nbytes + 4096,), 0x5C, dtype=torch.uint8, device=dev)
        out = buf[guard:guard + nbytes].view(*img.shape)
        out.fill_(0xA5)
        got = resident.hip_box_blur(d_img, r, out=out)
        torch.cuda.synchronize(dev)
        assert got.data_ptr() == out.data_ptr()
        same(got.cpu().numpy(), want, f"{hw}, r = {r}, device form, alignments {shift_in} and {shift_out}")
        assert bool((buf[:guard] == 0x5C).all()) and bool((buf[guard + nbytes:] == 0x5C).all()), "guard bytes around out"
        same(d_img.cpu().numpy(), img, "the picture is not modified")
    same(native_gpu.box_blur(img, 0), img, f"{hw}, r = 0")
    same(resident.hip_box_blur(torch.from_numpy(img).to(dev), 0).cpu().numpy(), img, f"{hw}, r = 0, device form")


ALL_RADII = tuple(range(1, 33))
EVERY_RADIUS_SHAPES = [(33, 65), (17, 129)]     # a tile row and a tile column more than one tile, under both tile heights
# the tile-edge shapes of SHAPES at the two radii between which the tile height switches
SWITCH_SHAPES = {16: EVERY_RADIUS_SHAPES + [(31, 63), (32, 64), (33, 129)], 17: EVERY_RADIUS_SHAPES + [(15, 127), (16, 128), (17, 65)]}

_pictures = {}


def random_picture(hw):
    """Seeded random bytes of a shape and, per radius asked for, the spec's blur; built once, read-only."""
    if hw not in _pictures:
        _pictures[hw] = (np.random.default_rng(hw[0] * 1000 + hw[1] + 7).integers(0, 256, hw + (3,), dtype=np.uint8), {})
    return _pictures[hw]


def blurred(hw, r):
    img, by_radius = random_picture(hw)
    if r not in by_radius:
        by_radius[r] = P.box_blur(img, r)
    return img, by_radius[r]


@pytest.mark.parametrize("r", ALL_RADII)
def test_every_radius(native_gpu, r):
    """Every LDS layout of the kernel (rows_in, the padded in_stride of an odd radius, the place of the row sums are functions of
    r): random bytes through the host-buffer form and the device form."""
    import torch
    from cvx_proj_amd import resident
    for hw in SWITCH_SHAPES.get(r, EVERY_RADIUS_SHAPES):
        img, want = blurred(hw, r)
        assert (want != img).any()
        same(native_gpu.box_blur(img, r), want, f"{hw}, r = {r}, host buffers")
        same(resident.hip_box_blur(torch.from_numpy(img).to("cuda:0"), r).cpu().numpy(), want, f"{hw}, r = {r}, device form")


@pytest.mark.parametrize("r", sorted(SWITCH_SHAPES))
def test_both_sides_of_the_tile_switch_into_guarded_outputs(native_gpu, r):
    """r = 16, the last radius of the 32-row tile, and r = 17, the first of the 16-row tile: the device form with the picture
    and the output at all four alignments each, the output pre-filled with 0xA5 between guard bytes of 0x5C."""
    import torch
    from cvx_proj_amd import resident
    assert (TILE_ROWS_SMALL_R, TILE_ROWS_LARGE_R) == (32, 16)
    dev = torch.device("cuda", 0)
    for hw in SWITCH_SHAPES[r]:
        img, want = blurred(hw, r)
        nbytes = img.size
        src = torch.zeros(nbytes + 8, dtype=torch.uint8, device=dev)
        buf = torch.empty(4096 + 4 + nbytes + 4096, dtype=torch.uint8, device=dev)
        for shift_in in range(4):
            d_img = src[shift_in:shift_in + nbytes].view(*img.shape)
            d_img.copy_(torch.from_numpy(img).to(dev))
            for shift_out in range(4):
                guard = 4096 + shift_out
                buf.fill_(0x5C)
                out = buf[guard:guard + nbytes].view(*img.shape)
                out.fill_(0xA5)
                got = resident.hip_box_blur(d_img, r, out=out)
                torch.cuda.synchronize(dev)
                assert got.data_ptr() == out.data_ptr() and out.data_ptr() % 4 == shift_out and d_img.data_ptr() % 4 == shift_in
                same(got.cpu().numpy(), want, f"{hw}, r = {r}, device form, alignments {shift_in} and {shift_out}")
                assert bool((buf[:guard] == 0x5C).all()) and bool((buf[guard + nbytes:] == 0x5C).all()), "guard bytes around out"
            same(d_img.cpu().numpy(), img, "the picture is not modified")


@pytest.mark.parametrize("r", sorted(SWITCH_SHAPES))
def test_all_255_at_the_tile_switch(native_gpu, r):
    """T = 255 n^2 everywhere under both tile heights: every byte stays 255."""
    img = np.full((40, 70, 3), 255, np.uint8)
    assert (P.box_blur(img, r) == 255).all()
    same(native_gpu.box_blur(img, r), img, f"40 x 70 of 255, r = {r}")


@pytest.mark.parametrize("hw", [(1, 1), (40, 70), (130, 67)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_all_255_at_the_largest_radius(native_gpu, hw):
    """T = 255 x 4225 everywhere, the largest sum and its rounding term: every byte stays 255."""
    img = np.full(hw + (3,), 255, np.uint8)
    got = native_gpu.box_blur(img, 32)
    assert (P.box_blur(img, 32) == 255).all()
    same(got, img, f"{hw} of 255, r = 32")


def test_768_at_radius_8(native_gpu):
    """12 x 24 tiles; the default radius of the blend."""
    import torch
    from cvx_proj_amd import resident
    img = np.random.default_rng(768).integers(0, 256, (768, 768, 3), dtype=np.uint8)
    want = P.box_blur(img, 8)
    same(native_gpu.box_blur(img, 8), want, "768 x 768, r = 8, host buffers")
    same(resident.hip_box_blur(torch.from_numpy(img).to("cuda:0"), 8).cpu().numpy(), want, "768 x 768, r = 8, device form")
    assert (want != img).any()


def test_bad_arguments(native_gpu):
    import torch
    from cvx_proj_amd import resident
    img = torch.ones((4, 5, 3), dtype=torch.uint8, device="cuda:0")
    for bad in (-1, 33, 1.5, True):
        with pytest.raises(ValueError, match="band"):
            resident.hip_box_blur(img, bad)
    with pytest.raises(ValueError, match="overlaps"):
        resident.hip_box_blur(img, 2, out=img)
    with pytest.raises(ValueError, match="out must be"):
        resident.hip_box_blur(img, 2, out=torch.ones((4, 5, 4), dtype=torch.uint8, device="cuda:0"))
