"""What the feature front end defines once and uses in several places, as far as a machine without a GPU can tell: the two
numpy restatements of the grey conversion (tests/corner_spec.py for the detector, tests/sift_spec.py for the descriptor; the
kernels share apap::grey_at of csrc/apap_image_dev.h) and the binding's one offsets rule behind ``match_offsets`` and
``sift_offsets``."""
import numpy as np
import pytest

import corner_spec
import sift_spec


@pytest.mark.parametrize("img", [np.random.default_rng(911).integers(0, 256, (9, 11, 3)).astype(np.uint8),
                                 np.zeros((9, 11, 3), np.uint8), np.full((9, 11, 3), 255, np.uint8)], ids=["seeded", "all 0", "all 255"])
def test_the_two_specifications_have_one_grey(img):
    a, b = corner_spec.grey(img), sift_spec.grey(img)
    assert a.shape == b.shape == (9, 11) and np.array_equal(a, b)
    if img.min() == img.max():       # the weights sum to 2^15: a flat picture keeps its value
        assert np.all(b == img[0, 0, 0])
    else:
        assert len(np.unique(b)) > 50
    for plane in (img[:, :, 0], img[:, :, :1]):      # grey as it is, in both
        assert np.array_equal(corner_spec.grey(plane), plane.reshape(9, 11)) and np.array_equal(sift_spec.grey(plane), plane.reshape(9, 11))


def test_match_and_sift_offsets_are_one_rule(native):
    a, b = native.match_offsets([1, 3, 2], "q_lengths"), native.sift_offsets([1, 3, 2])
    assert a.dtype == b.dtype == np.int32 and a.tolist() == b.tolist() == [0, 1, 4, 6]
    assert native.MATCH_MAX_ROWS == native.SIFT_MAX_KEYPOINTS == 2 ** 24 and native.MATCH_MAX_PAIRS == native.SIFT_MAX_IMAGES == 65535


class Lengths:
    """128 counts of 2^24, whose sum is 2^31, without 2^31 of anything."""

    def __len__(self):
        return 128

    def __iter__(self):
        return iter([2 ** 24] * 128)


@pytest.mark.parametrize("lengths, match_text, sift_text", [
    ([], "0 pairs (1 .. 65535)", "0 images (1 .. 65535)"),
    ([2, 0], "a pair holds 1 .. 2^24 rows; got [2, 0]", "an image holds 1 .. 2^24 keypoints; got [2, 0]"),
    ([2 ** 24 + 1], "a pair holds 1 .. 2^24 rows; got [16777217]", "an image holds 1 .. 2^24 keypoints; got [16777217]"),
    (Lengths(), "2147483648 rows in all exceed the int32 offsets", "2147483648 keypoints in all exceed the int32 offsets"),
], ids=["none", "a zero", "2^24 + 1", "2^31 in all"])
def test_offsets_refuse_with_their_own_nouns(native, lengths, match_text, sift_text):
    with pytest.raises(ValueError) as e:
        native.match_offsets(lengths, "t_lengths")
    assert str(e.value) == "t_lengths: " + match_text
    with pytest.raises(ValueError) as e:
        native.sift_offsets(lengths)
    assert str(e.value) == "lengths: " + sift_text
    with pytest.raises(ValueError) as e:
        native.sift_offsets(lengths, "counts")
    assert str(e.value) == "counts: " + sift_text
