"""The one image-sequence check of cvx_proj_amd.resident behind hip_sift_describe_batch and hip_corner_detect_batch: both
refuse the same bad image lists, in the same words but for their own names, before anything is launched."""
import pytest

pytestmark = pytest.mark.gpu

SIFT, CORNER = "hip_sift_describe_batch", "hip_corner_detect_batch"


@pytest.fixture(scope="module")
def dev(native):
    if native.lib().apap_device_count() < 1:
        pytest.skip("no HIP device")
    import torch
    return torch.device("cuda", 0)


def bad_images(torch, dev):
    return {"int32": (torch.zeros((8, 8), dtype=torch.int32, device=dev), "imgs[1] must be a contiguous uint8 (h, w) or (h, w, 3) tensor on cuda:0"),
            "not contiguous": (torch.zeros((16, 16), dtype=torch.uint8, device=dev)[:, ::2],
                               "imgs[1] must be a contiguous uint8 (h, w) or (h, w, 3) tensor on cuda:0"),
            "6 x 40": (torch.zeros((6, 40), dtype=torch.uint8, device=dev), "imgs[1]: sides must be 7 .. 32768; got (6, 40)")}


@pytest.mark.parametrize("which", ["int32", "not contiguous", "6 x 40"])
def test_both_refuse_a_bad_image_in_the_same_words(native, dev, which):
    import torch
    from cvx_proj_amd import resident
    bad, text = bad_images(torch, dev)[which]
    assert which != "not contiguous" or (tuple(bad.shape) == (16, 8) and not bad.is_contiguous())
    imgs = [torch.zeros((9, 12, 3), dtype=torch.uint8, device=dev), bad]
    pts = torch.ones((2, 2), dtype=torch.float32, device=dev)
    with pytest.raises(ValueError) as e:
        resident.hip_sift_describe_batch(imgs, pts, [1, 1])
    assert str(e.value) == f"{SIFT}: {text}"
    with pytest.raises(ValueError) as f:
        resident.hip_corner_detect_batch(imgs, 10)
    assert str(f.value) == f"{CORNER}: {text}"
    assert str(e.value).replace(SIFT, "") == str(f.value).replace(CORNER, "")
