"""The library reads what it writes: mesh.png (cvhip_png_encode) of 1- to 4-channel pictures under every
filter setting, decoded by image.decode_png (cvhip_png_decode), returns the input's grey / RGB exactly -
alpha dropped, and from device memory to device memory."""
import numpy as np
import pytest

from cybervision_amd import image, mesh

pytestmark = pytest.mark.gpu


def _picture(h, w, c):
    rng = np.random.default_rng([7, h, w, c])
    y, x = np.mgrid[0:h, 0:w]
    base = ((x * 3 + y * 5) % 251)[:, :, None] + np.arange(c) * 40
    return ((base + rng.integers(0, 4, (h, w, c))) % 256).astype(np.uint8)


@pytest.mark.parametrize("shape", [(1, 1), (9, 17), (160, 160)])
@pytest.mark.parametrize("channels", [1, 2, 3, 4])
def test_decode_of_encode_is_the_picture(gpu_device, shape, channels):
    import torch

    pixels = _picture(*shape, channels)
    grey_in = channels <= 2
    want_rgb = np.repeat(pixels[:, :, :1], 3, axis=2) if grey_in else pixels[:, :, :3]
    r, g, b = (want_rgb[:, :, k].astype(np.int64) for k in range(3))
    want_luma = pixels[:, :, 0] if grey_in else ((2126 * r + 7152 * g + 722 * b) // 10000).astype(np.uint8)
    for filt in mesh.PngFilter:
        file = mesh.png(gpu_device, pixels[:, :, 0] if channels == 1 else pixels, filt)
        assert (image.decode_png(gpu_device, file, "RGB") == want_rgb).all(), filt
        assert (image.decode_png(gpu_device, file, "L") == want_luma).all(), filt
    # device memory to device memory
    d_pixels = torch.from_numpy(np.ascontiguousarray(pixels[:, :, 0] if channels == 1 else pixels)).cuda()
    file = mesh.png(gpu_device, d_pixels, mesh.PngFilter.Adaptive)
    d_rgb = image.decode_png(gpu_device, file, "RGB", out="device")
    assert d_rgb.is_cuda and (d_rgb.cpu().numpy() == want_rgb).all()
