"""The library reads what it writes: mesh.jpeg (cvhip_jpeg_encode) of grey and RGB pictures at each sampling,
decoded by image.decode_jpeg (cvhip_jpeg_decode), gives the pixels that tests/ref_jpeg.py, the decoder's
definition, gives for the same file - as RGB8 and as Luma8."""
import numpy as np
import pytest

import ref_jpeg
from cybervision_amd import image, mesh
from cybervision_amd.mesh import JpegSampling  # (without the encoder every test here fails at this import)

pytestmark = pytest.mark.gpu


def _picture(h, w, c):
    rng = np.random.default_rng([11, h, w, c])
    y, x = np.mgrid[0:h, 0:w]
    base = ((x * 3 + y * 5) % 251)[:, :, None] + np.arange(c) * 40
    return ((base + rng.integers(0, 4, (h, w, c))) % 256).astype(np.uint8)


@pytest.mark.parametrize("shape", [(1, 1), (9, 17), (50, 70)])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("sampling", list(JpegSampling))
def test_decode_of_encode_is_the_restated_decode(gpu_device, shape, channels, sampling):
    pixels = _picture(*shape, channels)
    file = mesh.jpeg(gpu_device, pixels[:, :, 0] if channels == 1 else pixels, 85, sampling, optimize=shape == (9, 17)).tobytes()
    want_rgb, want_luma = ref_jpeg.decode(file, ref_jpeg.RGB8), ref_jpeg.decode(file, ref_jpeg.LUMA8)
    assert want_rgb.shape == (*shape, 3) and want_luma.shape == shape
    assert (image.decode_jpeg(gpu_device, file, "RGB") == want_rgb).all()
    assert (image.decode_jpeg(gpu_device, file, "L") == want_luma).all()
