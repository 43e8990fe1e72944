"""The library reads what it writes: mesh.tiff (cvhip_tiff_encode) of a device tensor, decoded by
image.decode_tiff (cvhip_tiff_decode) into device memory, gives the pixels back - Luma8 of 1 channel, RGB8 of 3
channels, RGB8 of 4 channels with the alpha dropped.  A file of 2 channels is read by Pillow alone: cvhip_tiff_decode refuses 2
samples, and keeps doing so."""
import io

import numpy as np
import pytest

import tiff_out_scenes as S
from cybervision_amd import _lib, image, mesh
from cybervision_amd.mesh import TiffCompression  # (without the encoder every test here fails at this import)

pytestmark = pytest.mark.gpu
NAMES = ["pred_g8", "pred_rgb8", "pred_rgba8", "short_last_strip_lzw", "lzw_noise_8192_one_strip", "lzw_strip_64k", "pb_seams", "pb_rgb",
         "pb_rgba_sparse", "two_strips_raw_rgb", "strips_257_lzw", "lzw_1x1",
         # the encoder's staging and launch seams (tests/test_tiff_out_ref.py: test_scene_seams)
         "lzw_flat_640k", "lzw_dense_4096", "lzw_clear_at_1023", "strips_lzw_second_trip", "pb_rows_second_trip", "widest_rgba_lzw_pred"]


@pytest.mark.parametrize("name", NAMES)
def test_decode_of_encode_is_the_pixels(gpu_device, name):
    import torch

    pixels, compression, predictor, rps = S.scene(name)
    d_pixels = torch.from_numpy(np.array(pixels)).cuda()
    file = mesh.tiff(gpu_device, d_pixels, TiffCompression(compression), predictor, rps)
    c = pixels.shape[2]
    got = image.decode_tiff(gpu_device, file, "L" if c == 1 else "RGB", 0, out="device")
    torch.cuda.synchronize()
    assert got.is_cuda
    want = pixels[:, :, 0] if c == 1 else pixels[:, :, :3]
    assert got.shape == want.shape and (got.cpu().numpy() == want).all()


def test_two_channels_are_pillows_alone(gpu_device):
    from PIL import Image

    pixels, compression, predictor, rps = S.scene("pred_ga8")
    file = mesh.tiff(gpu_device, pixels, compression, predictor, rps).tobytes()
    img = Image.open(io.BytesIO(file))
    assert img.mode == "LA" and (np.asarray(img) == pixels).all()
    with pytest.raises(_lib.CvhipError) as e:
        image.decode_tiff(gpu_device, file, "L", 0)
    assert e.value.code == -3
