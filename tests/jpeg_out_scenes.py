"""The images the JPEG encoder's tests encode (tests/ref_jpeg_out.py is the definition of the file): name -> (pixels, quality,
sampling, optimize).  Every image is the smallest at which one part of the encoder can break; test_jpeg_out_ref.py asserts,
on the restatement alone, that each scene does reach the case it is here for, and that the restated file is Pillow's.  Two
scenes too slow to restate in every run stand beside scenes(): BIG."""
from __future__ import annotations

import functools

import numpy as np

import ref_jpeg_out
from ref_jpeg_out import S420, S422, S444

# found by a search over seeds on the CPU (test_jpeg_out_ref.py asserts what each is here for)
SEED_COEF63, SEED_ADJACENT_FF, SEED_LAST_FF, SEED_TILE_FF = 31, 111, 27, 25


def noise(seed: int, h: int, w: int, c: int = 0):
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, size=(h, w, c) if c else (h, w)).astype(np.uint8)


def binary(seed: int, h: int, w: int):
    """noise of 0 and 255 only: the largest coefficients that noise gives"""
    return (np.random.RandomState(seed).randint(0, 2, size=(h, w)) * 255).astype(np.uint8)


def smooth(seed: int, h: int, w: int, c: int = 0):
    """a smooth surface with two bits of noise"""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = (128 + 100 * np.sin(x / 23.0 + seed) * np.cos(y / 31.0)).astype(np.int64)
    if c:
        base = base[:, :, None] + 29 * np.arange(c)[None, None, :] * (1 + x[:, :, None] % 3)
    return ((base + rng.randint(0, 4, size=base.shape)) & 0xFF).astype(np.uint8)


def dc_swing():
    """8 wide, 64 high: flat blocks of 0 and of 255 in turn"""
    img = np.zeros((64, 8), dtype=np.uint8)
    for k in range(1, 8, 2):
        img[8 * k:8 * k + 8] = 255
    return img


def with_alpha(pixels, seed: int):
    """the image with a channel of noise behind its own: the alpha that the encoder drops"""
    px = pixels if pixels.ndim == 3 else pixels[:, :, None]
    return np.concatenate([px, noise(seed, *px.shape[:2], 1)], axis=2)


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> (pixels, quality, sampling, optimize); sizes in the names are width x height"""
    s = {
        "grey_1x1": (np.array([[77]], dtype=np.uint8), 75, S444, False),
        "rgb_1x1_444": (np.array([[[200, 30, 90]]], dtype=np.uint8), 75, S444, False),
        "rgb_1x1_422": (np.array([[[200, 30, 90]]], dtype=np.uint8), 75, S422, False),
        "rgb_1x1_420": (np.array([[[200, 30, 90]]], dtype=np.uint8), 75, S420, False),
        "rgb_8x8_420": (noise(1, 8, 8, 3), 90, S420, False),
        "rgb_8x24_420": (noise(2, 24, 8, 3), 90, S420, False),
        "rgb_24x8_420": (noise(3, 8, 24, 3), 90, S420, False),
        "rgb_9x17_420": (noise(4, 17, 9, 3), 90, S420, False),
        "rgb_17x33_420": (noise(5, 33, 17, 3), 75, S420, True),
        "rgb_9x9_422": (noise(6, 9, 9, 3), 90, S422, False),
        "rgb_17x9_444": (noise(7, 9, 17, 3), 90, S444, True),
        "noise_16x16_q100": (binary(SEED_COEF63, 16, 16), 100, S444, False),
        "dc_swing_8x64_q100": (dc_swing(), 100, S444, False),
        "noise_32x32_q1": (noise(8, 32, 32), 1, S444, False),
        "flat_64x64": (np.full((64, 64, 3), 90, dtype=np.uint8), 75, S420, False),
        "flat_64x64_optimize": (np.full((64, 64, 3), 128, dtype=np.uint8), 75, S420, True),  # every coefficient is zero
        "adjacent_ff": (binary(SEED_ADJACENT_FF, 16, 16), 100, S444, False),
        "last_byte_ff": (noise(SEED_LAST_FF, 16, 16), 90, S444, False),
        "tile_end_ff": (noise(SEED_TILE_FF, 48, 48), 100, S444, False),
        "grey_strip_8x40000": (smooth(9, 40000, 8), 75, S444, False),
        "rgb_2048x24_420": (smooth(10, 24, 2048, 3), 90, S420, True),
        "smooth_rgb_70x50_422_optimize": (smooth(11, 50, 70, 3), 85, S422, True),
    }
    for q in (1, 49, 50, 51, 100):
        s["quality_%d" % q] = (smooth(12, 13, 19, 3), q, S420, False)
    # past one launch of the transform's workgroups (32 blocks each): a ragged last group in the second trip, a dummy column
    # in every MCU row and a dummy row at the bottom, so dummies in both trips; 65496 is the largest multiple of 8 that libjpeg takes
    s["rgb_24x65496_420_optimize"] = (smooth(21, 65496, 24, 3), 75, S420, True)
    # the largest width and height: SOF0's size bytes FF FF, the edge clamps at the last row and column, 8192 blocks in a line
    s["grey_65535x8"] = (smooth(23, 8, 65535), 75, S444, False)
    s["grey_8x65535"] = (smooth(23, 65535, 8), 75, S444, False)
    s["grey_alpha_copy"] = (with_alpha(s["last_byte_ff"][0], 13), 90, S444, False)
    s["rgba_copy"] = (with_alpha(s["rgb_9x17_420"][0], 14), 90, S420, False)
    return s


# the scenes beyond libjpeg's 65500: Pillow refuses them (test_jpeg_out_ref.py asserts that it does), so no file of Pillow's
# stands behind the restatement there
OVERSIZE = ("grey_65535x8", "grey_8x65535")

# Past one launch of a lane a block (mesh.GRID_LANES).  Not in scenes(): the restatement of a quarter of a million blocks takes
# a quarter of a minute, so the device's file is compared with Pillow's (test_jpeg_out_gpu.py) and one CPU test pins the
# restatement to Pillow on the first.
#   grey_4104x4096_optimize  262656 blocks and 3.2 MB of unstuffed stream, past three launches of the stuffing tiles too
#   rgb_3352x3352_420        264600 blocks with a dummy column in every MCU row and a dummy row: dummies in the second trip
BIG = ("grey_4104x4096_optimize", "rgb_3352x3352_420")


def big_scene(name):
    """(pixels, quality, sampling, optimize) of a scene of BIG; the grey one is the smooth surface with noise of 0 .. 11 on it"""
    if name == "grey_4104x4096_optimize":
        pixels = smooth(22, 4096, 4104).astype(np.int64) + np.random.RandomState(22).randint(0, 12, size=(4096, 4104))
        return (pixels & 0xFF).astype(np.uint8), 90, S444, True
    assert name == "rgb_3352x3352_420"
    return smooth(24, 3352, 3352, 3), 75, S420, False


# the scene whose file a 2- or 4-channel scene must give: that of its grey or RGB part
ALPHA_COPIES = {"grey_alpha_copy": "last_byte_ff", "rgba_copy": "rgb_9x17_420"}


def opaque(pixels):
    """what Pillow can take of a scene's pixels: [h, w] or [h, w, 3]"""
    if pixels.ndim == 2:
        return pixels
    return pixels[:, :, 0] if pixels.shape[2] <= 2 else pixels[:, :, :3]


@functools.lru_cache(maxsize=None)
def restated(name):
    """ref_jpeg_out.encode of a scene, computed once"""
    pixels, quality, sampling, optimize = scenes()[name]
    return ref_jpeg_out.encode(pixels, quality, sampling, optimize)
