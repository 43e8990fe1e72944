"""Inputs of the OBJ tests (test_obj_ref.py, test_f64_display_host_cpu.py, test_mesh_obj_gpu.py, test_host_mesh_obj_cpp_gpu.py):
the value set of the f64 formatter, the whole-file scene (ply_scenes.scene() with the polygons of all three cameras), the
long-record surface and the five-polygon Texture file."""
import functools
import struct

import numpy as np

import mesh_scenes
import ply_scenes

VT_SIZES = (160, 200, 250, 280, 320, 1333)


def _from_bits(bits):
    return np.asarray(bits, dtype=np.uint64).view(np.float64)


@functools.lru_cache(maxsize=None)
def value_set(random_count=1_000_000):
    """-> float64 array: the specials, the worked examples, every power of two with both neighbours, c / 255, the vt forms
    x / w and 1 - y / h, `random_count` random bit patterns and 200 000 scaled coordinates."""
    nan_bits = [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000123, 0xFFF4000000000001, 0x7FFFFFFFFFFFFFFF]
    parts = [np.array([0.0, -0.0, np.inf, -np.inf]), _from_bits(nan_bits),
             np.array([1.0, 100.0, 0.1, 0.1 + 0.2, 1.0 / 3.0, 1e21, 1e22, 1e23, 1e-7, 123456789012345680000.0, 2.0 ** 53 - 1.0,
                       2.0 ** 53, 2.0 ** 53 + 2.0, 5e-324, 2.225073858507201e-308, 2.2250738585072014e-308, 1.7976931348623157e308,
                       -1.5, -1e23, -5e-324])]
    # 2^-1074 .. 2^1023 with both neighbours (bit patterns: the neighbours of a double are its bit pattern +- 1)
    powers = np.array([struct.unpack("<Q", struct.pack("<d", 2.0 ** e))[0] for e in range(-1074, 1024)], dtype=np.uint64)
    parts.append(_from_bits(np.concatenate([powers - np.uint64(1), powers, powers + np.uint64(1)])))
    parts.append(np.arange(256, dtype=np.float64) / 255.0)
    for size in VT_SIZES:
        t = np.arange(size, dtype=np.float64)
        parts += [t / float(size), 1.0 - t / float(size)]
    rng = np.random.default_rng(20250607)
    parts.append(_from_bits(rng.integers(0, 2 ** 64, random_count, dtype=np.uint64)))
    r, s = rng.random(200_000), rng.choice(np.array(ply_scenes.SCALE), 200_000)
    parts.append((r * 640.0 - 320.0) * s)
    return np.ascontiguousarray(np.concatenate(parts))


@functools.lru_cache(maxsize=None)
def scene():
    """-> (points, tracks, polygons [38 377, 3], camera [38 377], images): ply_scenes.scene()'s surface with the polygons of
    cameras 0, 1 and 2, concatenated."""
    points, tracks, _, images = ply_scenes.scene()
    s = mesh_scenes.scene(3)
    polys = [mesh_scenes.polygons(s, c) for c in range(3)]
    camera = np.concatenate([np.full(len(p), c, dtype=np.uint32) for c, p in enumerate(polys)])
    return points, tracks, np.ascontiguousarray(np.concatenate(polys).astype(np.uint32)), camera, images


@functools.lru_cache(maxsize=None)
def long_records():
    """600 tracks for Plain mode and out_scale (1, 1, 1): 0 .. 255 all subnormals with 17 digits (lines of ~985 bytes: the block
    is ~250 KB), 256 .. 511 alternating +-1.79e308-class values and 0, the rest ordinary; 10 polygons."""
    rng = np.random.default_rng(11)
    points = rng.uniform(-300.0, 300.0, (600, 3))
    sub = _from_bits(rng.integers(2 ** 51, 2 ** 52, (256, 3), dtype=np.uint64))            # subnormals in [2^-1023, 2^-1022)
    sub[::2] *= -1.0
    points[:256] = sub
    big = _from_bits(rng.integers(0x7FE0000000000000, 0x7FF0000000000000, (256, 3), dtype=np.uint64))
    big[1::2] = 0.0
    big[::4] *= -1.0
    points[256:512] = big
    tracks = np.zeros((600, 1, 2), dtype=np.int32)
    polygons = rng.integers(0, 600, (10, 3)).astype(np.uint32)
    return points, tracks, polygons, np.zeros(10, dtype=np.uint32)


def texture_five():
    """Five polygons with cameras 0, 2, 2, 1, 0 over six tracks of three images: track 1 has no point in image 2 (the camera of
    polygons 1 and 2, which name it), track 2's point in image 0 lies past the image (u > 1), track 4 has one point only.
    -> (points, tracks, dims, polygons, camera, the file's text with stem "five" and out_scale (1, 1, 1))"""
    points = np.array([[0.0, 0.0, 0.0], [1.0, 0.5, -2.0], [0.25, -1.0, 1e-7], [3.0, 0.1, 100.0], [-0.5, 1e21, 0.3], [7.0, 8.0, 9.0]])
    tracks = np.array([[[0, 0], [10, 5], [20, 40]],
                       [[16, 8], [5, 10], [-1, -1]],
                       [[48, 2], [-1, -1], [30, 60]],
                       [[-1, -1], [15, 15], [10, 20]],
                       [[-1, -1], [-1, -1], [39, 79]],
                       [[8, 4], [1, 1], [1, 1]]], dtype=np.int32)
    dims = [(32, 16), (20, 20), (40, 80)]
    polygons = np.array([[0, 1, 2], [1, 2, 3], [3, 4, 5], [5, 0, 1], [2, 0, 5]], dtype=np.uint32)
    camera = np.array([0, 2, 2, 1, 0], dtype=np.uint32)
    text = """mtllib five.mtl
v 0 -0 0
v 1 -0.5 -2
v 0.25 1 0.0000001
v 3 -0.1 100
v -0.5 -1000000000000000000000 0.3
v 7 -8 9
vt 0 1
vt 0.5 0.75
vt 0.5 0.5
vt 0.5 0.5
vt 0.25 0.5
vt 1.5 0.875
vt 0.75 0.25
vt 0.75 0.25
vt 0.25 0.75
vt 0.975 0.012499999999999956
vt 0.25 0.75
vt 0.05 0.95
vt 0.025 0.9875
usemtl Textured0
f 3/6 2/4 1/1
usemtl Textured2
f 4/9 3/7 2/6
f 6/13 5/10 4/9
usemtl Textured1
f 2/5 1/2 6/12
usemtl Textured0
f 6/11 1/1 3/6
"""
    return points, tracks, dims, polygons, camera, text.encode("ascii")
