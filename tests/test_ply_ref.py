"""The restatement of the mesh output (tests/ref_ply.py) against hand-written bytes and against its own scalar
transcription: the PLY file image of PlyWriter (src/output.rs:648-772) and ImageWriter::complete's colour mapping
(:1117-1229).  No GPU."""
import math

import numpy as np
import pytest

import ref_ply

TABLE = ref_ply.generated_table()


def test_generated_table_is_not_monotone():
    assert TABLE.shape == (256, 3) and TABLE.dtype == np.uint8
    assert TABLE[0].tolist() == [11, 7, 0] and TABLE[1].tolist() == [48, 108, 201] and TABLE[255].tolist() == [230, 162, 55]
    for k in range(3):
        d = np.diff(TABLE[:, k].astype(int))
        assert (d > 0).any() and (d < 0).any() and len(set(TABLE[:, k].tolist())) > 100


def test_hand_written_file():
    """Two vertices and one face in Color mode, out_scale (2, 1, -1).  Track 0 has no point in image 0; its point in image 1
    is pixel (x 1, y 0) = (10, 20, 30).  Track 1's first point (x 2, y 1) lies past the 2-pixel-wide image 0: no colour
    bytes - its valid point in image 1 is not consulted.  Vertex 0 has y = 0: -0.0 * 1 is 80 00 ..."""
    points = np.array([[1.0, 0.0, 2.0], [-0.5, 2.0, 0.25]])
    tracks = np.array([[[-1, -1], [1, 0]], [[2, 1], [0, 0]]], dtype=np.int32)
    image0 = np.full((2, 2, 3), 200, dtype=np.uint8)
    image1 = np.array([[[1, 2, 3], [10, 20, 30]]], dtype=np.uint8)  # 1 row, 2 columns
    polygons = np.array([[0, 1, 0x01020304]], dtype=np.uint32)
    want = (b"ply\n"
            b"format binary_big_endian 1.0\n"
            b"comment Cybervision 3D surface\n"
            b"element vertex 2\n"
            b"property double x\n"
            b"property double y\n"
            b"property double z\n"
            b"property uchar red\n"
            b"property uchar green\n"
            b"property uchar blue\n"
            b"element face 1\n"
            b"property list uchar int vertex_indices\n"
            b"end_header\n"
            + bytes([0x40, 0, 0, 0, 0, 0, 0, 0,          # 1.0 * 2 = 2.0
                     0x80, 0, 0, 0, 0, 0, 0, 0,          # (-0.0) * 1 = -0.0
                     0xC0, 0, 0, 0, 0, 0, 0, 0,          # 2.0 * -1 = -2.0
                     10, 20, 30,
                     0xBF, 0xF0, 0, 0, 0, 0, 0, 0,       # -0.5 * 2 = -1.0
                     0xC0, 0, 0, 0, 0, 0, 0, 0,          # (-2.0) * 1 = -2.0
                     0xBF, 0xD0, 0, 0, 0, 0, 0, 0,       # 0.25 * -1 = -0.25: 24 bytes, no colour
                     3, 1, 2, 3, 4, 0, 0, 0, 1, 0, 0, 0, 0]))   # vertices[2], [1], [0]
    assert len(want) == 198 + 60 + 1 + 1 + 27 + 24 + 13
    for fn in (ref_ply.ply_bytes, ref_ply.ply_bytes_scalar):
        assert fn(points, tracks, [image0, image1], ref_ply.COLOR, (2.0, 1.0, -1.0), polygons) == want
    # Plain and Texture: no colour lines, no colour bytes
    plain = ref_ply.ply_bytes(points, tracks, None, ref_ply.PLAIN, (2.0, 1.0, -1.0), polygons)
    assert plain == ref_ply.ply_bytes(points, tracks, None, ref_ply.TEXTURE, (2.0, 1.0, -1.0), polygons)
    body = 260  # the Color header: 198 + 60 + 1 + 1
    assert plain == want[:want.index(b"property uchar red")] + want[want.index(b"element face"):body + 24] + want[body + 27:]


def test_header_length_formula():
    for n, n_poly in [(0, 0), (1, 1), (12, 5), (255, 9), (257, 10), (256, 300), (4194304, 8382466), (4294967294, 4294967294)]:
        for mode in (ref_ply.PLAIN, ref_ply.COLOR, ref_ply.TEXTURE):
            assert len(ref_ply.header(n, n_poly, mode)) == ref_ply.header_length(n, n_poly, mode)
    assert [ref_ply.header_length(n, p, ref_ply.PLAIN) % 4 for n, p in [(1, 1), (12, 5), (255, 9), (257, 10), (256, 300)]] == [0, 1, 2, 3, 0]
    assert ref_ply.parse_header(ref_ply.header(12, 5, ref_ply.COLOR) + b"xyz") == (261, 12, 5, True)


def random_surface(n, m, seed):
    rng = np.random.default_rng(seed)
    points = rng.normal(0.0, 3.0, (n, 3))
    points[rng.random(n) < 0.05, 1] = 0.0
    points[0] = [np.nan, np.inf, -0.0]
    tracks = rng.integers(0, 40, (n, m, 2)).astype(np.int32)
    tracks[rng.random((n, m)) < 0.4] = -1
    tracks[np.arange(n), rng.integers(0, m, n)] = rng.integers(0, 40, (n, 2))  # every track has a point
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in [(40, 30), (25, 40), (33, 35)][:m]]
    polygons = rng.integers(0, n, (2 * n, 3)).astype(np.uint32)
    return points, tracks, images, polygons


def test_vectorised_equals_scalar_on_random_tracks():
    points, tracks, images, polygons = random_surface(300, 3, 5)
    scale = (1.5, -2.0, 0.75)
    for mode in (ref_ply.PLAIN, ref_ply.COLOR, ref_ply.TEXTURE):
        a = ref_ply.ply_bytes(points, tracks, images, mode, scale, polygons)
        assert a == ref_ply.ply_bytes_scalar(points, tracks, images, mode, scale, polygons)
        end, n, n_poly, coloured = ref_ply.parse_header(a)
        assert (n, n_poly, coloured) == (300, 600, mode == ref_ply.COLOR)
    has, _ = ref_ply.vertex_colours(tracks, images)
    first, _ = ref_ply.first_points(tracks)
    assert 0 < has.sum() < 300 and (first > 0).any()
    assert len(a) == ref_ply.header_length(300, 600, ref_ply.PLAIN) + 24 * 300 + 13 * 600
    # a track without a point: the reference's error in Color mode only
    tracks[7] = -1
    for fn in (ref_ply.ply_bytes, ref_ply.ply_bytes_scalar):
        with pytest.raises(ref_ply.TrackHasNoImages):
            fn(points, tracks, images, ref_ply.COLOR, scale, polygons)
        assert fn(points, tracks, images, ref_ply.PLAIN, scale, polygons) == a


def test_colour_map_by_hand():
    """min 0, max 255, so that value = depth / 255 and step = 1 / 255."""
    below_one = math.nextafter(1.0, 0.0)
    cells = np.array([[0.0,            # value 0: table[0]
                       3.0,            # a box boundary (value / step is 3 or just below: table[3] either way)
                       0.5,            # value = step / 2 exactly: ratio 0.5, (c1 + c2) / 2 ends in .5 in every channel
                       255.0,          # value = 1: table[255]
                       300.0,          # value > 1
                       np.nan]])       # None
    want = [[11, 7, 0, 255],
            [122, 54, 91, 255],
            [30, 58, 101, 255],        # 29.5, 57.5, 100.5: half away from zero (half to even would give 100)
            [230, 162, 55, 255],
            [230, 162, 55, 255],
            [0, 0, 0, 0]]
    for fn in (ref_ply.colour_map, ref_ply.colour_map_scalar):
        assert fn(cells, 0.0, 255.0, TABLE)[0].tolist() == want
    # the constant map: value is NaN, every comparison false, box 0, ratio NaN -> (0, 0, 0, 255); None stays (0, 0, 0, 0)
    flat = np.array([[4.25, np.nan, 4.25]])
    for fn in (ref_ply.colour_map, ref_ply.colour_map_scalar):
        assert fn(flat, 4.25, 4.25, TABLE)[0].tolist() == [[0, 0, 0, 255], [0, 0, 0, 0], [0, 0, 0, 255]]
    # the largest double below 1.0: not the `>= 1` branch; box 254 (floor gives 254 or 255, the clamp 254), ratio just below 1
    step = 1.0 / 255.0
    box = min(int(math.floor(below_one / step)), 254)
    ratio = (below_one - step * float(box)) / step
    assert below_one < 1.0 and box == 254 and 1.0 - 1e-9 < ratio < 1.0
    for fn in (ref_ply.colour_map, ref_ply.colour_map_scalar):
        assert fn(np.array([[below_one]]), 0.0, 1.0, TABLE)[0, 0].tolist() == [230, 162, 55, 255]
    # an index off by one or c1 / c2 swapped changes bytes: a cell a quarter into box 7
    v = ref_ply.colour_map(np.array([[7.25]]), 0.0, 255.0, TABLE)[0, 0].tolist()
    c1, c2 = TABLE[7].astype(float), TABLE[8].astype(float)
    assert v[:3] == [int(math.floor(x + 0.5)) for x in 0.75 * c1 + 0.25 * c2] and v[:3] != [int(math.floor(x + 0.5)) for x in 0.25 * c1 + 0.75 * c2]


def test_colour_map_vectorised_equals_scalar():
    rng = np.random.default_rng(11)
    depth = rng.uniform(-3.0, 9.0, (23, 37))
    depth[rng.random(depth.shape) < 0.2] = np.nan
    lo, hi = float(np.nanmin(depth)), float(np.nanmax(depth))
    a = ref_ply.colour_map(depth, lo, hi, TABLE)
    assert a.tobytes() == ref_ply.colour_map_scalar(depth, lo, hi, TABLE).tobytes()
    assert a.shape == (23, 37, 4) and (a[np.isnan(depth)] == 0).all() and (a[~np.isnan(depth), 3] == 255).all()
    # a range narrower than the data: values below 0 and above 1
    b = ref_ply.colour_map(depth, 0.0, 5.0, TABLE)
    assert b.tobytes() == ref_ply.colour_map_scalar(depth, 0.0, 5.0, TABLE).tobytes()
