"""The mesh output on the device (cvhip_mesh_ply, cvhip_mesh_colour_map, csrc/mesh_output_kernels.hip)
against the numpy restatement (tests/ref_ply.py).  Every comparison is tobytes() equality, with no tolerance: every
operation is a single IEEE f64 operation or a byte move.

The surface is tests/ply_scenes.py's: mesh_scenes.scene(3) - 12 288 tracks, camera 0's polygons - with random RGB images
from a fixed seed that are narrower than the scene's 320^2, so that every one of the 48 blocks of 256 tracks holds 24-byte
and 27-byte records."""
import ctypes as C

import numpy as np
import pytest

import mesh_scenes
import ref_ply
from cybervision_amd import _lib, mesh, reconstruction, synth
from ply_scenes import SCALE, random_images, scene, surface_of

pytestmark = pytest.mark.gpu
TABLE = ref_ply.generated_table()
Plain, Color, Texture = mesh.VertexMode.Plain, mesh.VertexMode.Color, mesh.VertexMode.Texture


def same(got, want):
    got = np.asarray(got, dtype=np.uint8).tobytes()
    if got != want:
        k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        pytest.fail(f"file images differ: {len(got)} against {len(want)} bytes, first difference at byte {k}")
    return True


def test_whole_file_three_modes(gpu_device):
    points, tracks, polys, images = scene()
    sf = surface_of(points, tracks)
    first, _ = ref_ply.first_points(tracks)
    has, _ = ref_ply.vertex_colours(tracks, images)
    assert len(points) == 12288 and (first > 0).sum() > 1000                     # first points outside image 0 occur
    blocks = has.reshape(48, 256)
    assert blocks.any(axis=1).all() and (~blocks).any(axis=1).all()              # 24- and 27-byte records in every block
    for mode in (Plain, Color, Texture):
        sections = []
        got = mesh.ply(gpu_device, sf, polys, images if mode == Color else None, mode, SCALE, sections=sections)
        want = ref_ply.ply_bytes(points, tracks, images, int(mode), SCALE, polys)
        assert same(got, want)
        assert sections == [ref_ply.header_length(len(points), len(polys), int(mode)),
                            24 * len(points) + (3 * int(has.sum()) if mode == Color else 0), 13 * len(polys)]
    # images that are given but not needed are not read
    assert same(mesh.ply(gpu_device, sf, polys, images, Plain, SCALE), ref_ply.ply_bytes(points, tracks, None, ref_ply.PLAIN, SCALE, polys))


SUBS = [(1, 1), (12, 5), (255, 9), (257, 10), (256, 300), (0, 0)]


def test_block_and_alignment_edges(gpu_device):
    """Sub-surfaces whose header lengths put the body at every residue mod 4 (the same in Color mode: + 60), at one track
    short of, at and one past a block of 256; the header alone; images that hold every first point, and none."""
    points, tracks, polys, images = scene()
    residues = set()
    for n, n_poly in SUBS:
        sub_p, sub_t = points[:n], tracks[:n]
        sub_poly = (polys[:n_poly] % max(n, 1)).astype(np.uint32)
        sf = surface_of(sub_p, sub_t)
        residues.add(ref_ply.header_length(n, n_poly, ref_ply.PLAIN) % 4)
        for mode in (Plain, Color):
            got = mesh.ply(gpu_device, sf, sub_poly, images if mode == Color else None, mode, SCALE)
            assert same(got, ref_ply.ply_bytes(sub_p, sub_t, images, int(mode), SCALE, sub_poly)), (n, n_poly, mode)
        if n == 0:
            assert got.tobytes() == ref_ply.header(0, 0, ref_ply.COLOR)
    assert residues == {0, 1, 2, 3}
    assert [ref_ply.header_length(n, p, ref_ply.PLAIN) % 4 for n, p in SUBS[:5]] == [0, 1, 2, 3, 0]
    sf = surface_of(points, tracks)
    for dims, count in (([(320, 320)] * 3, len(points)), ([(0, 5)] * 3, 0)):
        imgs = random_images(dims, seed=3)
        assert int(ref_ply.vertex_colours(tracks, imgs)[0].sum()) == count
        sections = []
        got = mesh.ply(gpu_device, sf, polys[:700], imgs, Color, SCALE, sections=sections)
        assert same(got, ref_ply.ply_bytes(points, tracks, imgs, ref_ply.COLOR, SCALE, polys[:700]))
        assert sections[1] == 24 * len(points) + 3 * count


def test_more_than_one_launch(gpu_device):
    """Tracks and polygons tiled past mesh.GRID_LANES: the grid-stride loops of the three kernels take a second trip, in
    Color mode with mixed record lengths."""
    points, tracks, polys, images = scene()
    n = mesh.GRID_LANES + 300
    reps = n // len(points) + 1
    big_p, big_t = np.tile(points, (reps, 1))[:n], np.tile(tracks, (reps, 1, 1))[:n]
    big_poly = np.tile(polys, (n // len(polys) + 1, 1))[:n]
    # more blocks than one launch has (GRID_LANES / 256), for the vertices and the faces
    assert (n + 255) // 256 > mesh.GRID_LANES // 256 and len(big_poly) == n
    got = mesh.ply(gpu_device, surface_of(big_p, big_t), big_poly, images, Color, SCALE)
    want = ref_ply.ply_bytes(big_p, big_t, images, ref_ply.COLOR, SCALE, big_poly)
    assert len(want) > 24 * n + 13 * n and same(got, want)


def raw_ply(gpu_device, points, tracks, polys, images, mode, out, cap):
    """cvhip_mesh_ply itself -> (rc, size, sections); out: a C pointer or None"""
    n = len(points)
    m = tracks.shape[1]
    img_args, keep = mesh._image_args(images) if images is not None else ([None, None, None], None)
    scale = np.array(SCALE)
    size, sec = C.c_uint64(0), np.zeros(3, dtype=np.uint64)
    rc = _lib.lib().cvhip_mesh_ply(gpu_device.handle, mesh._p(points), mesh._p(tracks), n, m, *img_args, int(mode), mesh._p(scale),
                                   mesh._p(polys), len(polys), out, cap, C.byref(size), mesh._p(sec))
    return rc, size.value, [int(v) for v in sec]


def test_sizing_errors_pointers(gpu_device):
    import torch

    points, tracks, polys, images = scene()
    polys = np.ascontiguousarray(polys[:3000])
    sf = surface_of(points, tracks)
    want = ref_ply.ply_bytes(points, tracks, images, ref_ply.COLOR, SCALE, polys)
    has = int(ref_ply.vertex_colours(tracks, images)[0].sum())
    L = _lib.lib()
    scale = np.array(SCALE)
    # cap = 0 sizes the image and writes nothing
    rc, size, sec = raw_ply(gpu_device, points, tracks, polys, images, Color, None, 0)
    assert (rc, size) == (0, len(want)) and sec == [ref_ply.header_length(len(points), len(polys), ref_ply.COLOR), 24 * len(points) + 3 * has,
                                                     13 * len(polys)]
    # a short cap: CVHIP_ERR_INVALID, the buffer untouched
    buf = np.full(len(want), 0xA5, dtype=np.uint8)
    rc, _, _ = raw_ply(gpu_device, points, tracks, polys, images, Color, mesh._p(buf), len(want) - 1)
    assert rc == -1 and (buf == 0xA5).all()
    # a track without a point: the reference's error in Color mode, nothing written; no error in Plain mode
    lost = tracks.copy()
    lost[4000] = -1
    rc, _, _ = raw_ply(gpu_device, points, lost, polys, images, Color, mesh._p(buf), len(buf))
    assert rc == -1 and b"Track has no images" in L.cvhip_last_error() and (buf == 0xA5).all()
    rc, _, _ = raw_ply(gpu_device, points, lost, polys, images, Color, None, 0)
    assert rc == -1 and b"Track has no images" in L.cvhip_last_error()
    with pytest.raises(_lib.CvhipError, match="Track has no images"):
        mesh.ply(gpu_device, surface_of(points, lost), polys, images, Color, SCALE)
    assert same(mesh.ply(gpu_device, surface_of(points, lost), polys, None, Plain, SCALE),
                ref_ply.ply_bytes(points, lost, None, ref_ply.PLAIN, SCALE, polys))
    # no images per track at all: an error in Color mode only
    bare = np.zeros((len(points), 0, 2), dtype=np.int32)
    with pytest.raises(_lib.CvhipError, match="Track has no images") as exc:
        mesh.ply(gpu_device, surface_of(points, bare), polys, [], Color, SCALE)
    assert exc.value.code == -1
    assert same(mesh.ply(gpu_device, surface_of(points, bare), polys, None, Texture, SCALE),
                ref_ply.ply_bytes(points, bare, None, ref_ply.TEXTURE, SCALE, polys))
    # a vertex >= n, a mode that does not exist, Color mode without images: CVHIP_ERR_INVALID, nothing written
    bad = polys.copy()
    bad[len(bad) // 2, 2] = len(points)
    for args in ((points, tracks, bad, images, Color), (points, tracks, bad, None, Plain), (points, tracks, polys, images, 3),
                 (points, tracks, polys, None, Color)):
        rc, _, _ = raw_ply(gpu_device, *args, mesh._p(buf), len(buf))
        assert rc == -1 and (buf == 0xA5).all(), args[4]
    # an image shorter than its dimensions say
    img_args, _keep = mesh._image_args(images)
    short = np.array(_keep[1], dtype=np.uint64)
    short[-1] -= 1
    size = C.c_uint64(0)
    rc = L.cvhip_mesh_ply(gpu_device.handle, mesh._p(points), mesh._p(tracks), len(points), 3, img_args[0], mesh._p(short), img_args[2], 1,
                          mesh._p(scale), mesh._p(polys), len(polys), mesh._p(buf), len(buf), C.byref(size), None)
    assert rc == -1 and (buf == 0xA5).all()
    # two runs give the same bytes; device pointers give the bytes of host pointers, at an output address that is not aligned
    a, b = (mesh.ply(gpu_device, sf, polys, images, Color, SCALE) for _ in range(2))
    assert same(a, want) and a.tobytes() == b.tobytes()
    flat = np.concatenate([im.reshape(-1) for im in images])
    d_pts, d_tracks, d_poly, d_img = (torch.from_numpy(np.ascontiguousarray(x)).cuda()
                                      for x in (points, tracks, polys.view(np.int32), flat))
    for shift in (0, 1, 2, 3):
        d_out = torch.full((len(want) + 8,), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()  # (the tensors are filled on torch's stream, the library works on its own)
        size = C.c_uint64(0)
        rc = L.cvhip_mesh_ply(gpu_device.handle, C.c_void_p(d_pts.data_ptr()), C.c_void_p(d_tracks.data_ptr()), len(points), 3,
                              C.c_void_p(d_img.data_ptr()), img_args[1], img_args[2], 1, mesh._p(scale),
                              C.c_void_p(d_poly.data_ptr()), len(polys), C.c_void_p(d_out.data_ptr() + shift), len(want), C.byref(size), None)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        assert rc == 0 and size.value == len(want)
        assert same(got[shift:shift + len(want)], want) and (got[:shift] == 0x5A).all() and (got[shift + len(want):] == 0x5A).all()
    # an affine-style call: no cameras anywhere, two images per track
    # (a track whose only point was in the image dropped keeps that point, in one of the two: Color mode refuses a
    # track without one)
    pair = np.ascontiguousarray(tracks[:, 1:])
    none = np.flatnonzero(ref_ply.first_points(pair)[0] < 0)
    pair[none, none % 2] = tracks[none, 0]
    two = random_images([(320, 320), (150, 320)], seed=9)
    first, has = ref_ply.first_points(pair)[0], ref_ply.vertex_colours(pair, two)[0]
    assert len(none) and (first == 0).any() and (first == 1).any() and has.any() and (~has).any()
    got = mesh.ply(gpu_device, surface_of(points, pair), polys, two, Color, SCALE)
    assert same(got, ref_ply.ply_bytes(points, pair, two, ref_ply.COLOR, SCALE, polys))


@pytest.mark.parametrize("shape", [(1, 1), (5, 51), (257, 1), (500, 600)])
def test_colour_map(gpu_device, shape):
    """1, 255, 257 and 600 x 500 cells with NaNs, cells exactly at min and max, a range narrower than the data, the constant
    map; host and device pointers."""
    import torch

    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    depth = rng.uniform(-2.0, 7.0, shape)
    if depth.size > 1:
        depth[rng.random(shape) < 0.2] = np.nan
        depth.flat[0], depth.flat[depth.size - 1] = -2.5, 7.5
        depth.flat[depth.size // 2] = 0.5 / 255.0                     # with (0, 1): value = step / 2, ratio 0.5 exactly
    lo, hi = float(np.nanmin(depth)), float(np.nanmax(depth))
    for mn, mx in ((lo, hi), (0.0, 1.0), (0.0, 5.0), (lo, lo)):
        got = mesh.colour_map(gpu_device, depth, mn, mx, TABLE)
        assert got.shape == shape + (4,) and got.tobytes() == ref_ply.colour_map(depth, mn, mx, TABLE).tobytes(), (mn, mx)
    if depth.size > 1:
        first, last = ref_ply.colour_map(depth, lo, hi, TABLE).reshape(-1, 4)[[0, -1]]
        assert first.tolist() == [11, 7, 0, 255] and last.tolist() == [230, 162, 55, 255]   # the cells at min and max
        assert got.reshape(-1, 4)[0].tolist() == [0, 0, 0, 255]                             # the constant map's Some cells
    d_map = torch.from_numpy(depth).cuda()
    d_out = torch.zeros(shape + (4,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cvhip_mesh_colour_map(gpu_device.handle, C.c_void_p(d_map.data_ptr()), shape[1], shape[0], lo, hi, mesh._p(TABLE),
                                                C.c_void_p(d_out.data_ptr())), "cvhip_mesh_colour_map")
    torch.cuda.synchronize()
    assert d_out.cpu().numpy().tobytes() == ref_ply.colour_map(depth, lo, hi, TABLE).tobytes()


def test_depth_image_rgba(gpu_device):
    """The map stays on the device: the RGBA equals the restatement applied to mesh.depth_image's own map and range (the
    device's map, so that sin / cos differences cannot enter)."""
    s = mesh_scenes.scene(3)
    sf = mesh_scenes.device_surface(s)
    polys = mesh_scenes.polygons(s, 0)
    img = mesh.depth_image(gpu_device, sf, s.image_dims, 0, -1.0, polys)
    got = mesh.depth_image_rgba(gpu_device, sf, s.image_dims, 0, -1.0, polys, TABLE)
    assert sorted(got) == ["max_depth", "min_depth", "origin", "rgba"]
    assert (got["origin"], got["min_depth"], got["max_depth"]) == (img["origin"], img["min_depth"], img["max_depth"])
    want = ref_ply.colour_map(img["map"], img["min_depth"], img["max_depth"], TABLE)
    assert got["rgba"].shape == want.shape and got["rgba"].tobytes() == want.tobytes()
    assert 0 < (want[..., 3] == 0).sum() < want[..., 3].size and len(np.unique(want.reshape(-1, 4), axis=0)) > 100


TODAYS_KEYS = {"surface", "camera_order", "poses", "initial_pair", "sparse", "sparse_tracks", "tracks", "cameras", "projections",
               "pairs", "timings_ms", "mesh", "depth_image", "mesh_image_shapes"}


def test_reconstruct_perspective_mesh_writes_ply(gpu_device, tmp_path):
    """Config 5's scene at 512^2 with ply_path, images, Color mode and a table: the file equals the restatement on the
    returned surface and list and parses; without the new keywords the dict has today's keys."""
    pytest.importorskip("scipy")
    size = 512
    views, K, _ = synth.make_sfm_views(size)
    steps = synth.optimal_scale_steps(size, size)
    pyrs = [synth.box_pyramid(v, steps) for v in views]
    images = [np.stack([np.asarray(v, dtype=np.uint8), 255 - np.asarray(v, dtype=np.uint8), np.asarray(v, dtype=np.uint8) // 2], axis=2)
              for v in views]
    path = tmp_path / "surface.ply"
    scale = (1.0, 1.0, -2.0)
    out = reconstruction.reconstruct_perspective_mesh(gpu_device, pyrs, K, project_to_image=0, bundle_adjustment=False, seed=3,
                                                      ply_path=str(path), images=images, vertex_mode=mesh.VertexMode.Color,
                                                      out_scale=scale, colour_table=TABLE)
    surface, polys = out["surface"], out["mesh"]["polygons"]
    assert len(surface.cameras) == 3 and len(surface.points) > 20000 and len(polys) > 20000
    data = path.read_bytes()
    assert data == ref_ply.ply_bytes(surface.points, surface.tracks, images, ref_ply.COLOR, scale, polys)
    end, n, n_poly, coloured = ref_ply.parse_header(data)
    assert (n, n_poly, coloured) == (len(surface.points), len(polys), True)
    assert out["ply_sections"][0] == end and sum(out["ply_sections"]) == len(data) and out["ply_sections"][2] == 13 * n_poly
    assert 24 * n <= out["ply_sections"][1] <= 27 * n and out["timings_ms"]["ply"] > 0.0
    img = out["depth_image"]
    assert img["rgba"].tobytes() == ref_ply.colour_map(img["map"], img["min_depth"], img["max_depth"], TABLE).tobytes()
    assert set(out) == TODAYS_KEYS | {"ply_sections"} and set(img) == {"map", "origin", "min_depth", "max_depth", "wide", "rgba"}
    plain = reconstruction.reconstruct_perspective_mesh(gpu_device, pyrs, K, project_to_image=0, bundle_adjustment=False, seed=3)
    assert set(plain) == TODAYS_KEYS and set(plain["depth_image"]) == {"map", "origin", "min_depth", "max_depth", "wide"}
    assert set(plain["timings_ms"]) == set(out["timings_ms"]) - {"ply"}
