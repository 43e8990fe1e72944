"""The OBJ writer on the device (cvhip_mesh_obj, cvhip_mesh_obj_mtl, cvhip_f64_display; csrc/mesh_obj_kernels.hip,
csrc/f64_display.hpp) against tests/ref_obj.py.  Every comparison is byte equality, with no tolerance: the
expected text comes from Python's repr, code that is not under test."""
import ctypes as C
import functools

import numpy as np
import pytest

import obj_scenes
import ref_obj
from cybervision_amd import _lib, mesh, reconstruction, synth
from ply_scenes import SCALE, surface_of

pytestmark = pytest.mark.gpu
Plain, Color, Texture = mesh.VertexMode.Plain, mesh.VertexMode.Color, mesh.VertexMode.Texture
ONE = (1.0, 1.0, 1.0)


def same(got, want):
    got = np.asarray(got, dtype=np.uint8).tobytes()
    if got != want:
        k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        pytest.fail(f"file images differ: {len(got)} against {len(want)} bytes, first difference at byte {k}: "
                    f"{got[max(k - 40, 0):k + 40]!r} against {want[max(k - 40, 0):k + 40]!r}")
    return True


@functools.lru_cache(maxsize=None)
def scene_want(mode):
    points, tracks, polys, camera, images = obj_scenes.scene()
    return ref_obj.obj_bytes(points, tracks, images, mode, SCALE, polys, camera, "scene")


def test_f64_display_value_set(gpu_device):
    """The formatter on the device, on the CPU test's value set with 200 000 random bit patterns: host pointers, then device
    pointers."""
    import torch

    values = obj_scenes.value_set(200_000)
    assert 400_000 < len(values) < 420_000
    want = [ref_obj.display_a(v) for v in values.tolist()]
    got = mesh.f64_display(gpu_device, values)
    wrong = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert len(got) == len(want) and not wrong, [(values[i].hex(), got[i], want[i]) for i in wrong[:5]]
    text = "".join(want).encode("ascii")
    ends = np.cumsum([0] + [len(w) for w in want]).astype(np.uint64)
    d_values = torch.from_numpy(values).cuda()
    d_out = torch.full((len(text) + 8,), 0x5A, dtype=torch.uint8, device="cuda")
    d_offsets = torch.zeros(len(values) + 1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()  # (the tensors are filled on torch's stream, the library works on its own)
    size = C.c_uint64(0)
    L = _lib.lib()
    assert L.cvhip_f64_display(gpu_device.handle, C.c_void_p(d_values.data_ptr()), len(values), None, 0, C.byref(size), None) == 0
    assert size.value == len(text)
    rc = L.cvhip_f64_display(gpu_device.handle, C.c_void_p(d_values.data_ptr()), len(values), C.c_void_p(d_out.data_ptr() + 1), len(text),
                             C.byref(size), C.c_void_p(d_offsets.data_ptr()))
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert rc == 0 and out[1:1 + len(text)].tobytes() == text and out[0] == 0x5A and (out[1 + len(text):] == 0x5A).all()
    assert (d_offsets.cpu().numpy().view(np.uint64) == ends).all()
    # nothing to format; a buffer that is too small
    assert mesh.f64_display(gpu_device, np.zeros(0)) == []
    buf = np.full(8, 0xA5, dtype=np.uint8)
    assert L.cvhip_f64_display(gpu_device.handle, mesh._p(values[:100]), 100, mesh._p(buf), 8, C.byref(size), None) == -1
    assert (buf == 0xA5).all()


def test_whole_file_three_modes(gpu_device):
    points, tracks, polys, camera, images = obj_scenes.scene()
    sf = surface_of(points, tracks)
    counts = (tracks[:, :, 0] >= 0).sum(axis=1)
    assert len(points) == 12288 and [int((counts == k).sum()) for k in (1, 2, 3)] == [1067, 5835, 5386]
    assert [int((camera == c).sum()) for c in range(3)] == [12941, 12910, 12526]
    # what makes the scene a test: every block of 256 tracks holds v lines of many lengths, in Color mode with and without colour.
    # (Plain lines are 15 .. 65 bytes, 14.5 .. 15.6 KB a block, but a block has only 6 .. 9 DISTINCT lengths: most lines have
    # three numbers of 16 to 19 characters.  With colours every block has 12 or more.)
    for mode, distinct in ((ref_obj.PLAIN, 6), (ref_obj.COLOR, 10)):
        lines = scene_want(mode).split(b"\n")[:len(points)]
        lengths = np.array([len(line) + 1 for line in lines]).reshape(48, 256)
        assert all(len(np.unique(row)) >= distinct for row in lengths)
        if mode == ref_obj.PLAIN:
            assert (lengths.min(), lengths.max()) == (15, 65) and 14_000 < lengths.sum(axis=1).min() and lengths.sum(axis=1).max() < 16_000
        else:
            coloured = np.array([line.count(b" ") == 6 for line in lines]).reshape(48, 256)
            assert coloured.any(axis=1).all() and (~coloured).any(axis=1).all()
    for mode in (Plain, Color, Texture):
        sections = []
        got = mesh.obj(gpu_device, sf, polys, camera, None if mode == Plain else images, mode, SCALE, stem="scene", sections=sections)
        assert same(got, scene_want(int(mode))), mode
        assert sum(sections) == len(got) and sections == ref_obj.obj_sections(scene_want(int(mode)), int(mode))
    assert sections[0] == len(b"mtllib scene.mtl\n") and sections[2] > 0
    # Texture mode reads only the sizes of the images
    dims = [(im.shape[1], im.shape[0]) for im in images]
    assert same(mesh.obj(gpu_device, sf, polys, camera, dims, Texture, SCALE, stem="scene"), scene_want(ref_obj.TEXTURE))
    # images that are given but not needed are not read
    assert same(mesh.obj(gpu_device, sf, polys, camera, images, Plain, SCALE, stem="scene"), scene_want(ref_obj.PLAIN))


def test_long_records(gpu_device):
    """A block of 256 lines of ~985 bytes (~250 KB, past any staging buffer), a block that alternates 900-byte and 9-byte lines,
    and an ordinary one."""
    points, tracks, polys, camera = obj_scenes.long_records()
    want = ref_obj.obj_bytes(points, tracks, None, ref_obj.PLAIN, ONE, polys, camera, "long")
    lines = want.split(b"\n")
    assert sum(len(line) + 1 for line in lines[:256]) > 245_000 and max(len(line) for line in lines[:256]) > 980
    assert min(len(line) for line in lines[256:512]) == 8 and max(len(line) for line in lines[256:512]) > 900
    sections = []
    got = mesh.obj(gpu_device, surface_of(points, tracks), polys, camera, None, Plain, ONE, stem="long", sections=sections)
    assert same(got, want) and sections == ref_obj.obj_sections(want, ref_obj.PLAIN)


def raw_obj(gpu_device, points, tracks, polys, camera, images, mode, out, cap, stem=b"scene", scale=SCALE):
    """cvhip_mesh_obj itself -> (rc, size, sections); out: a C pointer or None; images: arrays, (width, height) pairs or None"""
    n, m = len(points), tracks.shape[1]
    if images is None:
        img_args, keep = [None, None, None], None
    elif hasattr(images[0], "shape"):
        img_args, keep = mesh._image_args(images)
    else:
        img_args, keep = mesh._dims_args(images)
    scale = np.array(scale, dtype=np.float64)
    size, sec = C.c_uint64(0), np.zeros(4, dtype=np.uint64)
    rc = _lib.lib().cvhip_mesh_obj(gpu_device.handle, mesh._p(points), mesh._p(tracks), n, m, *img_args, int(mode), mesh._p(scale),
                                   mesh._p(polys), mesh._p(camera) if camera is not None else None, len(polys), stem, out, cap,
                                   C.byref(size), mesh._p(sec))
    return rc, size.value, [int(v) for v in sec]


def test_grid_edges(gpu_device):
    """0, 1, one short of, exactly and one past a block of 256 tracks, crossed with 0, 1 and 257 polygons, in Plain and Texture
    mode.  Polygons without tracks name a vertex >= n."""
    points, tracks, polys, camera, images = obj_scenes.scene()
    dims = [(im.shape[1], im.shape[0]) for im in images]
    pick = np.r_[0:86, 12941:13027, 25851:25936]                         # 257 polygons of the three cameras
    for n in (0, 1, 255, 256, 257):
        for n_poly in (0, 1, 257):
            sub_p, sub_t = points[:n], tracks[:n]
            sub_poly = (polys[pick[:n_poly]] % max(n, 1)).astype(np.uint32)
            sub_cam = np.ascontiguousarray(camera[pick[:n_poly]])
            for mode in (Plain, Texture):
                if n == 0 and n_poly:
                    with pytest.raises(_lib.CvhipError, match="names a track >= n"):
                        mesh.obj(gpu_device, surface_of(sub_p, sub_t), sub_poly, sub_cam, dims, mode, SCALE, stem="e")
                    continue
                got = mesh.obj(gpu_device, surface_of(sub_p, sub_t), sub_poly, sub_cam, dims, mode, SCALE, stem="e")
                assert same(got, ref_obj.obj_bytes(sub_p, sub_t, dims, int(mode), SCALE, sub_poly, sub_cam, "e")), (n, n_poly, mode)
    empty = surface_of(points[:0], tracks[:0])
    assert mesh.obj(gpu_device, empty, polys[:0], camera[:0], None, Plain, SCALE).size == 0
    assert mesh.obj(gpu_device, empty, polys[:0], camera[:0], dims, Texture, SCALE, stem="e").tobytes() == b"mtllib e.mtl\n"


def test_sizing_alignment_pointers(gpu_device):
    import torch

    points, tracks, polys, camera, images = obj_scenes.scene()
    pick = np.r_[0:1500, 12941:14000, 25851:27000]
    polys, camera = np.ascontiguousarray(polys[pick]), np.ascontiguousarray(camera[pick])
    dims = [(im.shape[1], im.shape[0]) for im in images]
    want = ref_obj.obj_bytes(points, tracks, dims, ref_obj.TEXTURE, SCALE, polys, camera, "scene")
    # cap = 0 sizes the image and writes nothing
    rc, size, sec = raw_obj(gpu_device, points, tracks, polys, camera, dims, Texture, None, 0)
    assert (rc, size) == (0, len(want)) and sec == ref_obj.obj_sections(want, ref_obj.TEXTURE)
    # a short cap: CVHIP_ERR_INVALID, the buffer untouched
    buf = np.full(len(want), 0xA5, dtype=np.uint8)
    rc, _, _ = raw_obj(gpu_device, points, tracks, polys, camera, dims, Texture, mesh._p(buf), len(want) - 1)
    assert rc == -1 and (buf == 0xA5).all()
    # device pointers, the output at every alignment, canaries around it
    d_pts, d_tracks, d_poly, d_cam = (torch.from_numpy(np.ascontiguousarray(x)).cuda()
                                      for x in (points, tracks, polys.view(np.int32), camera.view(np.int32)))
    img_args, _keep = mesh._dims_args(dims)
    scale = np.array(SCALE)
    for shift in (0, 1, 2, 3):
        d_out = torch.full((len(want) + 16,), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()  # (the tensors are filled on torch's stream, the library works on its own)
        size = C.c_uint64(0)
        rc = _lib.lib().cvhip_mesh_obj(gpu_device.handle, C.c_void_p(d_pts.data_ptr()), C.c_void_p(d_tracks.data_ptr()), len(points), 3,
                                       *img_args, int(Texture), mesh._p(scale), C.c_void_p(d_poly.data_ptr()), C.c_void_p(d_cam.data_ptr()),
                                       len(polys), b"scene", C.c_void_p(d_out.data_ptr() + 8 + shift), len(want), C.byref(size), None)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        assert rc == 0 and size.value == len(want)
        assert same(got[8 + shift:8 + shift + len(want)], want)
        assert (got[:8 + shift] == 0x5A).all() and (got[8 + shift + len(want):] == 0x5A).all()
    # two runs give the same bytes
    sf = surface_of(points, tracks)
    a, b = (mesh.obj(gpu_device, sf, polys, camera, images, Color, SCALE, stem="scene") for _ in range(2))
    assert a.tobytes() == b.tobytes() and same(a, ref_obj.obj_bytes(points, tracks, images, ref_obj.COLOR, SCALE, polys, camera, "scene"))


def test_texture_rules(gpu_device):
    points, tracks, dims, polys, camera, text = obj_scenes.texture_five()
    sf = surface_of(points, tracks)
    sections = []
    assert same(mesh.obj(gpu_device, sf, polys, camera, dims, Texture, ONE, stem="five", sections=sections), text)
    assert sections == [16, 97, 177, 142]
    # a camera past the track's images takes all of the track's points
    far = np.array([7, 3, 2, 0xFFFFFFFF, 0], dtype=np.uint32)
    got = mesh.obj(gpu_device, sf, polys, far, dims, Texture, ONE, stem="five")
    assert same(got, ref_obj.obj_bytes_scalar(points, tracks, dims, ref_obj.TEXTURE, ONE, polys, far, "five"))
    assert b"usemtl Textured4294967295\n" in got.tobytes() and got.tobytes().count(b"usemtl") == 5
    # an image of width 0, one of height 0: NaN, inf and -inf, restated
    zero = [(0, 16), (20, 0), (40, 80)]
    got = mesh.obj(gpu_device, sf, polys, camera, zero, Texture, ONE, stem="five")
    assert same(got, ref_obj.obj_bytes(points, tracks, zero, ref_obj.TEXTURE, ONE, polys, camera, "five"))
    assert b"vt NaN 1\n" in got.tobytes() and b"vt inf 0.5\n" in got.tobytes() and b"vt 0.5 -inf\n" in got.tobytes()
    assert mesh.obj_mtl("five", 3) == ref_obj.mtl_bytes("five", 3) and mesh.obj_mtl("x", 0) == b""


def test_errors(gpu_device):
    points, tracks, polys, camera, images = obj_scenes.scene()
    polys, camera = np.ascontiguousarray(polys[:3000]), np.ascontiguousarray(camera[:3000])
    dims = [(im.shape[1], im.shape[0]) for im in images]
    L = _lib.lib()
    buf = np.full(3_000_000, 0xA5, dtype=np.uint8)
    # a track without a point: the reference's error in Color and Texture mode, nothing written; no error in Plain mode
    lost = tracks.copy()
    lost[4000] = -1
    for mode, imgs in ((Color, images), (Texture, dims)):
        rc, _, _ = raw_obj(gpu_device, points, lost, polys, camera, imgs, mode, mesh._p(buf), len(buf))
        assert rc == -1 and b"Track has no images" in L.cvhip_last_error() and (buf == 0xA5).all()
        rc, _, _ = raw_obj(gpu_device, points, lost, polys, camera, imgs, mode, None, 0)
        assert rc == -1 and b"Track has no images" in L.cvhip_last_error()
        with pytest.raises(_lib.CvhipError, match="Track has no images"):
            mesh.obj(gpu_device, surface_of(points, lost), polys, camera, imgs, mode, SCALE)
    assert same(mesh.obj(gpu_device, surface_of(points, lost), polys, camera, None, Plain, SCALE),
                ref_obj.obj_bytes(points, lost, None, ref_obj.PLAIN, SCALE, polys, camera, "mesh"))
    # a vertex >= n, in every mode
    bad = polys.copy()
    bad[len(bad) // 2, 2] = len(points)
    for mode, imgs in ((Plain, None), (Color, images), (Texture, dims)):
        rc, _, _ = raw_obj(gpu_device, points, tracks, bad, camera, imgs, mode, mesh._p(buf), len(buf))
        assert rc == -1 and b"names a track >= n" in L.cvhip_last_error() and (buf == 0xA5).all()
    # Texture mode without a stem, without cameras, without sizes; Color mode without images; a mode that does not exist
    for args, kw in (((points, tracks, polys, camera, dims, Texture), {"stem": None}), ((points, tracks, polys, None, dims, Texture), {}),
                     ((points, tracks, polys, camera, None, Texture), {}), ((points, tracks, polys, camera, None, Color), {}),
                     ((points, tracks, polys, camera, dims, Color), {}), ((points, tracks, polys, camera, images, 3), {})):
        rc, _, _ = raw_obj(gpu_device, *args, mesh._p(buf), len(buf), **kw)
        assert rc == -1 and (buf == 0xA5).all(), args[5]
    # Plain mode needs neither
    rc, size, _ = raw_obj(gpu_device, points, tracks, polys, None, None, Plain, mesh._p(buf), len(buf), stem=None)
    want = ref_obj.obj_bytes(points, tracks, None, ref_obj.PLAIN, SCALE, polys, camera, "scene")
    assert rc == 0 and size == len(want) and same(buf[:size], want) and (buf[size:] == 0xA5).all()


TODAYS_KEYS = {"surface", "camera_order", "poses", "initial_pair", "sparse", "sparse_tracks", "tracks", "cameras", "projections",
               "pairs", "timings_ms", "mesh", "depth_image", "mesh_image_shapes"}


def test_reconstruct_perspective_mesh_writes_obj(gpu_device, tmp_path):
    """Config 5's scene at 512^2 with obj_path in Texture mode: the .obj equals the restatement on the returned surface and
    list, the .mtl its text; a call without obj_path writes neither and has today's keys."""
    pytest.importorskip("scipy")
    size = 512
    views, K, _ = synth.make_sfm_views(size)
    steps = synth.optimal_scale_steps(size, size)
    pyrs = [synth.box_pyramid(v, steps) for v in views]
    images = [np.stack([np.asarray(v, dtype=np.uint8)] * 3, axis=2) for v in views]
    path = tmp_path / "with" / "surface.obj"
    path.parent.mkdir()
    scale = (1.0, 1.0, -2.0)
    out = reconstruction.reconstruct_perspective_mesh(gpu_device, pyrs, K, bundle_adjustment=False, seed=3, obj_path=str(path),
                                                      images=images, vertex_mode=Texture, out_scale=scale)
    surface, polys, camera = out["surface"], out["mesh"]["polygons"], out["mesh"]["camera"]
    assert len(surface.cameras) == 3 and len(surface.points) > 20000 and len(polys) > 20000 and len(set(camera.tolist())) > 1
    data = path.read_bytes()
    assert data == ref_obj.obj_bytes(surface.points, surface.tracks, images, ref_obj.TEXTURE, scale, polys, camera, "surface")
    assert (path.parent / "surface.mtl").read_bytes() == ref_obj.mtl_bytes("surface", 3)
    assert list(out["obj_sections"]) == ref_obj.obj_sections(data, ref_obj.TEXTURE) and out["timings_ms"]["obj"] > 0.0
    assert set(out) == TODAYS_KEYS | {"obj_sections"} and sorted(p.name for p in path.parent.iterdir()) == ["surface.mtl", "surface.obj"]
    plain = reconstruction.reconstruct_perspective_mesh(gpu_device, pyrs, K, bundle_adjustment=False, seed=3)
    assert set(plain) == TODAYS_KEYS and set(plain["timings_ms"]) == set(out["timings_ms"]) - {"obj"}
    assert sorted(p.name for p in tmp_path.iterdir()) == ["with"]
