"""The PNG files of the mesh output: the textures an OBJ's .mtl names (mesh.write_obj(save_textures=True)),
the depth map (mesh.write_depth_png) and the keywords of the reconstructions that ask for them.  Pillow, which shares nothing
with the encoder, must open every file to exactly the pixels that went in."""
import re

import numpy as np
import pytest
from PIL import Image

import cases
import mesh_scenes
import obj_scenes
import ref_ply
from cybervision_amd import mesh, reconstruction, synth
from ply_scenes import SCALE, surface_of

pytestmark = pytest.mark.gpu
TABLE = ref_ply.generated_table()
Texture = mesh.VertexMode.Texture


def opened(path):
    im = Image.open(path)
    im.load()
    return im


def test_write_obj_saves_the_textures_the_mtl_names(gpu_device, tmp_path):
    points, tracks, polys, camera, images = obj_scenes.scene()
    sf = surface_of(points, tracks)
    with_dir, without_dir = tmp_path / "with", tmp_path / "without"
    with_dir.mkdir(), without_dir.mkdir()
    before = mesh.write_obj(without_dir / "scene.obj", gpu_device, sf, polys, camera, images, Texture, SCALE)
    assert sorted(p.name for p in without_dir.iterdir()) == ["scene.mtl", "scene.obj"]  # the default: what it was
    sections = mesh.write_obj(with_dir / "scene.obj", gpu_device, sf, polys, camera, images, Texture, SCALE, save_textures=True)
    assert sections == before
    assert (with_dir / "scene.obj").read_bytes() == (without_dir / "scene.obj").read_bytes()
    mtl = (with_dir / "scene.mtl").read_bytes()
    assert mtl == (without_dir / "scene.mtl").read_bytes() == mesh.obj_mtl("scene", len(images))
    named = sorted(set(re.findall(rb"map_Kd (\S+)", mtl)))
    assert named == sorted(b"scene-%d.png" % i for i in range(len(images))) and len(named) == 3
    assert sorted(p.name for p in with_dir.iterdir()) == sorted(["scene.mtl", "scene.obj"] + [n.decode() for n in named])
    for i, want in enumerate(images):
        im = opened(with_dir / ("scene-%d.png" % i))
        assert im.mode == "RGB" and im.size == (want.shape[1], want.shape[0])  # 8-bit colour type 2, as the reference's files
        assert (np.asarray(im) == want).all()
    # sizes instead of arrays, or another mode: there is nothing to save
    other = tmp_path / "other"
    other.mkdir()
    mesh.write_obj(other / "a.obj", gpu_device, sf, polys, camera, [(im.shape[1], im.shape[0]) for im in images], Texture, SCALE,
                   save_textures=True)
    mesh.write_obj(other / "b.obj", gpu_device, sf, polys, camera, images, mesh.VertexMode.Color, SCALE, save_textures=True)
    assert sorted(p.name for p in other.iterdir()) == ["a.mtl", "a.obj", "b.obj"]


def test_write_depth_png_is_the_depth_maps_rgba(gpu_device, tmp_path):
    s = mesh_scenes.scene(3)
    sf = mesh_scenes.device_surface(s)
    polys = mesh_scenes.polygons(s, 0)
    want = mesh.depth_image_rgba(gpu_device, sf, s.image_dims, 0, -1.0, polys, TABLE)
    got = mesh.write_depth_png(tmp_path / "depth.png", gpu_device, sf, s.image_dims, 0, -1.0, polys, TABLE)
    im = opened(tmp_path / "depth.png")
    rgba = want["rgba"]
    assert im.mode == "RGBA" and im.size == (rgba.shape[1], rgba.shape[0]) == (got["width"], got["height"])  # 8-bit colour type 6
    assert (np.asarray(im) == rgba).all()
    assert (got["origin"], got["min_depth"], got["max_depth"]) == (want["origin"], want["min_depth"], want["max_depth"])
    assert sum(got["sections"]) == (tmp_path / "depth.png").stat().st_size and got["sections"][0] == 41 and got["sections"][2] == 16
    assert 0 < (rgba[..., 3] == 0).sum() < rgba[..., 3].size  # cells without a depth and cells with one


def test_reconstruct_perspective_mesh_png_keywords(gpu_device, tmp_path):
    """Config 5's scene at 512^2, Texture mode: the three textures and the depth map next to the .obj."""
    size = 512
    views, K, _ = synth.make_sfm_views(size)
    steps = synth.optimal_scale_steps(size, size)
    pyrs = [synth.box_pyramid(v, steps) for v in views]
    images = [np.stack([np.asarray(v, dtype=np.uint8), 255 - np.asarray(v, dtype=np.uint8), np.asarray(v, dtype=np.uint8) // 2], axis=2)
              for v in views]
    out = reconstruction.reconstruct_perspective_mesh(gpu_device, pyrs, K, triangulate=mesh.delaunay_device(gpu_device), project_to_image=0,
                                                      bundle_adjustment=False, seed=3, obj_path=str(tmp_path / "s.obj"), images=images,
                                                      vertex_mode=Texture, colour_table=TABLE, save_textures=True,
                                                      depth_png_path=str(tmp_path / "depth.png"))
    m = len(out["surface"].cameras)
    assert m >= 2 and len(out["mesh"]["polygons"]) > 1000
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(["depth.png", "s.mtl", "s.obj"] + ["s-%d.png" % i for i in range(m)])
    for i in range(m):
        assert (np.asarray(opened(tmp_path / ("s-%d.png" % i))) == images[i]).all()
    assert (np.asarray(opened(tmp_path / "depth.png")) == out["depth_image"]["rgba"]).all()
    assert out["timings_ms"]["png"] > 0.0 and out["depth_png"]["sections"][0] == 41


def test_reconstruct_affine_mesh_png_keywords(gpu_device, tmp_path):
    c = cases.make_case("tilt3_200x150")
    p1, p2 = cases.pyramids(c)
    images = [np.stack([np.asarray(im, dtype=np.uint8), 255 - np.asarray(im, dtype=np.uint8), np.asarray(im, dtype=np.uint8) // 2], axis=2)
              for im in (c["img1"], c["img2"])]
    with pytest.raises(ValueError):
        reconstruction.reconstruct_affine_mesh(gpu_device, p1, p2, c["F"], depth_png_path=str(tmp_path / "d.png"))
    with pytest.raises(ValueError):
        reconstruction.reconstruct_affine_mesh(gpu_device, p1, p2, c["F"], project_to_image=0, depth_png_path=str(tmp_path / "d.png"))
    with pytest.raises(ValueError):
        reconstruction.reconstruct_perspective_mesh(gpu_device, [], None, depth_png_path=str(tmp_path / "d.png"))
    assert list(tmp_path.iterdir()) == []
    plain_dir, png_dir = tmp_path / "plain", tmp_path / "png"
    plain_dir.mkdir(), png_dir.mkdir()
    plain = reconstruction.reconstruct_affine_mesh(gpu_device, p1, p2, c["F"], project_to_image=0, obj_path=str(plain_dir / "s.obj"),
                                                   images=images, vertex_mode=Texture, colour_table=TABLE)
    out = reconstruction.reconstruct_affine_mesh(gpu_device, p1, p2, c["F"], project_to_image=0, obj_path=str(png_dir / "s.obj"),
                                                 images=images, vertex_mode=Texture, colour_table=TABLE, save_textures=True,
                                                 depth_png_path=str(png_dir / "depth.png"))
    assert sorted(p.name for p in plain_dir.iterdir()) == ["s.mtl", "s.obj"]  # the defaults write what they wrote
    assert sorted(p.name for p in png_dir.iterdir()) == ["depth.png", "s-0.png", "s-1.png", "s.mtl", "s.obj"]
    assert set(out) == set(plain) | {"depth_png"} and set(out["timings_ms"]) == set(plain["timings_ms"]) | {"png"}
    assert out["timings_ms"]["png"] > 0.0
    for i, want in enumerate(images):
        assert (np.asarray(opened(png_dir / ("s-%d.png" % i))) == want).all()
    depth = opened(png_dir / "depth.png")
    assert depth.mode == "RGBA" and (np.asarray(depth) == out["depth_image"]["rgba"]).all()
    assert out["depth_image"]["rgba"].tobytes() == plain["depth_image"]["rgba"].tobytes()
