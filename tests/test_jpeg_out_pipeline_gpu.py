"""The JPEG file of the depth map: mesh.write_depth_jpeg and the keywords of the reconstructions that ask for
it.  The file on disk is tests/ref_jpeg_out.py's file of the depth map's RGB (alpha dropped)."""
import pytest

import cases
import mesh_scenes
import ref_jpeg_out
import ref_ply
from cybervision_amd import mesh, reconstruction
from cybervision_amd.mesh import write_depth_jpeg  # (without the encoder every test here fails at this import)

pytestmark = pytest.mark.gpu
TABLE = ref_ply.generated_table()


def test_write_depth_jpeg_is_the_depth_maps_rgb(gpu_device, tmp_path):
    s = mesh_scenes.scene(3)
    sf = mesh_scenes.device_surface(s)
    polys = mesh_scenes.polygons(s, 0)
    want = mesh.depth_image_rgba(gpu_device, sf, s.image_dims, 0, -1.0, polys, TABLE)
    rgba = want["rgba"]
    assert 0 < (rgba[..., 3] == 0).sum() < rgba[..., 3].size  # cells without a depth and cells with one
    for quality, sampling, optimize in ((75, mesh.JpegSampling.S420, False), (90, mesh.JpegSampling.S444, True)):
        got = write_depth_jpeg(tmp_path / "depth.jpg", gpu_device, sf, s.image_dims, 0, -1.0, polys, TABLE, quality, sampling, optimize)
        restated = ref_jpeg_out.encode(rgba[..., :3], quality, int(sampling), optimize)
        assert (tmp_path / "depth.jpg").read_bytes() == restated["file"] == ref_jpeg_out.encode(rgba, quality, int(sampling), optimize)["file"]
        assert (got["width"], got["height"]) == (rgba.shape[1], rgba.shape[0]) and got["sections"] == restated["sections"]
        assert (got["origin"], got["min_depth"], got["max_depth"]) == (want["origin"], want["min_depth"], want["max_depth"])


def test_reconstruct_affine_mesh_jpeg_keywords(gpu_device, tmp_path):
    c = cases.make_case("tilt3_200x150")
    p1, p2 = cases.pyramids(c)
    with pytest.raises(ValueError):
        reconstruction.reconstruct_affine_mesh(gpu_device, p1, p2, c["F"], depth_jpeg_path=str(tmp_path / "d.jpg"))
    with pytest.raises(ValueError):
        reconstruction.reconstruct_affine_mesh(gpu_device, p1, p2, c["F"], project_to_image=0, depth_jpeg_path=str(tmp_path / "d.jpg"))
    with pytest.raises(ValueError):
        reconstruction.reconstruct_perspective_mesh(gpu_device, [], None, depth_jpeg_path=str(tmp_path / "d.jpg"))
    assert list(tmp_path.iterdir()) == []
    plain = reconstruction.reconstruct_affine_mesh(gpu_device, p1, p2, c["F"], project_to_image=0, colour_table=TABLE)
    out = reconstruction.reconstruct_affine_mesh(gpu_device, p1, p2, c["F"], project_to_image=0, colour_table=TABLE,
                                                 depth_jpeg_path=str(tmp_path / "depth.jpg"), jpeg_quality=60)
    assert [p.name for p in tmp_path.iterdir()] == ["depth.jpg"]
    assert set(out) == set(plain) | {"depth_jpeg"} and set(out["timings_ms"]) == set(plain["timings_ms"]) | {"jpeg"}
    assert out["timings_ms"]["jpeg"] > 0.0
    rgba = out["depth_image"]["rgba"]
    assert rgba.tobytes() == plain["depth_image"]["rgba"].tobytes()
    restated = ref_jpeg_out.encode(rgba[..., :3], 60, ref_jpeg_out.S420, False)
    assert (tmp_path / "depth.jpg").read_bytes() == restated["file"]
    assert out["depth_jpeg"]["sections"] == restated["sections"] and (out["depth_jpeg"]["width"], out["depth_jpeg"]["height"]) == rgba.shape[1::-1]
