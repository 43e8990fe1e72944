"""The TIFF file of the depth map: mesh.write_depth_tiff and the keyword of the reconstructions that asks for
it.  The file on disk is tests/ref_tiff_out.py's file of the depth map's RGBA, and reads back to it."""
import numpy as np
import pytest

import cases
import mesh_scenes
import ref_ply
import ref_tiff
import ref_tiff_out
from cybervision_amd import mesh, reconstruction
from cybervision_amd.mesh import write_depth_tiff  # (without the encoder every test here fails at this import)

pytestmark = pytest.mark.gpu
TABLE = ref_ply.generated_table()


def test_write_depth_tiff_is_the_depth_maps_rgba(gpu_device, tmp_path):
    s = mesh_scenes.scene(3)
    sf = mesh_scenes.device_surface(s)
    polys = mesh_scenes.polygons(s, 0)
    want = mesh.depth_image_rgba(gpu_device, sf, s.image_dims, 0, -1.0, polys, TABLE)
    rgba = want["rgba"]
    assert 0 < (rgba[..., 3] == 0).sum() < rgba[..., 3].size  # cells without a depth and cells with one
    for compression, predictor in ((mesh.TiffCompression.LZW, None), (mesh.TiffCompression.PACKBITS, None), (mesh.TiffCompression.NONE, 1)):
        got = write_depth_tiff(tmp_path / "depth.tif", gpu_device, sf, s.image_dims, 0, -1.0, polys, TABLE, compression, predictor)
        sections = []
        restated = ref_tiff_out.encode(rgba, int(compression), 2 if compression == mesh.TiffCompression.LZW else 1, 0, sections=sections)
        assert (tmp_path / "depth.tif").read_bytes() == restated
        assert (got["width"], got["height"]) == (rgba.shape[1], rgba.shape[0]) and got["sections"] == tuple(sections)
        assert (got["origin"], got["min_depth"], got["max_depth"]) == (want["origin"], want["min_depth"], want["max_depth"])
        assert np.array_equal(ref_tiff.samples(restated)[1], rgba)


def test_reconstruct_affine_mesh_tiff_keyword(gpu_device, tmp_path):
    c = cases.make_case("tilt3_200x150")
    p1, p2 = cases.pyramids(c)
    with pytest.raises(ValueError):
        reconstruction.reconstruct_affine_mesh(gpu_device, p1, p2, c["F"], depth_tiff_path=str(tmp_path / "d.tif"))
    with pytest.raises(ValueError):
        reconstruction.reconstruct_affine_mesh(gpu_device, p1, p2, c["F"], project_to_image=0, depth_tiff_path=str(tmp_path / "d.tif"))
    with pytest.raises(ValueError):
        reconstruction.reconstruct_perspective_mesh(gpu_device, [], None, depth_tiff_path=str(tmp_path / "d.tif"))
    with pytest.raises(ValueError):
        reconstruction.reconstruct_perspective_mesh(gpu_device, [], None, project_to_image=0, depth_tiff_path=str(tmp_path / "d.tif"))
    assert list(tmp_path.iterdir()) == []
    plain = reconstruction.reconstruct_affine_mesh(gpu_device, p1, p2, c["F"], project_to_image=0, colour_table=TABLE)
    out = reconstruction.reconstruct_affine_mesh(gpu_device, p1, p2, c["F"], project_to_image=0, colour_table=TABLE,
                                                 depth_tiff_path=str(tmp_path / "depth.tif"))
    assert [p.name for p in tmp_path.iterdir()] == ["depth.tif"]
    assert set(out) == set(plain) | {"depth_tiff"} and set(out["timings_ms"]) == set(plain["timings_ms"]) | {"tiff"}
    assert out["timings_ms"]["tiff"] > 0.0
    rgba = out["depth_image"]["rgba"]
    assert rgba.tobytes() == plain["depth_image"]["rgba"].tobytes()
    sections = []
    restated = ref_tiff_out.encode(rgba, ref_tiff_out.LZW, 2, 0, sections=sections)
    data = (tmp_path / "depth.tif").read_bytes()
    assert data == restated and np.array_equal(ref_tiff.samples(data)[1], rgba)
    assert out["depth_tiff"]["sections"] == tuple(sections) and (out["depth_tiff"]["width"], out["depth_tiff"]["height"]) == rgba.shape[1::-1]


def test_reconstruct_perspective_mesh_tiff_keyword(gpu_device, tmp_path):
    """The scene of the PNG pipeline test (three views at 512^2): the depth map next to nothing else."""
    from cybervision_amd import synth

    size = 512
    views, K, _ = synth.make_sfm_views(size)
    steps = synth.optimal_scale_steps(size, size)
    pyrs = [synth.box_pyramid(v, steps) for v in views]
    out = reconstruction.reconstruct_perspective_mesh(gpu_device, pyrs, K, triangulate=mesh.delaunay_device(gpu_device), project_to_image=0,
                                                      bundle_adjustment=False, seed=3, colour_table=TABLE,
                                                      depth_tiff_path=str(tmp_path / "depth.tif"))
    assert [p.name for p in tmp_path.iterdir()] == ["depth.tif"]
    rgba = out["depth_image"]["rgba"]
    data = (tmp_path / "depth.tif").read_bytes()
    sections = []
    assert data == ref_tiff_out.encode(rgba, ref_tiff_out.LZW, 2, 0, sections=sections)
    assert np.array_equal(ref_tiff.samples(data)[1], rgba)
    assert out["timings_ms"]["tiff"] > 0.0 and out["depth_tiff"]["sections"] == tuple(sections)
