"""The perspective pipeline from JPEG FILES (reconstruction.reconstruct_perspective_files): config 5's three
views written as JPEG files with an EXIF focal length must give exactly what reconstruct_perspective_mesh gives on the
pixels tests/ref_jpeg.py decodes from the same files, with ref_jpeg.calibration_matrix's K: same inputs, same code
downstream, so every comparison is equality."""
import numpy as np
import pytest

import jpeg_scenes
import ref_jpeg
from cybervision_amd import correlation, image, mesh, reconstruction, synth

pytestmark = pytest.mark.gpu
SIZE = 512  # (the size at which tests/test_png_pipeline_gpu.py reconstructs config 5's scene)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """The three views as colour JPEG files at 4:2:0 and quality 95, with the focal length that is nearest to the scene's K."""
    views, K, _ = synth.make_sfm_views(SIZE)
    focal = int(round(K[0, 0] * np.sqrt(24.0 ** 2 + 36.0 ** 2) / np.sqrt(2.0 * SIZE * SIZE)))
    folder = tmp_path_factory.mktemp("jpeg_views")
    paths = []
    for i, v in enumerate(views):
        v = np.asarray(v, dtype=np.uint8)
        rgb = np.stack([v, 255 - v, v // 2 + 60], axis=2)
        paths.append(folder / ("view%d.jpg" % i))
        paths[-1].write_bytes(jpeg_scenes.pillow_jpeg(rgb, quality=95, subsampling=2, exif=b"Exif\0\0" + jpeg_scenes.exif_bytes(focal)))
    return paths, focal


@pytest.fixture(scope="module")
def restated(files):
    paths, _focal = files
    return [(ref_jpeg.decode(p.read_bytes(), ref_jpeg.LUMA8), ref_jpeg.decode(p.read_bytes(), ref_jpeg.RGB8)) for p in paths]


def _equal(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes() and np.asarray(a).shape == np.asarray(b).shape


def test_load_is_the_restated_image(gpu_device, files, restated):
    paths, focal = files
    for p, (luma, rgb) in zip(paths, restated):
        src = image.load(gpu_device, p, rgb=True)
        assert _equal(src.img, luma) and _equal(src.rgb, rgb) and src.focal_length_35mm == focal and src.filename == str(p)
        assert _equal(src.calibration_matrix(), ref_jpeg.calibration_matrix(SIZE, SIZE, focal))
        assert _equal(src.calibration_matrix(50), ref_jpeg.calibration_matrix(SIZE, SIZE, 50))   # the argument overrides the file's
        dropped = image.load(gpu_device, p, drop_rows=12, out="device")
        assert _equal(dropped.img.cpu().numpy(), luma[:SIZE - 12]) and dropped.rgb is None
        assert _equal(dropped.calibration_matrix(), ref_jpeg.calibration_matrix(SIZE, SIZE - 12, focal))
    assert _equal(image.calibration_matrix(640, 480, None), ref_jpeg.calibration_matrix(640, 480, None))   # no focal length: 1


def test_files_give_what_the_decoded_arrays_give(gpu_device, files, restated, tmp_path):
    paths, focal = files
    Color = mesh.VertexMode.Color
    kw = dict(triangulate=mesh.delaunay_device(gpu_device), project_to_image=0, bundle_adjustment=False, seed=3, vertex_mode=Color)
    got = reconstruction.reconstruct_perspective_files(gpu_device, paths, ply_path=str(tmp_path / "files.ply"), **kw)
    K = np.stack([ref_jpeg.calibration_matrix(SIZE, SIZE, focal)] * 3)
    steps = correlation.optimal_scale_steps(SIZE, SIZE)
    pyramids = [correlation.lanczos_pyramid(gpu_device, luma, steps) for luma, _rgb in restated]
    want = reconstruction.reconstruct_perspective_mesh(gpu_device, pyramids, K, ply_path=str(tmp_path / "arrays.ply"),
                                                       images=[rgb for _luma, rgb in restated], **kw)
    assert len(want["surface"].cameras) >= 2 and len(want["mesh"]["polygons"]) > 1000
    assert _equal(got["K"], K) and got["timings_ms"]["decode"] > 0.0 and "decode" not in want["timings_ms"]
    assert got["camera_order"] == want["camera_order"]
    assert _equal(got["surface"].points, want["surface"].points) and _equal(got["surface"].tracks, want["surface"].tracks)
    assert len(got["surface"].cameras) == len(want["surface"].cameras)
    for a, b in zip(got["surface"].cameras, want["surface"].cameras):
        assert _equal(a.projection, b.projection) and _equal(a.r, b.r) and _equal(a.t, b.t)
    assert _equal(got["mesh"]["polygons"], want["mesh"]["polygons"]) and _equal(got["mesh"]["camera"], want["mesh"]["camera"])
    assert _equal(got["depth_image"]["map"], want["depth_image"]["map"])
    # the Color-mode PLY without images=: the files' decoded RGB was passed
    assert (tmp_path / "files.ply").read_bytes() == (tmp_path / "arrays.ply").read_bytes()
    assert got["ply_sections"] == want["ply_sections"]
    # the argument overrides the EXIF value; mesh=False stops at the surface; host arrays give the same
    other = reconstruction.reconstruct_perspective_files(gpu_device, paths, focal_length_35mm=focal, mesh=False, on_device=False,
                                                         bundle_adjustment=False, seed=3)
    assert "mesh" not in other and _equal(other["K"], K) and _equal(other["surface"].points, want["surface"].points)
