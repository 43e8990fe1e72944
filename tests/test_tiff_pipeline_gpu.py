"""The affine pipeline from an SEM pair's two FILES (reconstruction.reconstruct_affine_files): a small affine
pair written as TIFF files with the microscope's text block must give exactly what reconstruct_pairs' sparse stage plus
reconstruct_affine_mesh give on the pixels tests/ref_tiff.py decodes from the same files: same inputs, same code downstream,
so every comparison is equality.  The pair is synth.make_pair(200, 150, seed=7), the size at which
tests/test_delaunay_lattice_gpu.py::test_reconstruct_affine_mesh runs; the affine sparse stage finds an F on it with seed 0."""
import numpy as np
import pytest

import ref_tiff
import tiff_scenes
from cybervision_amd import correlation, image, mesh, reconstruction, synth
from cybervision_amd.fundamentalmatrix import ProjectionMode

pytestmark = pytest.mark.gpu
W, H, BAR, SEED = 200, 150, 12, 0
SEM_1 = ("[Scan]\r\nPixelWidth=2.5e-9\r\nPixelHeight=5e-9\r\n[Stage]\r\nStageT=0\r\n[PrivateFei]\r\nDatabarHeight=%d\r\n" % BAR)
SEM_2 = b"[Stage]\nStageT=10\n\0"


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Image 1: an 8-bit LZW file of libtiff's with 12 databar rows below the image and the whole SEM block; image 2: a 16-bit
    big-endian uncompressed file whose samples are v * 257, with a tilt angle only."""
    a, b, _ = synth.make_pair(W, H, seed=7)
    a, b = np.asarray(a, dtype=np.uint8), np.asarray(b, dtype=np.uint8)
    bar = np.tile((np.arange(W) * 7 % 256).astype(np.uint8), (BAR, 1))
    folder = tmp_path_factory.mktemp("sem_pair")
    p1, p2 = folder / "sem1.tif", folder / "sem2.tif"
    p1.write_bytes(tiff_scenes.pillow(np.concatenate([a, bar]), "tiff_lzw", sem=SEM_1))
    p2.write_bytes(tiff_scenes.write((b.astype(np.uint16) * 257)[:, :, None], ">", rps=16, extra=[(34682, tiff_scenes.ASCII, SEM_2)]))
    return (p1, p2), (a, b)


@pytest.fixture(scope="module")
def restated(files):
    (p1, p2), _ = files
    return [(ref_tiff.decode(p.read_bytes(), ref_tiff.LUMA8, ref_tiff.DROP_DATABAR), ref_tiff.decode(p.read_bytes(), ref_tiff.RGB8, ref_tiff.DROP_DATABAR))
            for p in (p1, p2)]


def _equal(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes() and np.asarray(a).shape == np.asarray(b).shape


def test_load_is_the_restated_image(gpu_device, files, restated):
    (p1, p2), (a, b) = files
    assert _equal(restated[0][0], a) and _equal(restated[1][0], b)   # the databar is cut; (v * 257 + 128) / 257 = v
    one = image.load(gpu_device, p1, rgb=True)
    assert _equal(one.img, restated[0][0]) and _equal(one.rgb, restated[0][1]) and one.filename == str(p1)
    assert one.scale == (float(np.float32(2.5e-9)), float(np.float32(5e-9))) and one.tilt_angle == 0.0 and one.databar_height == BAR
    assert one.focal_length_35mm is None
    assert _equal(one.calibration_matrix(), image.calibration_matrix(W, H, None))
    two = image.load(gpu_device, p2, out="device")
    assert _equal(two.img.cpu().numpy(), restated[1][0]) and two.rgb is None
    assert two.scale == (1.0, 1.0) and two.tilt_angle == 10.0 and two.databar_height == 0 and two.focal_length_35mm is None
    # drop_rows given: it overrides the file's databar height
    whole = image.load(gpu_device, p1, drop_rows=0)
    assert whole.img.shape == (H + BAR, W) and _equal(whole.img[:H], a) and whole.databar_height == 0
    # four-argument construction keeps working
    plain = image.SourceImage(a, None, None, "x")
    assert plain.scale == (1.0, 1.0) and plain.tilt_angle is None and plain.databar_height == 0


def test_load_of_a_jpeg_is_unchanged(gpu_device, tmp_path):
    import jpeg_scenes
    import ref_jpeg

    data = jpeg_scenes.scene("e_exif")
    (tmp_path / "in.jpg").write_bytes(data)
    luma, rgb = ref_jpeg.decode(data, ref_jpeg.LUMA8), ref_jpeg.decode(data, ref_jpeg.RGB8)
    src = image.load(gpu_device, tmp_path / "in.jpg", rgb=True)
    assert _equal(src.img, luma) and _equal(src.rgb, rgb) and src.focal_length_35mm == ref_jpeg.info(data)["focal_length_35mm"] is not None
    assert src.scale == (1.0, 1.0) and src.tilt_angle is None and src.databar_height == 0
    assert _equal(image.load(gpu_device, tmp_path / "in.jpg", drop_rows=2).img, luma[:-2])
    (tmp_path / "no.bin").write_bytes(b"II+\0 not an image")   # neither: the JPEG path's error
    with pytest.raises(Exception) as raised:
        image.load(gpu_device, tmp_path / "no.bin")
    assert raised.value.code == -1


def test_files_give_what_the_decoded_arrays_give(gpu_device, files, restated, tmp_path):
    (p1, p2), _ = files
    Color = mesh.VertexMode.Color
    got = reconstruction.reconstruct_affine_files(gpu_device, p1, p2, seed=SEED, project_to_image=0, ply_path=str(tmp_path / "files.ply"),
                                                  vertex_mode=Color, depth_scale=-0.5)
    steps = correlation.optimal_scale_steps(W, H)
    pyramids = [correlation.lanczos_pyramid(gpu_device, luma, steps) for luma, _rgb in restated]
    pair = reconstruction.reconstruct_pairs(gpu_device, pyramids, ProjectionMode.Affine, dense=False, seed=SEED)["pairs"][(0, 1)]
    assert pair["f"] is not None
    want = reconstruction.reconstruct_affine_mesh(gpu_device, pyramids[0], pyramids[1], pair["f"], project_to_image=0, depth_scale=-0.5,
                                                  ply_path=str(tmp_path / "arrays.ply"), images=[rgb for _luma, rgb in restated],
                                                  vertex_mode=Color, out_scale=(1.0, 1.0, -0.5))

    def same_result(x):
        assert _equal(x["surface"].points, want["surface"].points) and _equal(x["surface"].tracks, want["surface"].tracks)
        assert _equal(x["mesh"]["polygons"], want["mesh"]["polygons"]) and _equal(x["mesh"]["camera"], want["mesh"]["camera"])
        assert _equal(x["depth_image"]["map"], want["depth_image"]["map"])
        return True

    assert len(want["surface"].points) > 100 and len(want["mesh"]["polygons"]) > 100   # (a surface, not an empty result)
    assert _equal(got["f"], pair["f"]) and same_result(got)
    assert (tmp_path / "files.ply").read_bytes() == (tmp_path / "arrays.ply").read_bytes() and got["ply_sections"] == want["ply_sections"]
    assert got["relative_tilt_angle"] == 10.0 and got["timings_ms"]["decode"] > 0.0 and "decode" not in want["timings_ms"]
    assert [s.databar_height for s in got["source_images"]] == [BAR, 0] and got["source_images"][0].scale != (1.0, 1.0)
    # with f= given the sparse stage is skipped; host arrays give the same
    other = reconstruction.reconstruct_affine_files(gpu_device, p1, p2, f=pair["f"], on_device=False, project_to_image=0, depth_scale=-0.5)
    assert same_result(other) and _equal(other["f"], pair["f"]) and other["relative_tilt_angle"] == 10.0
    # one file without a tilt angle: no relative angle
    p3 = tmp_path / "plain.tif"
    p3.write_bytes(tiff_scenes.write(restated[1][0][:, :, None]))
    assert reconstruction.reconstruct_affine_files(gpu_device, p1, p3, f=pair["f"])["relative_tilt_angle"] is None
