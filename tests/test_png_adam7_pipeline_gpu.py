"""The pipelines from Adam7 interlaced PNG FILES (reconstruction.reconstruct_perspective_files / reconstruct_affine_files
through image.load): an affine pair written as 16-bit grey Adam7 files gives what the run on the restated
arrays gives; config 5's three views at 512^2, one of them an Adam7 RGB file with an eXIf focal length, give the surface,
mesh and PLY of the run on the decoded arrays.  Same inputs, same code downstream, so every comparison is equality.
(ref_png_in's inflate is pure Python; for these pictures zlib.decompress, which tests/test_png_in_ref.py pins it to, stands in.)"""
import io
import zlib

import numpy as np
import pytest

import png_adam7_scenes
import png_in_scenes
import ref_jpeg
import ref_png_adam7
from cybervision_amd import correlation, image, mesh, reconstruction, synth
from cybervision_amd.fundamentalmatrix import ProjectionMode

pytestmark = pytest.mark.gpu
SIZE = 512  # (the size at which tests/test_png_in_pipeline_gpu.py reconstructs config 5's scene)


def _restate(data):
    out = ref_png_adam7.decode(data, inflater=zlib.decompress, fast=True)
    return out["luma"], out["rgb"]


def _equal(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes() and np.asarray(a).shape == np.asarray(b).shape


def test_affine_files_give_what_the_decoded_arrays_give(gpu_device, tmp_path):
    W, H, SEED = 200, 150, 0   # (the pair of tests/test_png_in_pipeline_gpu.py)
    a, b, _ = synth.make_pair(W, H, seed=7)
    paths, restated = [], []
    for i, v in enumerate((a, b)):
        samples = (np.asarray(v, dtype=np.uint8).astype(np.int64) * 257)[:, :, None]   # (v * 257 + 128) / 257 = v
        paths.append(tmp_path / ("sem%d.png" % i))
        paths[-1].write_bytes(png_adam7_scenes.adam7_png(samples, 16, 0, (4, 1, 2, 3, 0)))
        assert image.png_ext_info(paths[-1].read_bytes())["interlace"] == 1
        restated.append(_restate(paths[-1].read_bytes()))
        assert _equal(restated[-1][0], np.asarray(v, dtype=np.uint8))
    got = reconstruction.reconstruct_affine_files(gpu_device, paths[0], paths[1], seed=SEED, project_to_image=0, depth_scale=-0.5)
    steps = correlation.optimal_scale_steps(W, H)
    pyramids = [correlation.lanczos_pyramid(gpu_device, luma, steps) for luma, _rgb in restated]
    pair = reconstruction.reconstruct_pairs(gpu_device, pyramids, ProjectionMode.Affine, dense=False, seed=SEED)["pairs"][(0, 1)]
    assert pair["f"] is not None
    want = reconstruction.reconstruct_affine_mesh(gpu_device, pyramids[0], pyramids[1], pair["f"], project_to_image=0, depth_scale=-0.5,
                                                  out_scale=(1.0, 1.0, -0.5))
    assert len(want["surface"].points) > 100 and len(want["mesh"]["polygons"]) > 100
    assert _equal(got["f"], pair["f"])
    assert _equal(got["surface"].points, want["surface"].points) and _equal(got["surface"].tracks, want["surface"].tracks)
    assert _equal(got["mesh"]["polygons"], want["mesh"]["polygons"]) and _equal(got["mesh"]["camera"], want["mesh"]["camera"])
    assert _equal(got["depth_image"]["map"], want["depth_image"]["map"])
    assert got["relative_tilt_angle"] is None and [s.databar_height for s in got["source_images"]] == [0, 0]


def test_perspective_files_give_what_the_decoded_arrays_give(gpu_device, tmp_path):
    from PIL import Image

    pictures, K, _ = synth.make_sfm_views(SIZE)
    focal = int(round(K[0, 0] * np.sqrt(24.0 ** 2 + 36.0 ** 2) / np.sqrt(2.0 * SIZE * SIZE)))
    exif = (png_in_scenes.chunk(b"eXIf", png_in_scenes.exif_block(focal, short=True, order=">")),)
    paths = []
    for i, v in enumerate(pictures):
        v = np.asarray(v, dtype=np.uint8)
        rgb = np.ascontiguousarray(np.stack([v, 255 - v, v // 2 + 60], axis=2))
        if i == 1:   # the interlaced view, zlib's own choice of blocks, a filter cycle per pass
            data = png_adam7_scenes.adam7_png(rgb.astype(np.int64), 8, 2, png_adam7_scenes.rotated, exif)
        else:
            buf = io.BytesIO()
            Image.fromarray(rgb).save(buf, "PNG")
            data = buf.getvalue()
            at = data.index(b"IDAT") - 4
            data = data[:at] + exif[0] + data[at:]
        paths.append(tmp_path / ("view%d.png" % i))
        paths[-1].write_bytes(data)
    assert [image.png_ext_info(p.read_bytes())["interlace"] for p in paths] == [0, 1, 0]
    restated = [_restate(p.read_bytes()) for p in paths]
    for p, (luma, rgb) in zip(paths, restated):
        src = image.load(gpu_device, p, rgb=True)
        assert _equal(src.img, luma) and _equal(src.rgb, rgb) and src.focal_length_35mm == focal
    Color = mesh.VertexMode.Color
    kw = dict(triangulate=mesh.delaunay_device(gpu_device), project_to_image=0, bundle_adjustment=False, seed=3, vertex_mode=Color)
    got = reconstruction.reconstruct_perspective_files(gpu_device, paths, ply_path=str(tmp_path / "files.ply"), **kw)
    Ks = np.stack([ref_jpeg.calibration_matrix(SIZE, SIZE, focal)] * 3)
    steps = correlation.optimal_scale_steps(SIZE, SIZE)
    pyramids = [correlation.lanczos_pyramid(gpu_device, luma, steps) for luma, _rgb in restated]
    want = reconstruction.reconstruct_perspective_mesh(gpu_device, pyramids, Ks, ply_path=str(tmp_path / "arrays.ply"),
                                                       images=[rgb for _luma, rgb in restated], **kw)
    assert len(want["surface"].cameras) >= 2 and len(want["mesh"]["polygons"]) > 1000
    assert _equal(got["K"], Ks) and got["camera_order"] == want["camera_order"]
    assert _equal(got["surface"].points, want["surface"].points) and _equal(got["surface"].tracks, want["surface"].tracks)
    assert len(got["surface"].cameras) == len(want["surface"].cameras)
    for a, b in zip(got["surface"].cameras, want["surface"].cameras):
        assert _equal(a.projection, b.projection) and _equal(a.r, b.r) and _equal(a.t, b.t)
    assert _equal(got["mesh"]["polygons"], want["mesh"]["polygons"]) and _equal(got["mesh"]["camera"], want["mesh"]["camera"])
    assert _equal(got["depth_image"]["map"], want["depth_image"]["map"])
    assert (tmp_path / "files.ply").read_bytes() == (tmp_path / "arrays.ply").read_bytes()
