"""Deflate and tiled TIFF files through the layers above the decoder: image.load, the affine pipeline from an
SEM pair's two FILES (reconstruction.reconstruct_affine_files), and the C++ host layer.  The pair is
tests/test_tiff_pipeline_gpu.py's - synth.make_pair(200, 150, seed=7) with 12 databar rows and the microscope's text block -
written twice: as tiled Deflate files with Predictor 2, and as uncompressed strip files of the same pixels.  Same pixels, same
code downstream, so every comparison is equality."""
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ref_tiff_ext
import tiff_ext_scenes
import tiff_scenes
from cybervision_amd import image, reconstruction, synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
W, H, BAR, SEED = 200, 150, 12, 0
SEM_1 = ("[Scan]\r\nPixelWidth=2.5e-9\r\nPixelHeight=5e-9\r\n[Stage]\r\nStageT=0\r\n[PrivateFei]\r\nDatabarHeight=%d\r\n" % BAR).encode()
SEM_2 = b"[Stage]\nStageT=10\n\0"


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """(the tiled Deflate pair, the uncompressed strip pair): image 1 in 8 bits and tiles of 64 x 32 with 12 databar rows and the
    whole SEM block; image 2 in 16 big-endian bits (v * 257) and tiles of 16 x 16 with a tilt angle only, code 32946."""
    a, b, _ = synth.make_pair(W, H, seed=7)
    a, b = np.asarray(a, dtype=np.uint8), np.asarray(b, dtype=np.uint8)
    bar = np.tile((np.arange(W) * 7 % 256).astype(np.uint8), (BAR, 1))
    one, two = np.concatenate([a, bar])[:, :, None], (b.astype(np.uint16) * 257)[:, :, None]
    e1, e2 = [(34682, tiff_scenes.ASCII, SEM_1)], [(34682, tiff_scenes.ASCII, SEM_2)]
    folder = tmp_path_factory.mktemp("sem_pair_ext")
    paths = [folder / n for n in ("tiled1.tif", "tiled2.tif", "strip1.tif", "strip2.tif")]
    paths[0].write_bytes(tiff_ext_scenes.write_tiles(one, 64, 32, compression=8, predictor=2, extra=e1, exif_focal=35))
    paths[1].write_bytes(tiff_ext_scenes.write_tiles(two, 16, 16, ">", compression=32946, predictor=2, extra=e2))
    paths[2].write_bytes(tiff_scenes.write(one, rps=16, extra=e1, exif_focal=35))
    paths[3].write_bytes(tiff_scenes.write(two, ">", rps=16, extra=e2))
    return paths[:2], paths[2:], (a, b)


def _equal(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes() and np.asarray(a).shape == np.asarray(b).shape


def test_load_takes_the_new_path(gpu_device, files):
    tiled, strip, (a, b) = files
    for k, pixels in enumerate((a, b)):
        assert image._tiff_is_ext(tiled[k].read_bytes()) and not image._tiff_is_ext(strip[k].read_bytes())
        with pytest.raises(Exception) as raised:
            image.tiff_info(tiled[k].read_bytes())
        assert raised.value.code == -3
        got, want = image.load(gpu_device, tiled[k], rgb=True), image.load(gpu_device, strip[k], rgb=True)
        assert _equal(got.img, pixels) and _equal(got.img, want.img) and _equal(got.rgb, want.rgb) and got.filename == str(tiled[k])
        assert (got.scale, got.tilt_angle, got.databar_height, got.focal_length_35mm) == (want.scale, want.tilt_angle, want.databar_height, want.focal_length_35mm)
        assert _equal(got.img, ref_tiff_ext.decode(tiled[k].read_bytes(), ref_tiff_ext.LUMA8, ref_tiff_ext.DROP_DATABAR))
    one = image.load(gpu_device, tiled[0])
    assert one.scale == (float(np.float32(2.5e-9)), float(np.float32(5e-9))) and one.tilt_angle == 0.0 and one.databar_height == BAR
    assert one.focal_length_35mm == 35 and one.rgb is None
    two = image.load(gpu_device, tiled[1], out="device")
    assert _equal(two.img.cpu().numpy(), b) and two.tilt_angle == 10.0 and two.databar_height == 0
    whole = image.load(gpu_device, tiled[0], drop_rows=0)
    assert whole.img.shape == (H + BAR, W) and _equal(whole.img[:H], a) and whole.databar_height == 0


def test_files_give_what_the_strip_files_give(gpu_device, files):
    tiled, strip, _ = files
    want = reconstruction.reconstruct_affine_files(gpu_device, strip[0], strip[1], seed=SEED, project_to_image=0, depth_scale=-0.5)
    got = reconstruction.reconstruct_affine_files(gpu_device, tiled[0], tiled[1], seed=SEED, project_to_image=0, depth_scale=-0.5)
    assert len(want["surface"].points) > 100 and len(want["mesh"]["polygons"]) > 100   # (a surface, not an empty result)
    assert _equal(got["f"], want["f"]) and _equal(got["surface"].points, want["surface"].points) and _equal(got["surface"].tracks, want["surface"].tracks)
    assert _equal(got["mesh"]["polygons"], want["mesh"]["polygons"]) and _equal(got["depth_image"]["map"], want["depth_image"]["map"])
    assert got["relative_tilt_angle"] == want["relative_tilt_angle"] == 10.0
    assert [s.databar_height for s in got["source_images"]] == [BAR, 0]


def test_cpp_host_tiff_ext(gpu_device, tmp_path):
    exe = tmp_path / "host_tiff_ext"
    lib_dir = ROOT / "cybervision_amd"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", str(exe), str(ROOT / "tests" / "cpp" / "host_tiff_ext.cpp"),
                           f"-L{lib_dir}", "-lcvhip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    for name, drop in (("t_sem", -1), ("s_mm_g16_pred", 3)):
        data = tiff_ext_scenes.scene(name)
        ref = ref_tiff_ext.info(data)
        rows = ref["height"] - (ref["databar_height"] if drop < 0 else drop)
        (tmp_path / "in.tif").write_bytes(data)
        res = subprocess.run([str(exe), str(tmp_path / "in.tif"), str(drop), str(tmp_path / "luma.bin"), str(tmp_path / "rgb.bin")],
                             capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stderr
        info = json.loads(res.stdout.strip().splitlines()[-1])
        assert (tmp_path / "luma.bin").read_bytes() == ref_tiff_ext.decode(data, ref_tiff_ext.LUMA8)[:rows].tobytes(), name
        assert (tmp_path / "rgb.bin").read_bytes() == ref_tiff_ext.decode(data, ref_tiff_ext.RGB8)[:rows].tobytes(), name
        keys = ("width", "height", "samples", "bits", "compression", "photometric", "predictor", "strips", "rows_per_strip", "sem", "tile_width",
                "tile_length", "tiles_across")
        assert {k: info[k] for k in keys} == {k: ref[k] for k in keys}
        assert info["focal"] == (ref["focal_length_35mm"] or 0) and info["databar"] == ref["databar_height"]
        assert info["scale"] == [int(np.float32(v).view(np.uint32)) for v in ref["scale"]]
        assert info["has_tilt"] == (ref["tilt_angle"] is not None)
