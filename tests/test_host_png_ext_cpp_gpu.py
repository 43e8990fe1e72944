"""The PNG decoder that reads Adam7 files too, through the C++ host layer (cybervision_amd/csrc/host/cvhip_host.hpp,
namespace image: png_ext_info, png_ext_decode, calibration_matrix) on a real GPU: a g++-built program decodes two interlaced
scenes and one that is not; the pixels must equal tests/ref_png_adam7.py's byte for byte, the matrix ref_jpeg's f64 values."""
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import png_adam7_scenes
import png_in_scenes
import ref_jpeg
import ref_png_adam7

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_cpp_host_png_ext(gpu_device, tmp_path):
    exe = tmp_path / "host_png_ext"
    lib_dir = ROOT / "cybervision_amd"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", str(exe), str(ROOT / "tests" / "cpp" / "host_png_ext.cpp"),
                           f"-L{lib_dir}", "-lcvhip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    cases = (("x_exif", 2, png_adam7_scenes.scene("x_exif"), png_adam7_scenes.FOCAL, -3),
             ("k_pal_d2_17x9", 0, png_adam7_scenes.scene("k_pal_d2_17x9"), 0, -3),
             ("x_long_be", 1, png_in_scenes.scene("x_long_be"), png_in_scenes.FOCAL["x_long_be"], 0))
    for name, drop, data, focal, old_code in cases:
        want = ref_png_adam7.decode(data, fast=True)
        (tmp_path / "in.png").write_bytes(data)
        res = subprocess.run([str(exe), str(tmp_path / "in.png"), str(drop), str(tmp_path / "luma.bin"), str(tmp_path / "rgb.bin")],
                             capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stderr
        got = json.loads(res.stdout.strip().splitlines()[-1])
        h, w = want["luma"].shape
        assert (tmp_path / "luma.bin").read_bytes() == want["luma"][:h - drop].tobytes(), name
        assert (tmp_path / "rgb.bin").read_bytes() == want["rgb"][:h - drop].tobytes(), name
        info = ref_png_adam7.info(data)
        assert tuple(got["info"]) == info and info[6] == focal and got["old_code"] == old_code, name
        assert np.array(got["k"]).tobytes() == ref_jpeg.calibration_matrix(w, h - drop, info[6] or None).tobytes()
