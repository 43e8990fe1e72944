"""The TIFF decoder through the C++ host layer (cybervision_amd/csrc/host/cvhip_host.hpp, namespace image: tiff_info,
tiff_decode) on a real GPU: a g++-built program decodes two scenes; the pixels must equal tests/ref_tiff.py's byte for
byte, the metadata its values."""
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ref_tiff
import tiff_scenes

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_cpp_host_tiff(gpu_device, tmp_path):
    exe = tmp_path / "host_tiff"
    lib_dir = ROOT / "cybervision_amd"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", str(exe), str(ROOT / "tests" / "cpp" / "host_tiff.cpp"),
                           f"-L{lib_dir}", "-lcvhip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    for name, drop in (("o_sem_exif", -1), ("o_pred_g16_mm_lzw", 3)):
        data = tiff_scenes.scene(name)
        ref = ref_tiff.info(data)
        rows = ref["height"] - (ref["databar_height"] if drop < 0 else drop)
        (tmp_path / "in.tif").write_bytes(data)
        res = subprocess.run([str(exe), str(tmp_path / "in.tif"), str(drop), str(tmp_path / "luma.bin"), str(tmp_path / "rgb.bin")],
                             capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stderr
        info = json.loads(res.stdout.strip().splitlines()[-1])
        assert (tmp_path / "luma.bin").read_bytes() == ref_tiff.decode(data, ref_tiff.LUMA8)[:rows].tobytes(), name
        assert (tmp_path / "rgb.bin").read_bytes() == ref_tiff.decode(data, ref_tiff.RGB8)[:rows].tobytes(), name
        keys = ("width", "height", "samples", "bits", "compression", "photometric", "predictor", "strips", "rows_per_strip", "sem")
        assert {k: info[k] for k in keys} == {k: ref[k] for k in keys}
        assert info["focal"] == (ref["focal_length_35mm"] or 0) and info["databar"] == ref["databar_height"]
        assert info["scale"] == [int(np.float32(v).view(np.uint32)) for v in ref["scale"]]
        assert info["has_tilt"] == (ref["tilt_angle"] is not None)
        if ref["tilt_angle"] is not None:
            assert info["tilt"] == int(np.float32(ref["tilt_angle"]).view(np.uint32))
    assert ref_tiff.info(tiff_scenes.scene("o_sem_exif"))["databar_height"] == 5
