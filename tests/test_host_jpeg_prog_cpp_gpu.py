"""The progressive JPEG decoder through the C++ host layer (cybervision_amd/csrc/host/cvhip_host.hpp, namespace image:
jpeg_progressive_info, jpeg_progressive_decode) on a real GPU: a g++-built program decodes two scenes; the pixels must equal
tests/ref_jpeg_prog.py's byte for byte."""
import json
import subprocess
from pathlib import Path

import pytest

import jpeg_prog_scenes
import ref_jpeg_prog

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_cpp_host_jpeg_progressive(gpu_device, tmp_path):
    exe = tmp_path / "host_jpeg_prog"
    lib_dir = ROOT / "cybervision_amd"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", str(exe), str(ROOT / "tests" / "cpp" / "host_jpeg_prog.cpp"),
                           f"-L{lib_dir}", "-lcvhip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    for name, drop in (("q_exif", 3), ("p_refine_444", 0)):
        data = jpeg_prog_scenes.scene(name)
        want = jpeg_prog_scenes.restated(name)
        (tmp_path / "in.jpg").write_bytes(data)
        res = subprocess.run([str(exe), str(tmp_path / "in.jpg"), str(drop), str(tmp_path / "luma.bin"), str(tmp_path / "rgb.bin")],
                             capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stderr
        info = json.loads(res.stdout.strip().splitlines()[-1])
        h, w = want["luma"].shape
        assert (tmp_path / "luma.bin").read_bytes() == want["luma"][:h - drop].tobytes(), name
        assert (tmp_path / "rgb.bin").read_bytes() == want["rgb"][:h - drop].tobytes(), name
        ref = ref_jpeg_prog.info(data)
        assert {k: info[k] for k in ("width", "height", "components", "h", "v", "scans")} == {k: ref[k] for k in ("width", "height", "components", "h", "v", "scans")}
        assert info["focal"] == ref["focal_length_35mm"] == jpeg_prog_scenes.FOCAL.get(name, 0)
