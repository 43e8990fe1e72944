"""The PNG encoder through the C++ host layer (cybervision_amd/csrc/host/cvhip_host.hpp, namespace mesh: png_encode) on a
real GPU: a g++-built program writes the file of the adaptive scene; it must equal tests/ref_png.py byte for byte."""
import json
import subprocess
from pathlib import Path

import pytest

import png_scenes

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_cpp_host_png(gpu_device, tmp_path):
    exe = tmp_path / "host_png"
    lib_dir = ROOT / "cybervision_amd"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", str(exe), str(ROOT / "tests" / "cpp" / "host_png.cpp"),
                           f"-L{lib_dir}", "-lcvhip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    pixels, kind = png_scenes.scenes()["adaptive"]
    want = png_scenes.restated("adaptive")
    pixels.tofile(tmp_path / "pixels.bin")
    h, w, c = pixels.shape
    res = subprocess.run([str(exe), str(tmp_path / "pixels.bin"), str(w), str(h), str(c), str(kind), str(tmp_path / "out.png")],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    info = json.loads(res.stdout.strip().splitlines()[-1])
    assert (tmp_path / "out.png").read_bytes() == want["file"]
    assert info == {"size": len(want["file"]), "sections": list(want["sections"])}
