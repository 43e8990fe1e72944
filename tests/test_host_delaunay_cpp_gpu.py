"""cvhip_mesh_delaunay through the C++ host layer (cybervision_amd/csrc/host/cvhip_host.hpp, mesh::delaunay) on a real GPU:
a g++-built program triangulates camera 0's points of a scene of tests/mesh_scenes.py; the faces must equal the ctypes
path byte for byte."""
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mesh_scenes
import ref_mesh
from cybervision_amd import mesh

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_cpp_host_delaunay(gpu_device, tmp_path):
    exe = tmp_path / "host_delaunay"
    lib_dir = ROOT / "cybervision_amd"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", str(exe), str(ROOT / "tests" / "cpp" / "host_delaunay.cpp"),
                           f"-L{lib_dir}", "-lcvhip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    _, xy = ref_mesh.camera_points(mesh_scenes.scene(3).surface, 0)
    np.ascontiguousarray(xy, dtype=np.float64).tofile(tmp_path / "xy.bin")
    res = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    info = json.loads(res.stdout.strip().splitlines()[-1])
    want = mesh.delaunay(gpu_device, xy)
    got = np.fromfile(tmp_path / "faces.bin", dtype=np.uint32).reshape(-1, 3)
    assert info["points"] == len(xy) and info["faces"] == len(got) == len(want) > 5000
    assert got.tobytes() == want.tobytes()
