"""cvhip_surface_subset through the C++ host layer (cybervision_amd/csrc/host/cvhip_host.hpp, mesh::surface_subset) on a real
GPU: a g++-built program takes the subset of a surface; rows, points and track rows must equal the ctypes path byte for byte."""
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

from cybervision_amd import triangulation

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_cpp_host_subset(gpu_device, tmp_path):
    exe = tmp_path / "host_subset"
    lib_dir = ROOT / "cybervision_amd"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", str(exe), str(ROOT / "tests" / "cpp" / "host_subset.cpp"),
                           f"-L{lib_dir}", "-lcvhip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    n, cameras, max_points, seed = 3 * triangulation.SUBSET_WG_ROWS + 41, 3, 1500, 12345678901234567
    rng = np.random.default_rng(4)
    points = rng.standard_normal((n, 3))
    tracks = rng.integers(-1, 2048, size=(n, cameras, 2), dtype=np.int32)
    points.tofile(tmp_path / "points.bin")
    tracks.tofile(tmp_path / "tracks.bin")
    res = subprocess.run([str(exe), str(tmp_path), str(cameras), str(max_points), str(seed)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    info = json.loads(res.stdout.strip().splitlines()[-1])
    cams = [triangulation.Camera(np.zeros(3), np.zeros(3), np.zeros((3, 4))) for _ in range(cameras)]
    surface = triangulation.Surface(points=points, track_index=np.arange(n, dtype=np.int64), tracks=tracks, cameras=cams)
    want, want_info = triangulation.subset(gpu_device, surface, max_points, seed=seed)
    assert info == {"rows_in": n, "rows_out": max_points, "cameras": cameras}
    assert np.fromfile(tmp_path / "out_rows.bin", dtype=np.uint64).tobytes() == want_info["rows"].tobytes()
    assert np.fromfile(tmp_path / "out_points.bin", dtype=np.float64).tobytes() == want.points.tobytes()
    assert np.fromfile(tmp_path / "out_tracks.bin", dtype=np.int32).tobytes() == want.tracks.tobytes()
    assert len(want.points) == max_points
