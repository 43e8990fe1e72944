"""The mesh stage through the C++ host layer (cybervision_amd/csrc/host/cvhip_host.hpp, namespace mesh) on a real GPU: a
g++-built program runs Mesh::create and depth_image on a scene of tests/mesh_scenes.py with the lattice split as its
Delaunay; the polygon list, its cameras and the depth map must equal the ctypes path bit for bit."""
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


def test_cpp_host_mesh(gpu_device, tmp_path):
    exe = tmp_path / "host_mesh"
    lib_dir = ROOT / "cybervision_amd"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", str(exe), str(ROOT / "tests" / "cpp" / "host_mesh.cpp"),
                           f"-L{lib_dir}", "-lcvhip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    m = 3
    s = mesh_scenes.scene(m)
    dev_surface = mesh_scenes.device_surface(s)
    s.surface.points.tofile(tmp_path / "points.bin")
    s.surface.tracks.tofile(tmp_path / "tracks.bin")
    np.concatenate([np.concatenate([c.projection.reshape(12), c.r, c.t]) for c in dev_surface.cameras]).tofile(tmp_path / "cameras.bin")
    np.asarray(s.image_dims, dtype=np.uint32).tofile(tmp_path / "dims.bin")
    tri = [mesh_scenes.lattice_triangulate(s, i) for i in range(m)]
    for i in range(m):
        idx, xy = ref_mesh.camera_points(s.surface, i)
        tri[i](xy).astype(np.uint32).tofile(tmp_path / f"faces{i}.bin")
    res = subprocess.run([str(exe), str(tmp_path), str(len(s.surface.points)), str(m)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    info = json.loads(res.stdout.strip().splitlines()[-1])
    calls = iter(tri)
    want = mesh.create(gpu_device, dev_surface, s.image_dims, lambda xy: next(calls)(xy))
    polys = np.fromfile(tmp_path / "polygons.bin", dtype=np.uint32).reshape(-1, 3)
    cams = np.fromfile(tmp_path / "camera.bin", dtype=np.uint32)
    assert info["polygons"] == len(polys) == len(want["polygons"]) > 1000 and info["points0"] == want["per_camera"][0]["points"]
    assert np.array_equal(polys, want["polygons"]) and np.array_equal(cams, want["camera"])
    img = mesh.depth_image(gpu_device, dev_surface, s.image_dims, 0, -1.0, want["polygons"])
    got = np.fromfile(tmp_path / "map.bin", dtype=np.float64).reshape(info["height"], info["width"])
    assert got.shape == img["map"].shape and got.tobytes() == img["map"].tobytes()
    assert (info["min_x"], info["min_y"]) == img["origin"] and (info["min_depth"], info["max_depth"]) == (img["min_depth"], img["max_depth"])
