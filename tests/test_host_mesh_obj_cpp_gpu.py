"""The OBJ writer through the C++ host layer (cybervision_amd/csrc/host/cvhip_host.hpp, namespace mesh: mesh_obj,
mesh_obj_mtl) on a real GPU: a g++-built program writes the Plain, Color and Texture file images of obj_scenes.scene() and the
.mtl text; each must equal tests/ref_obj.py byte for byte."""
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import obj_scenes
import ref_obj
from ply_scenes import SCALE

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_cpp_host_mesh_obj(gpu_device, tmp_path):
    exe = tmp_path / "host_mesh_obj"
    lib_dir = ROOT / "cybervision_amd"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", str(exe), str(ROOT / "tests" / "cpp" / "host_mesh_obj.cpp"),
                           f"-L{lib_dir}", "-lcvhip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    points, tracks, polys, camera, images = obj_scenes.scene()
    keep = np.r_[0:3000, 12941:15000, 25851:28000]          # polygons of all three cameras
    polys, camera = np.ascontiguousarray(polys[keep]), np.ascontiguousarray(camera[keep])
    assert set(camera.tolist()) == {0, 1, 2}
    points.tofile(tmp_path / "points.bin")
    tracks.tofile(tmp_path / "tracks.bin")
    polys.tofile(tmp_path / "polygons.bin")
    camera.tofile(tmp_path / "cameras.bin")
    np.concatenate([im.reshape(-1) for im in images]).tofile(tmp_path / "images.bin")
    np.array([[im.shape[1], im.shape[0]] for im in images], dtype=np.uint32).tofile(tmp_path / "dims.bin")
    np.array(SCALE).tofile(tmp_path / "scale.bin")
    res = subprocess.run([str(exe), str(tmp_path), str(len(points)), "3"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    info = json.loads(res.stdout.strip().splitlines()[-1])
    want = {name: ref_obj.obj_bytes(points, tracks, images, mode, SCALE, polys, camera, "scene")
            for name, mode in (("plain", ref_obj.PLAIN), ("color", ref_obj.COLOR), ("texture", ref_obj.TEXTURE))}
    assert (tmp_path / "plain.obj").read_bytes() == want["plain"] and info["plain"] == len(want["plain"])
    assert (tmp_path / "color.obj").read_bytes() == want["color"] and info["color"] == len(want["color"])
    assert (tmp_path / "scene.obj").read_bytes() == want["texture"] and info["texture"] == len(want["texture"])
    assert info["sections"] == ref_obj.obj_sections(want["texture"], ref_obj.TEXTURE)
    assert (tmp_path / "scene.mtl").read_bytes() == ref_obj.mtl_bytes("scene", 3)
