"""The mesh output through the C++ host layer (cybervision_amd/csrc/host/cvhip_host.hpp, namespace mesh: ply, colour_map) on
a real GPU: a g++-built program writes the Plain and the Color file image of tests/mesh_scenes.py's scene(3) and the RGBA of
a depth map; each must equal the ctypes path byte for byte."""
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ref_ply
import ply_scenes as scenes
from cybervision_amd import mesh

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_cpp_host_mesh_output(gpu_device, tmp_path):
    exe = tmp_path / "host_mesh_output"
    lib_dir = ROOT / "cybervision_amd"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", str(exe), str(ROOT / "tests" / "cpp" / "host_mesh_output.cpp"),
                           f"-L{lib_dir}", "-lcvhip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    points, tracks, polys, images = scenes.scene()
    polys = np.ascontiguousarray(polys[:5001])
    rng = np.random.default_rng(21)
    depth = rng.uniform(1.0, 4.0, (97, 131))
    depth[rng.random(depth.shape) < 0.3] = np.nan
    lo, hi = float(np.nanmin(depth)), float(np.nanmax(depth))
    table = ref_ply.generated_table()
    points.tofile(tmp_path / "points.bin")
    tracks.tofile(tmp_path / "tracks.bin")
    polys.tofile(tmp_path / "polygons.bin")
    np.concatenate([im.reshape(-1) for im in images]).tofile(tmp_path / "images.bin")
    np.array([[im.shape[1], im.shape[0]] for im in images], dtype=np.uint32).tofile(tmp_path / "dims.bin")
    np.array(scenes.SCALE).tofile(tmp_path / "scale.bin")
    depth.tofile(tmp_path / "map.bin")
    np.array([depth.shape[1], depth.shape[0]], dtype=np.uint32).tofile(tmp_path / "mapdims.bin")
    np.array([lo, hi]).tofile(tmp_path / "minmax.bin")
    table.tofile(tmp_path / "table.bin")
    res = subprocess.run([str(exe), str(tmp_path), str(len(points)), "3"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    info = json.loads(res.stdout.strip().splitlines()[-1])
    sf = scenes.surface_of(points, tracks)
    sections = []
    plain = mesh.ply(gpu_device, sf, polys, None, mesh.VertexMode.Plain, scenes.SCALE)
    color = mesh.ply(gpu_device, sf, polys, images, mesh.VertexMode.Color, scenes.SCALE, sections=sections)
    assert (tmp_path / "plain.ply").read_bytes() == plain.tobytes() and info["plain"] == len(plain)
    assert (tmp_path / "color.ply").read_bytes() == color.tobytes() and info["color"] == len(color) > len(plain)
    assert [info["color_header"], info["color_vertices"], info["color_faces"]] == sections
    rgba = mesh.colour_map(gpu_device, depth, lo, hi, table)
    assert (tmp_path / "rgba.bin").read_bytes() == rgba.tobytes() and info["rgba"] == rgba.size
