"""The TIFF encoder through the C++ host layer (cybervision_amd/csrc/host/cvhip_host.hpp, namespace mesh: tiff_encode) on a
real GPU: a g++-built program writes the file of one scene per compression; it must equal tests/ref_tiff_out.py byte for byte."""
import json
import subprocess
from pathlib import Path

import pytest

import tiff_out_scenes as S

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_cpp_host_tiff_out(gpu_device, tmp_path):
    exe = tmp_path / "host_tiff_out"
    lib_dir = ROOT / "cybervision_amd"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", str(exe), str(ROOT / "tests" / "cpp" / "host_tiff_out.cpp"),
                           f"-L{lib_dir}", "-lcvhip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    for name in ("short_last_strip_lzw", "pb_rgba_sparse", "two_strips_raw_rgb"):
        pixels, compression, predictor, rps = S.scene(name)
        want, st, sections = S.expected(name)
        pixels.tofile(tmp_path / "pixels.bin")
        h, w, c = pixels.shape
        res = subprocess.run([str(exe), str(tmp_path / "pixels.bin"), str(w), str(h), str(c), str(compression), str(predictor), str(rps),
                              str(tmp_path / "out.tif")], capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stderr
        info = json.loads(res.stdout.strip().splitlines()[-1])
        assert (tmp_path / "out.tif").read_bytes() == want
        assert info == {"size": len(want), "sections": list(sections), "stats": [st["strips"], st["codes"], st["clears"], st["packets"]]}
